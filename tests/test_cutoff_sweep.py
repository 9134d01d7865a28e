"""Filter cutoff sweeps in repeated fragments: a2amd_fragment_repeat[_noise] with filter12 cutoffs ramping, the
coefficients made on the device (a2amd_cutsweep.hip) - the ramper arithmetic on the CPU against a restatement of
a2_dsp.h:128-155 and the oracle's f12_pitch2coeff, the rendering bit for bit against the oracle driven fragment by
fragment through Scene.walk()."""
import ctypes
import os
import re

import numpy as np
import pytest

from audiality2_amd import synth
from audiality2_amd.synth import fix
from conftest import ROOT, make_gpu, make_oracle

M32 = 0xFFFFFFFF
EUNSUPPORTED, ESTATE = -4, -5
NONE = -0x7F7F7F80          # A2AMD_SWEEP_NONE, (int32_t)0x80808080
SR = 48000


def i32(x):
    x &= M32
    return x - (1 << 32) if x & 0x80000000 else x


def cdiv(a, b):
    """C's integer division: towards zero"""
    q = abs(a) // abs(b)
    return -q if (a < 0) != (b < 0) else q


# ---- a2_dsp.h:128-170 on a list [value, target, delta, timer] ------------------------------
def prepare(r, frames):
    if not r[3]:
        r[0], r[2] = r[1], 0
    elif frames <= (r[3] >> 8):
        r[2] = i32(cdiv(i32(r[1] - r[0]) << 8, r[3]))
        r[3] = i32(r[3] - (frames << 8))
    else:
        r[2] = cdiv(i32(r[1] - r[0]), frames)
        r[3] = 0


def run(r, frames):
    r[0] = i32(r[0] + r[2] * frames)


def set_ramper(r, target, start, dur):
    r[1] = i32(target << 8)
    r[3] = i32(dur + start)
    if r[3] < 256:
        r[0] = r[1]
    else:
        r[0] = i32(r[0] + (i32(r[2] * start) >> 8))


class Ref:
    """the head of f12_process (filter12.c:87-96), window by window, with the oracle's own table and coefficient"""

    def __init__(self, oracle_lib):
        self.tab = (ctypes.c_uint32 * 128)()
        oracle_lib.a2o_build_pitch_table(self.tab)
        oracle_lib.a2o_f12_coeff.restype = ctypes.c_int
        oracle_lib.a2o_f12_coeff.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.c_int, ctypes.c_int]
        self.coeff = lambda value: int(oracle_lib.a2o_f12_coeff(self.tab, value, SR))

    def sweep(self, r, frames, count):
        out = []
        for _ in range(count):
            prepare(r, frames)
            if r[2]:
                run(r, frames)
                out.append(self.coeff(r[0]))
            else:
                out.append(NONE)
        return out


def lib_sweep(lib, tab, r, frames, count):
    """a2amd_cutoff_sweep: the ramper in and out, the coefficients"""
    lib.a2amd_cutoff_sweep.restype = ctypes.c_int
    lib.a2amd_cutoff_sweep.argtypes = [ctypes.POINTER(ctypes.c_int32), ctypes.c_uint, ctypes.c_uint,
                                       ctypes.POINTER(ctypes.c_uint32), ctypes.c_int, ctypes.POINTER(ctypes.c_int32)]
    rr = (ctypes.c_int32 * 4)(*r)
    coef = (ctypes.c_int32 * max(count, 1))()
    n = lib.a2amd_cutoff_sweep(rr, frames, count, tab, SR, coef)
    r[:] = list(rr)
    got = list(coef)[:count]
    assert n == sum(c != NONE for c in got)
    return got


# ---- CPU ---------------------------------------------------------------------------------
def test_header_and_exports(gpu_lib):
    text = open(os.path.join(ROOT, "include", "a2amd_sweep.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(a2amd_[a-z_0-9]+)\s*\(", text)))
    assert syms == ["a2amd_cutoff_sweep", "a2amd_last_batch_sweeps"]
    for s in syms:
        assert hasattr(gpu_lib, s), f"liba2amd.so lacks {s}"
    assert '#include "a2amd_sweep.h"' in open(os.path.join(ROOT, "include", "a2amd.h")).read()


def rampers(frames):
    """(name, ramper, windows, [(window, target, start, dur) rewrites])"""
    P = lambda octaves: i32(fix(octaves) << 8)      # a ramper value: 16:16 pitch << 8
    span = frames << 8
    out = []
    rng = np.random.default_rng(frames)
    for k in range(40):
        v, t = (int(x) for x in rng.integers(-6 << 24, 9 << 24, 2))
        out.append((f"random{k}", [v, t, int(rng.integers(-5000, 5000)), int(rng.integers(0, 30 * span))], 24, []))
    out.append(("boundary", [P(1.0), P(4.25), 0, 6 * span], 12, []))
    out.append(("inside", [P(3.0), P(-1.5), 0, 5 * span + (13 << 8) + 0x5b], 12, []))
    out.append(("snap first", [P(2.0) - 777, P(2.0), -31, 0], 6, []))
    out.append(("snap first, then a ramp", [P(2.0) + 5, P(2.0), 12, 0], 12, [(3, fix(3.5), 0x80, 4 * span)]))
    # 48 kHz: the coefficient is pinned above 12 kHz, 5.52 octaves over middle C
    out.append(("plateau and back", [P(4.0), P(7.5), 0, 9 * span + 0x33], 24, [(11, fix(3.0), 0x1c0, 8 * span)]))
    out.append(("below octave 0", [P(-0.25), P(-9.0), 0, 14 * span + 99], 20, []))
    out.append(("from below octave 0", [P(-12.5), P(0.5), 0, 7 * span], 12, []))
    out.append(("at rest", [P(1.0), P(1.0), 0, 0], 4, []))
    out.append(("timer without a way to go", [P(1.0), P(1.0), 0, 3 * span], 6, []))
    return out


@pytest.mark.parametrize("frames", [64, 37])
def test_cutoff_sweep_equals_the_reference_ramper(gpu_lib, oracle_lib, frames):
    ref = Ref(oracle_lib)
    seen = set()
    for name, r0, windows, rewrites in rampers(frames):
        a, b = list(r0), list(r0)
        at = 0
        for w, target, start, dur in rewrites + [(windows, 0, 0, 0)]:
            want = ref.sweep(a, frames, w - at)
            got = lib_sweep(gpu_lib, ref.tab, b, frames, w - at)
            assert got == want, (name, at, got, want)
            assert a == b, (name, at, a, b)
            seen.update(("moved" if c != NONE else "still") for c in want)
            seen.update("plateau" for c in want if c == 362 << 16)
            at = w
            if w < windows:
                set_ramper(a, target, start, dur)
                set_ramper(b, target, start, dur)
    assert seen == {"moved", "still", "plateau"}
    # one window at a time is the same as all at once
    r1, r2 = [i32(fix(2.0) << 8), i32(fix(5.0) << 8), 0, (7 * frames + 3) << 8], None
    r2 = list(r1)
    whole = lib_sweep(gpu_lib, ref.tab, r1, frames, 10)
    steps = [lib_sweep(gpu_lib, ref.tab, r2, frames, 1)[0] for _ in range(10)]
    assert whole == steps and r1 == r2


# ---- GPU ---------------------------------------------------------------------------------
def first_diff(a, b):
    if a.shape != b.shape:
        return ("shape", a.shape, b.shape)
    bad = np.argwhere(a != b)
    if not len(bad):
        return None
    ch, fr = bad[np.argmin(bad[:, 1])]
    return int(ch), int(fr), int(a[ch, fr]), int(b[ch, fr])


LOUD = 48


def sweep_scene(be):
    """root; a group whose voice filters its bus (inline; filter12 2 -> 2); 72 + 6 wtosc-filter12-panmix voices, 2 x
    wtosc-filter12-panmix voices, a chain outside the classes (wtosc; filter12; filter12; panmix) - sc.swept: the filter
    units that will sweep, in walk order; the six voices and two of the 2 x wtosc ones stay settled in between"""
    sc = synth.Scene(be)
    sc.root()
    key = sc._key()
    gu = [be.unit_init(key, synth.K_INLINE, 0, 0, 2, 0), be.unit_init(key, synth.K_FILTER12, synth.PROCADD, 2, 2, 1)]
    be.unit_write(gu[1], 0, fix(3.0))
    be.unit_write(gu[1], 1, fix(2.0))
    grp = dict(units=gu, leaves=[])
    sc.groups.append(grp)
    sc.add_voices(3, "osc-pan", group=grp, total=LOUD)
    sc.swept = [gu[1]]
    sc.add_voices(32, "osc-filter-pan", total=LOUD)
    sc.swept += [u[1] for u in sc.leaves[-32:]]
    sc.add_voices(3, "osc-filter-pan", total=LOUD)                  # settled
    sc.add_voices(5, "osc2-filter-pan", total=LOUD)
    sc.swept += [u[2] for u in sc.leaves[-5:-2]]                    # (the last two: settled)
    key = sc._key()
    odd = [be.unit_init(key, synth.K_WTOSC, 0, 0, 1, 0), be.unit_init(key, synth.K_FILTER12, 0, 1, 1, 0),
           be.unit_init(key, synth.K_FILTER12, 0, 1, 1, 0), be.unit_init(key, synth.K_PANMIX, synth.PROCADD, 1, 2, 1)]
    be.unit_write(odd[0], 0, sc.wave_ids[5])
    be.unit_write(odd[0], 1, fix(-0.5))
    be.unit_write(odd[0], 2, fix(0.06))
    for f, cut in ((odd[1], 2.0), (odd[2], 4.0)):
        be.unit_write(f, 0, fix(cut))
        be.unit_write(f, 1, fix(3.0))
    be.unit_write(odd[3], 1, fix(0.3))
    sc.leaves.append(odd)
    sc.swept += odd[1:3]
    sc.add_voices(40, "osc-filter-pan", total=LOUD)
    sc.swept += [u[1] for u in sc.leaves[-40:]]
    sc.add_voices(3, "osc-filter-pan", total=LOUD)                  # settled
    sc.late = [u[1] for u in sc.leaves[-3:-1]]                      # ... until a later walked fragment
    return sc


def start_ramps(be, sc, frames):
    """the seven kinds, dealt over the filters in walk order"""
    F = frames << 8
    for i, f in enumerate(sc.swept):
        kind = i % 7
        if kind == 0:       # longer than all batches
            be.unit_write(f, 0, fix(5.0), 0, 1000 * F)
        elif kind == 1:     # ends on a fragment boundary inside the first stretch
            be.unit_write(f, 0, fix(0.5), 0, 4 * F)
        elif kind == 2:     # ends inside a fragment, with subsample bits
            be.unit_write(f, 0, fix(4.5), 0, 3 * F + (17 << 8) + 0x40)
        elif kind == 3:     # no ramp: an R_F1SET record, not listed
            be.unit_write(f, 0, fix(2.75), 0, 200)
        elif kind == 4:     # a start inside the fragment
            be.unit_write(f, 0, fix(1.25), (5 << 8) + 0x80, 6 * F)
        elif kind == 5:     # rewritten in flight later
            be.unit_write(f, 0, fix(6.0), 0, 30 * F)
        else:               # through the plateau (12 kHz: 5.52 octaves) within the second batch
            be.unit_write(f, 0, fix(7.5), 0, 12 * F + 77)


def rewrite_ramps(be, sc, frames):
    F = frames << 8
    for i, f in enumerate(sc.swept):
        if i % 7 == 5:
            be.unit_write(f, 0, fix(-1.5), 0x55, 4 * F + 0x99)
        elif i % 7 == 6 and i % 2:
            be.unit_write(f, 0, fix(2.0), 0, 5 * F)               # ... and back
    for f in sc.late:       # new columns beside the old ones
        be.unit_write(f, 0, fix(4.0), 0, 9 * F)


def play(be, sc, repeat, frames, rest_of=None):
    """the four batches; repeat: stretches through fragment_repeat, else every fragment walked"""
    got, info = [], []

    def rest(n):
        if repeat:
            (rest_of or be.fragment_repeat)(frames, n)
        else:
            for _ in range(n):
                sc.walk(frames)

    def snap(n):
        got.append(be.render(n * frames))
        if repeat:
            info.append(be.last_batch_sweeps())

    start_ramps(be, sc, frames)
    sc.walk(frames)
    rest(7)
    snap(8)
    rest(8)                         # a whole batch of repeats
    snap(8)
    sc.walk(frames)
    rest(3)
    rewrite_ramps(be, sc, frames)
    sc.walk(frames)
    rest(3)
    snap(8)
    rest(1)
    snap(1)
    return got, info


@pytest.mark.gpu
@pytest.mark.parametrize("frames", [64, 37])
@pytest.mark.parametrize("win,nofast", [("1", "0"), ("0", "0"), ("1", "255")])
def test_parity_with_the_oracle(oracle_lib, monkeypatch, win, nofast, frames):
    """(win: k_win_ctl or k_leaf_recs; nofast=255: every voice through the general kernel, k_voices)"""
    monkeypatch.setenv("A2AMD_WIN", win)
    monkeypatch.setenv("A2AMD_NO_FAST", nofast)
    gpu, ora = make_gpu(max_batch=8), make_oracle(oracle_lib)
    a, info = play(gpu, sweep_scene(gpu), True, frames)
    b, _ = play(ora, sweep_scene(ora), False, frames)
    gpu.close()
    ora.close()
    for k, (x, y) in enumerate(zip(a, b)):
        assert first_diff(x, y) is None, f"batch {k}: (ch, frame, gpu, oracle) = {first_diff(x, y)}"
        assert np.abs(x).max() > 0
    # the lists run past a wavefront: of the 78 filters written to, one in seven is set without a ramp
    assert info[0].pass_launched == 1 and info[0].filters >= 65, info[0]
    assert all(i.pass_launched == 1 and i.filters > 0 and i.ramp_windows > 0 for i in info), info


def noise_sweep_scene(be):
    sc = synth.Scene(be)
    sc.root()
    sc.add_voices(4, "osc-pan", total=LOUD)
    sc.add_voices(11, "noisefilt-pan", total=LOUD)
    sc.noisy = sc.leaves[-11:]
    sc.add_voices(3, "osc-filter-pan", total=LOUD)
    sc.swept = [u[1] for u in sc.noisy[::2]] + [sc.leaves[-2][1]]      # six of the noise voices, one wave voice
    return sc


@pytest.mark.gpu
def test_noise_and_sweeps_together(oracle_lib, monkeypatch):
    """fragment_repeat_noise: seeds and coefficients both from tables; only the settled noise-filter voices are quiet"""
    monkeypatch.setenv("A2AMD_NZF_MIN", "1")
    res, quiet, info = [], [], []
    for repeat in (True, False):
        be = make_gpu(max_batch=8) if repeat else make_oracle(oracle_lib)
        be.noise.value = 0x2545F491
        sc = noise_sweep_scene(be)
        got = []

        def rest(n):
            if repeat:
                be.fragment_repeat_noise(64, n)
            else:
                for _ in range(n):
                    sc.walk(64)

        def snap(n):
            got.append((be.render(n * 64), be.noise.value))
            if repeat:
                quiet.append(be.last_batch_noise_filter())
                info.append(be.last_batch_sweeps())

        for i, f in enumerate(sc.swept):
            be.unit_write(f, 0, fix(5.5 if i % 2 else -0.5), 0, (1000 if i != 1 else 11) * (64 << 8) + 0x21)
        sc.walk(64)
        rest(7)
        snap(8)
        rest(8)
        snap(8)
        sc.walk(64)
        rest(3)
        snap(4)
        rest(8)                     # the short ramp has snapped: its voice is quiet again
        snap(8)
        res.append(got)
        be.close()
    for k, ((a, na), (b, nb)) in enumerate(zip(*res)):
        assert first_diff(a, b) is None, f"batch {k}: (ch, frame, gpu, oracle) = {first_diff(a, b)}"
        assert na == nb, f"batch {k}: noise word {na:#x} against the oracle's {nb:#x}"
    # batch 1, repeats only: no noise voice has a record - the five settled ones are k_leaf_noisefiltpan's, the six
    # with a listed filter are not
    assert (quiet[1].quiet_launched, quiet[1].quiet_voices, quiet[1].class_voices) == (1, 5, 11), quiet[1]
    assert (info[1].filters, info[1].standin_voices) == (7, 7), info[1]
    assert (quiet[3].quiet_voices, info[3].filters) == (6, 6), (quiet[3], info[3])


def small_scene(be):
    sc = synth.Scene(be)
    sc.root()
    sc.add_voices(3, "osc-filter-pan", total=8)
    return sc


@pytest.mark.gpu
def test_counters(gpu_lib, oracle_lib):
    from test_gpu_parity import last_batch
    ref = Ref(oracle_lib)
    gpu, ora = make_gpu(max_batch=8), make_oracle(oracle_lib)
    sg, so = small_scene(gpu), small_scene(ora)
    lib = gpu.lib
    lib.a2amd_fragment_repeat.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint]

    def batch(walked, repeats):
        for _ in range(walked):
            sg.walk(64)
        assert lib.a2amd_fragment_repeat(gpu.ctx, 64, repeats) == 0
        for _ in range(walked + repeats):
            so.walk(64)
        a, b = gpu.render((walked + repeats) * 64), ora.render((walked + repeats) * 64)
        assert first_diff(a, b) is None, first_diff(a, b)
        return gpu.last_batch_sweeps()

    # nothing sweeps: no list, no table, no launch
    bi = batch(1, 7)
    assert (bi.pass_launched, bi.filters, bi.ramp_windows, bi.standin_voices) == (0, 0, 0, 0), bi
    # one ramp in flight (a refusal before): 10 fragments and 20 frames, written in a walked fragment
    f = sg.leaves[1][1]
    cut0 = fix(((1 % 61) - 30) / 12.0) + fix(2.0)          # (Scene.add_voices: voice 1's cutoff)
    r = [i32(cut0 << 8), i32(cut0 << 8), 0, 0]
    for be, sc in ((gpu, sg), (ora, so)):
        be.unit_write(sc.leaves[1][1], 0, fix(4.0), 0, (10 * 64 + 20) << 8)
    set_ramper(r, fix(4.0), 0, (10 * 64 + 20) << 8)
    assert lib_sweep(gpu_lib, ref.tab, r, 64, 1) != [NONE]  # the walked fragment
    want = lib_sweep(gpu_lib, ref.tab, r, 64, 7)
    bi = batch(1, 7)
    assert (bi.pass_launched, bi.filters, bi.ramp_windows, bi.standin_voices) == (1, 1, 7, 0), bi
    assert sum(c != NONE for c in want) == 7
    # a batch of repeats alone: the voice has no record - the stand-in run; the ramp ends in it (two whole windows, the
    # one it ends in; the next only snaps)
    want = lib_sweep(gpu_lib, ref.tab, r, 64, 8)
    assert sum(c != NONE for c in want) == 3 and r[2] == 0 and r[0] == r[1] and r[3] == 0
    bi = batch(0, 8)
    assert (bi.pass_launched, bi.filters, bi.ramp_windows, bi.standin_voices) == (1, 1, 3, 1), bi
    assert last_batch(gpu).n_moving_listed == 1
    # the ramper has snapped: nothing is listed, the voice is its quiet kernel's again
    bi = batch(0, 8)
    assert (bi.pass_launched, bi.filters, bi.ramp_windows, bi.standin_voices) == (0, 0, 0, 0), bi
    assert last_batch(gpu).n_moving_listed == 0
    gpu.close()
    ora.close()


@pytest.mark.gpu
def test_refusals_leave_the_recording_alone(oracle_lib):
    gpu, ora = make_gpu(max_batch=8), make_oracle(oracle_lib)
    sg, so = small_scene(gpu), small_scene(ora)
    lib = gpu.lib
    lib.a2amd_fragment_repeat.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint]

    def both(f):
        for be, sc in ((gpu, sg), (ora, so)):
            f(be, sc)

    def same(frames):
        a, b = gpu.render(frames), ora.render(frames)
        assert first_diff(a, b) is None, first_diff(a, b)

    both(lambda be, sc: be.unit_write(sc.leaves[0][1], 0, fix(4.5), 0, 1000 * (64 << 8)))
    both(lambda be, sc: sc.walk(64))
    gpu.fragment_repeat(64, 2)
    [so.walk(64) for _ in range(2)]
    # a write to the sweeping filter's voice between two stretches belongs to a fragment walked by calls
    both(lambda be, sc: be.unit_write(sc.leaves[0][1], 1, fix(2.0)))
    assert lib.a2amd_fragment_repeat(gpu.ctx, 64, 2) == ESTATE
    both(lambda be, sc: sc.walk(64))
    same(4 * 64)
    # KEEP / replay of a batch with a sweep table
    both(lambda be, sc: sc.walk(64))
    gpu.fragment_repeat(64, 2)
    [so.walk(64) for _ in range(2)]
    with pytest.raises(RuntimeError, match="sweep"):
        gpu.render(3 * 64, phases=15 | 16)
    gpu.render(3 * 64, phases=4)           # (upload only)
    assert lib.a2amd_replay(gpu.ctx, 1) == EUNSUPPORTED
    a = gpu.render(3 * 64, phases=1 | 2 | 8)
    b = ora.render(3 * 64)
    assert first_diff(a, b) is None, first_diff(a, b)
    # the following fragments, walked by calls
    for _ in range(2):
        both(lambda be, sc: [sc.walk(64) for _ in range(3)])
        same(3 * 64)
    gpu.close()
    ora.close()
