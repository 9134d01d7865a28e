"""k_leaf_noisefiltpan: settled wtosc (noise) -> filter12 -> panmix voices of a batch with device-seeded fragments in a
quiet kernel of their own (a2amd_noisefiltpan.hip) - its arithmetic on the CPU against the sample loops of wtosc.c:140-150
and filter12.c:97-118, the rendering bit for bit against the oracle walked fragment by fragment, and who rendered what
(a2amd_last_batch_noise_filter, a2amd_last_batch_noise)."""
import ctypes
import os
import re

import numpy as np
import pytest

from audiality2_amd import synth
from conftest import ROOT, make_gpu, make_oracle
from test_noise_quiet import B23, _both, _tools, compare, noise_pitch, p2i, regimes
from test_noise_repeat import M32, SEED0, lcg


# ---- CPU ---------------------------------------------------------------------------------
def i32(x):
    x &= M32
    return x - (1 << 32) if x & 0x80000000 else x


def _window(lib):
    i, u, p = ctypes.c_int32, ctypes.c_uint32, ctypes.POINTER
    lib.a2amd_noise_filter_window.restype = u
    lib.a2amd_noise_filter_window.argtypes = [u, ctypes.c_uint64, u, i, i, i, i, i, i, i, p(i), p(i), ctypes.c_uint, p(i), p(u), p(i)]
    buf, after, hafter = (i * 64)(), u(0), i(0)

    def window(seed, phase, dphase, held, avalue, qvalue, f1, mix, d1, d2, frames):
        c1, c2 = i(d1), i(d2)
        n = lib.a2amd_noise_filter_window(seed, phase, dphase, held, avalue, qvalue, f1, mix[0], mix[1], mix[2],
                                          ctypes.byref(c1), ctypes.byref(c2), frames, buf, ctypes.byref(after), ctypes.byref(hafter))
        return list(buf[:frames]), n, after.value, hafter.value, c1.value, c2.value

    return window


def window_by_sample(seed, phase, dphase, held, avalue, qvalue, f1, mix, d1, d2, frames):
    """wtosc.c:140-150 with a2_Noise (a2_dsp.h:37-42), then f12_process's loop body (filter12.c:97-118: one channel, no cutoff
    ramp, q at rest), frame by frame; every +, -, * an int32 operation that wraps, every >> arithmetic.  The filter's
    output, the draws, the generator word, the held sample and d1 / d2 afterwards."""
    lp, bp, hp = mix
    out, n = [], 0
    f, q = f1 >> 12, qvalue >> 12
    for _ in range(frames):
        nph = (phase + dphase) & ((1 << 64) - 1)
        if dphase >= B23 or ((nph ^ phase) >> 23):
            seed = (seed * 1566083941 + 1) & M32
            held = i32(((seed * (seed >> 16)) & M32) >> 16) - 32767
            n += 1
        phase = nph
        x = i32(held * (avalue >> 10)) >> 6
        s1 = d1 >> 4
        lo = i32(d2 + (i32(f * s1) >> 8))
        hi = i32(i32((x >> 5) - lo) - (i32(q * s1) >> 8))
        b = i32((i32(f * (hi >> 4)) >> 8) + d1)
        out.append(i32(i32(i32(lo * lp) + i32(b * bp)) + i32(hi * hp)) >> 3)
        d1, d2 = b, lo
    return out, n, seed, held, d1, d2


F1S = [1000, 5 << 16, 100 << 16, 300 << 16, 362 << 16]                  # (f12_pitch2coeff's range and its clamp value)
QS = [32768 << 8, ((65536 << 8) // synth.fix(4.0)) << 8, ((65536 << 8) // 655) << 8, ((65536 << 8) // synth.fix(20.0)) << 8]
MIXES = [(256, 0, 0), (128, 77, -50), (0, 256, 0), (64, 0, 200)]


def _filter_state(rng):
    return dict(avalue=int(rng.integers(0, 1 << 25)), qvalue=QS[int(rng.integers(len(QS)))], f1=F1S[int(rng.integers(len(F1S)))],
                mix=MIXES[int(rng.integers(len(MIXES)))], d1=int(rng.integers(-(1 << 27), 1 << 27)),
                d2=int(rng.integers(-(1 << 27), 1 << 27)))


def test_header_and_exports(gpu_lib):
    text = open(os.path.join(ROOT, "include", "a2amd_noisefilt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(a2amd_[a-z_0-9]+)\s*\(", text)))
    assert syms == ["a2amd_last_batch_noise_filter", "a2amd_noise_filter_window"]
    for s in syms:
        assert hasattr(gpu_lib, s), f"liba2amd.so lacks {s}"
    assert '#include "a2amd_noisefilt.h"' in open(os.path.join(ROOT, "include", "a2amd.h")).read()


def test_noise_filter_window_equals_the_sample_loop(gpu_lib):
    window = _window(gpu_lib)
    dphases = [1, 255, 0x594d, B23 // 3, B23 // 2, B23 - 2, B23 - 1, B23, B23 + 1, 2 * B23, 0x165373c, M32]
    phases = [0, 1, B23 - 1, B23 - 2, 5 * B23 - 1, 5 * B23, 5 * B23 + 1, 1000 * B23 - 3, (1 << 32) - 1, (1 << 32),
              (1 << 40) + B23 - 1, 977 * B23 - 0x594d]
    rng = np.random.default_rng(5)
    checked = 0
    for d in dphases:
        for ph in phases:
            for frames in range(1, 65):
                seed, held = int(rng.integers(0, 1 << 32)), int(rng.integers(-40000, 40000))
                st = _filter_state(rng)
                assert window(seed, ph, d, held, frames=frames, **st) == window_by_sample(seed, ph, d, held, frames=frames, **st), \
                    (seed, ph, d, held, frames, st)
                checked += 1
    assert checked == len(dphases) * len(phases) * 64
    # every coefficient, q and mix against every other, full windows
    for f1 in F1S:
        for q in QS:
            for mix in MIXES:
                seed, held = int(rng.integers(0, 1 << 32)), int(rng.integers(-40000, 40000))
                st = dict(_filter_state(rng), f1=f1, qvalue=q, mix=mix)
                ph, d = int(rng.integers(0, 1 << 48)), int(rng.integers(1, 1 << 25))
                assert window(seed, ph, d, held, frames=64, **st) == window_by_sample(seed, ph, d, held, frames=64, **st), (seed, ph, d, st)


def test_consecutive_windows_telescope(gpu_lib):
    window = _window(gpu_lib)
    rng = np.random.default_rng(6)
    for d in [1, 0x594d, 22861, B23 // 3, B23 - 1, B23, 3 * B23] + [int(x) for x in rng.integers(1, 1 << 25, 40)]:
        for _ in range(6):
            ph, seed, held = int(rng.integers(0, 1 << 48)), int(rng.integers(0, 1 << 32)), int(rng.integers(-40000, 40000))
            st = _filter_state(rng)
            whole = window(seed, ph, d, held, frames=64, **st)
            a = window(seed, ph, d, held, frames=23, **st)
            b = window(a[2], ph + 23 * d, d, a[3], frames=41, **dict(st, d1=a[4], d2=a[5]))
            assert (a[0] + b[0], a[1] + b[1]) + b[2:] == whole, (seed, ph, d, held, st)


# ---- GPU ---------------------------------------------------------------------------------
N_PAN, N_OTHER = 5, 1


class FiltScene:
    """test_noise_quiet.QuietScene's shape with the roles swapped: n_filt noise-filter-pan voices (synth's chain
    "noisefilt-pan": one voice each) in three blocks - under two delay-bus groups and under the root - with wave
    osc-filter-pan voices, five noise-pan voices and the voice with two noise oscillators between them in walk order:
    both quiet noise kernels read one seed table in one batch.  The first block's filters mix band and high pass in
    (registers 3, 4), the others stay pure low pass."""

    def __init__(self, be, n_filt):
        self.be = be
        sc = self.sc = synth.Scene(be)
        sc.root()
        g1, g2 = sc.add_group(), sc.add_group()
        loud = min(64, n_filt + 40)
        na, nb = n_filt // 3, n_filt // 3
        self.filt, self.filt_ks, self.other_ks = [], [], []

        def noise(n, chain, group, k0):
            sc.nvoices = k0             # (the voice number decides pitch, pan and phase: the blocks start where we say)
            sc.add_voices(n, chain, group=group, total=loud)
            dst = sc.leaves if group is None else group["leaves"]
            (self.filt_ks if chain == "noisefilt-pan" else self.other_ks).extend(range(k0, k0 + n))
            if chain == "noisefilt-pan" and n:
                self.filt.extend(dst[-n:])

        sc.add_voices(4, "osc-filter-pan", group=g1, total=loud)
        noise(na, "noisefilt-pan", g1, 31)
        noise(2, "noise-pan", g1, 17)               # (6.5 octaves up and more: a draw in every frame)
        sc.add_voices(3, "osc2-pan", group=g1, total=loud)
        sc.add_voices(2, "osc-pan", group=g2, total=loud)
        noise(nb, "noisefilt-pan", g2, 31 + na)
        noise(2, "noise-pan", g2, 2)                # (2.67 octaves up: a draw every few frames)
        sc.nvoices = 200
        sc.add_voices(5, "osc-filter-pan", total=loud)
        self.waves = sc.leaves[-5:]
        key = sc._key()
        two = [be.unit_init(key, synth.K_WTOSC, 0, 0, 1, 0), be.unit_init(key, synth.K_WTOSC, synth.PROCADD, 0, 1, 0),
               be.unit_init(key, synth.K_PANMIX, synth.PROCADD, 1, 2, 1)]
        for j, o in enumerate(two[:2]):
            be.unit_write(o, 0, sc.noise_id)
            be.unit_write(o, 1, synth.fix(7.0 if j else 2.25))
            be.unit_write(o, 2, synth.fix(0.05))
        be.unit_write(two[2], 1, synth.fix(-0.25))
        sc.leaves.append(two)
        noise(n_filt - na - nb, "noisefilt-pan", None, 0)    # (voice number 0: two octaves down, the sparsest)
        noise(1, "noise-pan", None, 62)             # (voice number 62 = 0 mod 31: as sparse)
        sc.nvoices = 300
        sc.add_voices(2, "osc-pan", total=loud)
        for j, v in enumerate(self.filt[:na]):
            if j % 3 != 1:
                be.unit_write(v[1], 3, synth.fix(0.5 - 0.125 * (j % 5)))
            if j % 3 != 0:
                be.unit_write(v[1], 4, synth.fix(0.25 * (j % 4) - 0.3))
        self.n_filt = n_filt

    def increments(self, ks):
        tab, base = self.be.get_pitch_table(), synth.basepitch_for(48000)
        return [p2i(tab, noise_pitch(k) + base) for k in ks]


def run_plan(be, repeat, n_filt, short=False):
    """the batch plan; per batch (audio, noise word, (a2amd_last_batch_noise_filter, a2amd_last_batch_noise) or None,
    repeat-only?) - the tuple's first four fields as test_noise_quiet.compare takes them.
    The kernel's branch for a voice without a column in the batch's seed table (it carries the word its last window left)
    has no scene: the kernel is launched only in a batch with device-seeded stretches, a2amd_fragment_repeat_noise gives
    every live noise oscillator a column or refuses the call (A2AMD_ESTATE: test_noise_repeat's refusals), and a voice
    born, switched to noise or killed since meets a fragment walked by calls first, i.e. carries records.  What the branch
    shares with the others - the word stored in OW_SEED and taken up again - is checked where state goes back to the
    window kernels (the pitch and cutoff writes below) and by the noise word compared after every batch."""
    be.noise.value = SEED0
    q = FiltScene(be, n_filt)
    sc = q.sc
    if repeat:
        assert all(regimes(q.increments(q.filt_ks + q.other_ks)))
        if n_filt >= 31 * 3:
            assert all(regimes(q.increments(q.filt_ks)))
        # the sparsest noise-filter voice draws less than once in five fragments
        assert min(q.increments(q.filt_ks)) * 64 * 5 < B23
    got = []

    def rest(n, frames=64):
        if repeat:
            be.fragment_repeat_noise(frames, n)
        else:
            for _ in range(n):
                sc.walk(frames)

    def snap(frames, only):
        a = be.render(frames)
        got.append((a, be.noise.value, (be.last_batch_noise_filter(), be.last_batch_noise()) if repeat else None, only))

    sc.walk(64)
    rest(3)
    snap(4 * 64, False)                 # records for every noise voice
    rest(8)
    snap(8 * 64, True)
    if short:
        rest(1)
        snap(64, True)
        be.close()
        return got, q
    rest(16)
    snap(16 * 64, True)                 # (= max_batch)
    for _ in range(3):                  # one fragment each: the pipeline's prologue and epilogue with nothing between them
        rest(1)
        snap(64, True)
    rest(2)
    snap(2 * 64, True)
    rest(3)
    snap(3 * 64, True)
    rest(2)
    be.noise.value = lcg(be.noise.value, 11)
    rest(5)                             # two stretches in one batch, host draws between them
    snap(7 * 64, True)
    rest(6, 37)
    snap(6 * 37, True)
    # the state the quiet kernel stored goes back to the window kernels: a pitch write, a cutoff write without duration
    be.unit_write(q.filt[0][0], 1, synth.fix(6.75))
    be.unit_write(q.filt[-1][1], 0, synth.fix(2.5))
    sc.walk(64)
    rest(7)
    snap(8 * 64, False)
    rest(8)
    snap(8 * 64, True)
    rest(5)
    snap(5 * 64, True)
    be.close()
    return got, q


_oracle = {}


def oracle_plan(oracle_lib, n_filt, short):
    """the oracle's side of the plan, rendered once per size"""
    if (n_filt, short) not in _oracle:
        _oracle[n_filt, short] = run_plan(make_oracle(oracle_lib), False, n_filt, short)[0]
    return _oracle[n_filt, short]


def _env(monkeypatch, nzf_min="1", vpg=None, **more):
    for k in ("A2AMD_NOISE_QUIET", "A2AMD_NZF_MIN", "A2AMD_NZFVPG"):
        monkeypatch.delenv(k, raising=False)
    if nzf_min is not None:
        monkeypatch.setenv("A2AMD_NZF_MIN", nzf_min)
    if vpg is not None:
        monkeypatch.setenv("A2AMD_NZFVPG", vpg)
    for k, v in more.items():
        monkeypatch.setenv(k, v)


# (n_filt, short plan, A2AMD_NZFVPG): one busy lane in the filter wavefront; the launcher's own shape (a voice per
# workgroup); two workgroups, the second partial, three bus runs; nine workgroups; many small workgroups sharing buses
SIZES = [(1, False, None), (70, True, None), (70, False, "64"), (530, True, "64"), (530, True, "5")]


@pytest.mark.gpu
@pytest.mark.parametrize("n_filt,short,vpg", SIZES)
def test_quiet_kernel_matches_the_oracle(oracle_lib, monkeypatch, n_filt, short, vpg):
    _env(monkeypatch, vpg=vpg)
    got, q = run_plan(make_gpu(max_batch=16), True, n_filt, short)
    for k, (_a, _n, (nf, nz), only) in enumerate(got):
        print(k, only, nf, nz)
    compare(got, oracle_plan(oracle_lib, n_filt, short))
    for k, (_a, _n, (nf, nz), only) in enumerate(got):
        assert nf.min_voices == 1 and nz.class_voices == N_PAN, k
        if only:
            assert (nf.quiet_launched, nf.quiet_voices, nf.class_voices) == (1, n_filt, n_filt), k
            assert (nz.quiet_launched, nz.quiet_voices, nz.standin_voices) == (1, N_PAN, N_OTHER), k
        else:
            assert (nf.quiet_launched, nf.quiet_voices, nf.class_voices) == (0, 0, n_filt), k
            assert (nz.quiet_launched, nz.quiet_voices, nz.standin_voices) == (0, 0, 0), k


@pytest.mark.gpu
def test_threshold(oracle_lib, monkeypatch):
    """A2AMD_NZF_MIN unset: the compiled threshold - that many recordless voices in a batch are the kernel's, one fewer all
    take the stand-in record; the same audio either way"""
    _env(monkeypatch, nzf_min=None)
    be = make_gpu(max_batch=16)
    m = int(be.last_batch_noise_filter().min_voices)
    be.close()
    assert 16 <= m <= 1024
    for n in (m, m - 1):
        got, q = run_plan(make_gpu(max_batch=16), True, n, True)
        compare(got, oracle_plan(oracle_lib, n, True))
        for k, (_a, _n, (nf, nz), only) in enumerate(got):
            assert (nf.class_voices, nf.min_voices) == (n, m), k
            if only and n >= m:
                assert (nf.quiet_launched, nf.quiet_voices, nz.standin_voices) == (1, n, N_OTHER), k
            elif only:
                assert (nf.quiet_launched, nf.quiet_voices, nz.standin_voices) == (0, 0, n + N_OTHER), k
            else:
                assert (nf.quiet_launched, nf.quiet_voices, nz.standin_voices) == (0, 0, 0), k
            assert (nz.quiet_launched, nz.quiet_voices) == ((1, N_PAN) if only else (0, 0)), k


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"A2AMD_NOISE_QUIET": "0"}, {"A2AMD_NO_FAST": "255"}])
def test_switched_off_routes_as_before(oracle_lib, monkeypatch, env):
    """A2AMD_NOISE_QUIET=0, A2AMD_NO_FAST=255: no class, no launch, the stand-in for every noise voice - and the same audio"""
    _env(monkeypatch, **env)
    got, q = run_plan(make_gpu(max_batch=16), True, 70, False)
    compare(got, oracle_plan(oracle_lib, 70, False))
    for k, (_a, _n, (nf, nz), only) in enumerate(got):
        assert (nf.quiet_launched, nf.quiet_voices, nf.class_voices) == (0, 0, 0), k
        assert (nz.quiet_launched, nz.quiet_voices, nz.class_voices) == (0, 0, 0), k
        assert nz.standin_voices == (70 + N_PAN + N_OTHER if only else 0), k


def _infos(infos):
    return [(nf.quiet_launched, nf.quiet_voices, nf.class_voices, nz.quiet_voices, nz.standin_voices) for nf, nz in infos]


def _pairs(be, sc, repeat, got):
    """test_noise_quiet._tools with both batch infos in the third field"""
    rest, _snap = _tools(be, sc, repeat, got)

    def snap(frames):
        got.append((be.render(frames), be.noise.value, (be.last_batch_noise_filter(), be.last_batch_noise()) if repeat else None))

    return rest, snap


@pytest.mark.gpu
def test_gliding_q_keeps_the_stand_in(oracle_lib, monkeypatch):
    """a 700-frame q glide on a noise-filter voice: the window kernels' while it lasts (moving_until), the quiet kernel's after"""
    _env(monkeypatch)

    def script(be, repeat):
        be.noise.value = SEED0
        q = FiltScene(be, 9)
        got = []
        rest, snap = _pairs(be, q.sc, repeat, got)
        be.unit_write(q.filt[4][1], 1, synth.fix(1.5), 0, 700 << 8)
        q.sc.walk(64)
        rest(7)
        snap(8 * 64)            # frames 0 .. 511
        rest(8)
        snap(8 * 64)            # 512 .. 1023: the glide ends at 700
        rest(8)
        snap(8 * 64)            # settled
        rest(3)
        snap(3 * 64)
        return got

    infos = _both(oracle_lib, script)
    assert _infos(infos) == [(0, 0, 9, 0, 0), (1, 8, 9, N_PAN, N_OTHER + 1), (1, 9, 9, N_PAN, N_OTHER), (1, 9, 9, N_PAN, N_OTHER)]


@pytest.mark.gpu
def test_mode_switch_and_death(oracle_lib, monkeypatch):
    _env(monkeypatch)

    def script(be, repeat):
        be.noise.value = SEED0
        q = FiltScene(be, 7)
        sc = q.sc
        got = []
        rest, snap = _pairs(be, sc, repeat, got)
        sc.walk(64)
        rest(3)
        snap(4 * 64)
        rest(8)
        snap(8 * 64)                                    # 7 quiet
        # a wave osc-filter-pan voice becomes a noise voice and joins the class ...
        wave = q.waves[1]
        be.unit_write(wave[0], 0, sc.noise_id)
        sc.walk(64)
        rest(3)
        snap(4 * 64)
        rest(8)
        snap(8 * 64)                                    # 8 quiet
        # ... and a wave voice again: k_leaf_oscfiltpan's
        be.unit_write(wave[0], 0, sc.wave_ids[3])
        sc.walk(64)
        rest(3)
        snap(4 * 64)
        rest(8)
        snap(8 * 64)                                    # 7 quiet
        # a noise-filter voice dies between two batches of repeats (a fragment walked by calls follows the kill)
        dead = q.filt[2]
        for u in dead:
            be.unit_deinit(u)
        for leaves in [sc.leaves] + [g["leaves"] for g in sc.groups]:
            if dead in leaves:
                leaves.remove(dead)
        sc.walk(64)
        rest(3)
        snap(4 * 64)
        rest(8)
        snap(8 * 64)                                    # 6 quiet
        return got

    infos = _both(oracle_lib, script)
    assert _infos(infos) == [
        (0, 0, 7, 0, 0), (1, 7, 7, N_PAN, N_OTHER), (0, 0, 8, 0, 0), (1, 8, 8, N_PAN, N_OTHER), (0, 0, 7, 0, 0), (1, 7, 7, N_PAN, N_OTHER),
        (0, 0, 7, 0, 0), (1, 6, 6, N_PAN, N_OTHER)]     # (a dying voice is listed to the end of its batch)
