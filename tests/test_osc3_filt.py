"""k_leaf_osc3filtpan (a2amd_osc3filtpan.hip): the three-oscillator subtractive lead, `struct { wtosc; wtosc o2; wtosc o3;
filter12; panmix }`, in a quiet kernel of its own in the batches in which it carries no run, settled or gliding.  Every
rendering bit for bit against the oracle's render of the same calls, batch by batch, and every batch with who rendered what
(a2amd_last_batch_osc3filt, include/a2amd_osc3filt.h): a test that names the kernel proves the kernel rendered.

The fixture lead3 (tests/a2s/lead3.a2s, tests/golden/make_lead3_golden.py) is the reference's own rendering of six such
leads under the root.  The root's VM wakes about every 61 fragments and cuts every descendant's fragment there, so at 64
fragments a batch no batch but the last, short one leaves the leads without a record; at 16 fragments a batch 69 of 94 do -
test_fixture_premise states both as facts of the trace, and the GPU replay holds the library to them batch by batch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from audiality2_amd import synth
from audiality2_amd.replay import (T_DEINIT, T_FRAGMENT, T_INIT, T_PROCESS, T_WAVEDROP, T_WRITE, Trace,
                                   a2amd_osc3filt_batch_info, replay)
from conftest import GOLDEN, ROOT, fnv1a_fragments, make_gpu, make_oracle
from test_gpu_parity import first_diff, is_gpu, last_batch

fix = synth.fix
K_WTOSC, K_FILTER12, K_PANMIX, PROCADD = synth.K_WTOSC, synth.K_FILTER12, synth.K_PANMIX, synth.PROCADD
O3 = "osc3-filter-pan"
FIELDS = ("launched", "class_voices", "quiet_voices", "gliding_voices", "record_voices", "vpg", "workgroups", "reserved")
W, P, A, PHASE = 0, 1, 2, 3                     # wtosc registers
CUT, Q, LP, BP, HP = 0, 1, 2, 3, 4              # filter12
VOL, PAN = 0, 1                                 # panmix


# ---- CPU ---------------------------------------------------------------------------------
def test_header_and_exports(gpu_lib):
    text = open(os.path.join(ROOT, "include", "a2amd_osc3filt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(a2amd_[a-z_0-9]+)\s*\(", text)))
    assert syms == ["a2amd_last_batch_osc3filt"]
    for s in syms:
        assert hasattr(gpu_lib, s), f"liba2amd.so lacks {s}"
    assert '#include "a2amd_osc3filt.h"' in open(os.path.join(ROOT, "include", "a2amd.h")).read()
    assert C.sizeof(a2amd_osc3filt_batch_info) == 32
    assert [n for n, _ in a2amd_osc3filt_batch_info._fields_] == list(FIELDS)
    # NULL arguments are refused, not dereferenced
    gpu_lib.a2amd_last_batch_osc3filt.restype = C.c_int
    gpu_lib.a2amd_last_batch_osc3filt.argtypes = [C.c_void_p, C.c_void_p]
    assert gpu_lib.a2amd_last_batch_osc3filt(None, None) != 0


class Recorder:
    """a backend that writes down the unit_init and unit_write calls"""

    def __init__(self):
        self.inits, self.writes, self.nwaves = [], [], 0

    def wave_upload(self, *_a):
        self.nwaves += 1
        return self.nwaves - 1

    def unit_init(self, key, kind, flags, nin, nout, wired, transpose=0, wakefrac=0):
        self.inits.append((key, kind, flags, nin, nout, wired))
        return len(self.inits) - 1

    def unit_write(self, unit, reg, value, start=0, dur=0, transpose=0):
        self.writes.append((unit, reg, value))


def test_synth_chain():
    """add_voices("osc3-filter-pan"): the chain of the class; the third oscillator an octave down; the first two as in
    "osc2-filter-pan" """
    pitches = {}
    for chain in (O3, "osc2-filter-pan"):
        rec = Recorder()
        sc = synth.Scene(rec)
        sc.add_voices(2, chain, total=8)
        pitches[chain] = [[v for u, r, v in rec.writes if u == o and r == P] for o in sc.leaves[1][:3 if chain == O3 else 2]]
        if chain == O3:
            assert [i[1:] for i in rec.inits[:5]] == [(K_WTOSC, 0, 0, 1, 0), (K_WTOSC, PROCADD, 0, 1, 0), (K_WTOSC, PROCADD, 0, 1, 0),
                                                     (K_FILTER12, 0, 1, 1, 0), (K_PANMIX, PROCADD, 1, 2, 1)]
            assert len({i[0] for i in rec.inits[:5]}) == 1 and len(sc.leaves[0]) == 5
    p = fix((1 - 30) / 12.0)
    assert pitches[O3] == [[p + fix(0.01)], [p - fix(0.01)], [p - fix(1.0)]]
    assert pitches[O3][:2] == pitches["osc2-filter-pan"]


@pytest.fixture(scope="module")
def lead3():
    return Trace(os.path.join(GOLDEN, "lead3.trace.xz"))


def lead_voices(tr):
    """the voices of the class from the T_INIT records alone: {voice: its five unit ids}"""
    chains = {}
    for r in tr.records:
        if r[0] == T_INIT:
            chains.setdefault(r[2], []).append((r[1], r[3]))
    return {v: [u for u, _k in us] for v, us in chains.items()
            if [k for _u, k in us] == [K_WTOSC, K_WTOSC, K_WTOSC, K_FILTER12, K_PANMIX]}


def at_rest_voices(tr, voices):
    """... of which never written after their first window: the Lead3 voices (Glide3 writes again 100 ms in)"""
    owner = {u: v for v, us in voices.items() for u in us}
    seen, late = set(), set()
    for r in tr.records:
        if r[0] == T_PROCESS and r[1] in owner:
            seen.add(owner[r[1]])
        elif r[0] == T_WRITE and r[1] in owner and owner[r[1]] in seen:
            late.add(owner[r[1]])
    return sorted(set(voices) - late)


def record_free(tr, voices, batch):
    """per voice, per rendered batch of replay(tr, batch=batch): True where the voice carries no record - no write, init
    or deinit to its units and every Process of them (0, the fragment's frames).  (song_record_free of test_fbd_pan.py,
    for several voices)"""
    owner = {u: v for v, us in voices.items() for u in us}
    out = {v: [] for v in voices}
    free = {v: True for v in voices}
    pending, nfrag, frames = 0, 0, 0

    def close():
        for v in voices:
            out[v].append(free[v])
            free[v] = True

    for r in tr.records:
        op = r[0]
        if op == T_FRAGMENT:
            if pending and nfrag % batch == 0:
                close()
                pending = 0
            frames = r[1]
            pending += frames
            nfrag += 1
        elif op == T_WAVEDROP:
            if pending:
                close()
                pending = 0
        elif op in (T_INIT, T_DEINIT, T_WRITE) and r[1] in owner:
            free[owner[r[1]]] = False
        elif op == T_PROCESS and r[1] in owner and (r[2], r[3]) != (0, frames):
            free[owner[r[1]]] = False
    if pending:
        close()
    return out


def test_fixture_on_the_oracle(oracle_lib, lead3):
    cfg = lead3.config
    ora = make_oracle(oracle_lib, cfg["samplerate"], cfg["basepitch"], cfg["channels"])
    out = replay(lead3, ora, batch=16, check_noise=True)
    ora.close()
    want = np.load(os.path.join(GOLDEN, "lead3.hash.npy"))
    got = fnv1a_fragments(out)
    assert len(want) == 1500 and len(got) == 1500
    assert not np.nonzero(got != want)[0].size
    assert int(np.abs(out).max()) == 19907713


RECORD_BATCHES = [0, 3, 7, 11, 15, 19, 22, 26, 30, 34, 38, 41, 45, 49, 53, 57, 61, 64, 68, 72, 76, 80, 83, 87, 91]


def test_fixture_premise(lead3):
    voices = lead_voices(lead3)
    rest = at_rest_voices(lead3, voices)
    assert (len(voices), len(rest)) == (6, 3)
    free = record_free(lead3, voices, 16)
    for v in rest:
        assert len(free[v]) == 94 and sum(free[v]) >= 60 and not free[v][0], (v, sum(free[v]))
        # the batches in which the root's wake-up (about every 61 fragments) cuts a fragment, and the births: 25 of 94
        assert [b for b, ok in enumerate(free[v]) if not ok] == RECORD_BATCHES
    # the gliding leads write again 100 ms = 4 800 frames in: fragment 75, batch 4
    for v in set(voices) - set(rest):
        assert not free[v][0] and not free[v][4] and all(a or not b for a, b in zip(free[rest[0]], free[v]))
    whole = record_free(lead3, voices, 64)
    for v in rest:
        assert len(whole[v]) == 24 and sum(whole[v]) <= 1, (v, whole[v])


# ---- GPU ---------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def snap(be, frames, got):
    """render, and - on the GPU - who rendered what: (audio, noise word, osc3filt info, batch info, sweep info)"""
    a = be.render(frames)
    on = is_gpu(be)
    got.append((a, be.noise.value, be.last_batch_osc3filt() if on else None, last_batch(be) if on else None,
                be.last_batch_sweeps() if on else None))


def walk(sc, frames):
    """one batch of fragments walked by calls; `frames`: their lengths"""
    for n in frames:
        sc.walk(n)
    return sum(frames)


def compare(got, want):
    assert len(got) == len(want)
    loud = 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0].shape == w[0].shape, k
        assert first_diff(g[0], w[0]) is None, f"batch {k}: (ch, frame, gpu, oracle) = {first_diff(g[0], w[0])}; {g[2]}"
        assert g[1] == w[1], f"batch {k}: noise word {g[1]:#x} against the oracle's {w[1]:#x}"
        loud += int(np.abs(g[0]).max() > 0)
    assert loud


_oracle = {}


def both(oracle_lib, key, script, max_batch=64):
    """script(be) -> [snap tuples]: on the GPU and - once per key - on the oracle; compared; the GPU's tuples"""
    be = make_gpu(max_batch=max_batch)
    got = script(be)
    be.close()
    if key not in _oracle:
        ora = make_oracle(oracle_lib)
        _oracle[key] = script(ora)
        ora.close()
        for w in _oracle[key]:
            w[0].setflags(write=False)
    compare(got, _oracle[key])
    return got


def env(monkeypatch, no_fast=None, vpg=None, **more):
    for name, val in {"A2AMD_NO_FAST": no_fast, "A2AMD_F2VPW": vpg, "A2AMD_O2F_MIN": more.get("o2f_min")}.items():
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))


def auto_vpg(n, forced=None):
    """launch_leaves' voices per workgroup: A2AMD_F2VPW when set, else a 256th of the class; 1 .. 64"""
    return min(max(forced if forced else (n + 255) // 256, 1), 64)


def quad(i):
    return (i.launched, i.quiet_voices, i.gliding_voices, i.record_voices)


def lead(be, sc, dst, waves, pitches, amps, cutoff=2.0, q=3.0, mix=None, pan=0.0, vol=None, third_flags=PROCADD, filt_ch=1,
         pan_wired=1, extra_osc=False):
    """one voice `wtosc; wtosc+; wtosc+; filter12; panmix+ >` by calls (or, by the last four arguments, a chain just
    outside the class).  waves / pitches / amps: per oscillator; a wave of None is never written"""
    key = sc._key()
    units = [be.unit_init(key, K_WTOSC, 0, 0, 1, 0), be.unit_init(key, K_WTOSC, PROCADD, 0, 1, 0),
             be.unit_init(key, K_WTOSC, third_flags, 0, 1, 0)]
    if extra_osc:
        units.append(be.unit_init(key, K_WTOSC, PROCADD, 0, 1, 0))
        waves, pitches, amps = list(waves) + [waves[0]], list(pitches) + [pitches[0] + 0.5], list(amps) + [amps[0]]
    nosc = len(units)
    units.append(be.unit_init(key, K_FILTER12, 0, filt_ch, filt_ch, 0))
    units.append(be.unit_init(key, K_PANMIX, PROCADD if pan_wired else 0, 1, 2, pan_wired))
    for o, w, p, a in zip(units[:nosc], waves, pitches, amps):
        if w is not None:
            be.unit_write(o, W, w)
        be.unit_write(o, P, p if isinstance(p, int) else fix(p))
        be.unit_write(o, A, a if isinstance(a, int) else fix(a))
    f, pm = units[nosc], units[nosc + 1]
    be.unit_write(f, CUT, fix(cutoff))
    be.unit_write(f, Q, fix(q))
    for reg, val in zip((LP, BP, HP), mix or ()):
        be.unit_write(f, reg, fix(val))
    be.unit_write(pm, PAN, pan if isinstance(pan, int) else fix(pan))
    if vol is not None:
        be.unit_write(pm, VOL, vol if isinstance(vol, int) else fix(vol))
    dst.append(units)
    return units


# -- 1. shapes and buses --
def split(n):
    """n leads over (root, stereo group, nested stereo group, delay group).  In list order - sorted by bus, the buses in
    the order of their owners' birth - the 130-voice scene at 64 voices a workgroup has a workgroup that spans the root's
    bus (1), the stereo group's (50) and the nested group's (13 of 30), one that spans two buses, and a last one of 2"""
    root = 1 if n >= 1 else 0
    rest = n - root
    st = rest * 50 // 129
    ne = rest * 30 // 129
    return root, st, ne, rest - st - ne


def shapes_scene(be, n):
    be.noise.value = 0x12345
    sc = synth.Scene(be)
    sc.root()
    nroot, nst, nne, ndl = split(n)
    total = n + 8
    st = sc.add_bus_group()
    sc.add_voices(nst, O3, group=st, total=total)
    ne = sc.add_bus_group(parent=st)
    sc.add_voices(nne, O3, group=ne, total=total)
    dl = sc.add_group()
    sc.add_voices(ndl, O3, group=dl, total=total)
    sc.add_voices(nroot, O3, total=total)
    return sc


SHAPE_BATCHES = [[64], [64], [64] * 8, [64] * 64, [64, 17, 1, 64, 17, 1, 64], [64] * 8]


def shapes_script(n):
    def script(be):
        sc = shapes_scene(be, n)
        got = []
        for frames in SHAPE_BATCHES:
            snap(be, walk(sc, frames), got)
        return got
    return script


def check_shapes(got, n, vpg, off=False):
    for k, (_a, _n, i, gen, _s) in enumerate(got):
        if off:
            assert tuple(getattr(i, f) for f in FIELDS) == (0,) * 8, (k, i)
        elif k == 0:     # (births: every voice carries its records)
            assert (i.launched, i.class_voices, i.quiet_voices, i.gliding_voices, i.record_voices) == (0, n, 0, 0, n), (k, i)
            assert gen.general_voices == n, (k, gen)
        else:
            assert (i.launched, i.class_voices, i.quiet_voices, i.gliding_voices, i.record_voices, i.vpg, i.workgroups) == (
                1, n, n, 0, 0, vpg, (n + vpg - 1) // vpg), (k, i)
            assert gen.general_voices == 0 and gen.n_moving_listed == 0, (k, gen)


@gpu
@pytest.mark.parametrize("vpg", [None, 1, 3, 64])
@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_shapes_and_buses(oracle_lib, monkeypatch, n, vpg):
    env(monkeypatch, vpg=vpg)
    assert split(130) == (1, 50, 30, 49)
    got = both(oracle_lib, ("shapes", n), shapes_script(n))
    check_shapes(got, n, auto_vpg(n, vpg))


# -- 2. waves --
def waves_script(be):
    be.noise.value = 0x777
    sc = synth.Scene(be)
    sc.root()
    st = sc.add_bus_group()
    n = np.arange(1000)
    odd = (np.sin(n * 2.0 * np.pi * 3 / 1000) * 30000.0).astype(np.int16)
    sizes, data = synth.wave_pyramid(odd)
    w_odd = be.wave_upload(0x900, synth.WMIPWAVE, synth.LOOPED, 1000, sizes + [0] * (synth.MIPLEVELS - len(sizes)), data)
    n = np.arange(2800)
    shot = (np.sin(n * 2.0 * np.pi / 70) * 28000.0 * (1.0 - n / 2800.0)).astype(np.int16)
    sizes, data = synth.wave_pyramid(shot, looped=False)
    w_shot = be.wave_upload(0x901, synth.WMIPWAVE, 0, 256, sizes + [0] * (synth.MIPLEVELS - len(sizes)), data)
    base = (sc.wave_ids[3], sc.wave_ids[8], sc.wave_ids[14])      # built-in looped cycles
    # per oscillator position: (wave, pitch) - looped and mip-mapped further up; 1 000 samples: the modulo wrap; a one-shot
    # wave, 1.4 samples a frame: over near frame 2 000, the row keeps the other two; no wave: a silent replacer writes
    # zeros, a silent adder adds nothing; beyond A2D_MAXPHINC at the last level: silence, the phase runs
    kinds = [(sc.wave_ids[1], 3.3), (w_odd, 0.4), (w_shot, 0.0), (None, 0.0), (sc.wave_ids[2], 8.5)]
    for pos in range(3):
        for k, (wv, pitch) in enumerate(kinds):
            waves, pitches = list(base), [-0.5 + 0.1 * k, -0.49 + 0.1 * k, -1.5 + 0.1 * k]
            waves[pos], pitches[pos] = wv, pitch
            lead(be, sc, st["leaves"], waves, pitches, (0.2, 0.15, 0.1), cutoff=1.0 + 0.3 * k, q=2.0 + pos,
                 mix=(1.0, 0.2 * pos, 0.1 * k), pan=((3 * pos + k) % 7 - 3) / 4.0)
    lead(be, sc, st["leaves"], (None, None, None), (0.0, 0.0, 0.0), (0.2, 0.2, 0.2))        # nothing plays: a row of zeros
    got = []
    snap(be, walk(sc, [64]), got)
    snap(be, walk(sc, [64] * 48), got)                  # the one-shot waves end in here
    snap(be, walk(sc, [64] * 8), got)
    snap(be, walk(sc, [64, 30, 64]), got)
    # what the kernel stored is what the general kernel goes on from: the phases, the filters' d1 / d2
    silent = st["leaves"][-1]
    be.unit_write(silent[0], W, sc.wave_ids[5])
    for units in st["leaves"][:15:4]:
        be.unit_write(units[1], A, fix(0.05), 100, 0)
    snap(be, walk(sc, [64] * 4), got)
    snap(be, walk(sc, [64] * 8), got)
    return got


@gpu
def test_waves(oracle_lib, monkeypatch):
    env(monkeypatch)
    got = both(oracle_lib, "waves", waves_script)
    want = [(0, 0, 0, 16), (1, 16, 0, 0), (1, 16, 0, 0), (1, 16, 0, 0), (1, 11, 0, 5), (1, 16, 0, 0)]
    assert [quad(i) for _a, _n, i, _g, _s in got] == want
    for _a, _n, i, gen, _s in got:
        assert i.class_voices == 16 and gen.general_voices == i.record_voices


# -- 3. fixed point outside the musical range --
def loud_script(be):
    be.noise.value = 0x31337
    sc = synth.Scene(be)
    sc.root()
    st = sc.add_bus_group()
    base = (sc.wave_ids[3], sc.wave_ids[8], sc.wave_ids[14])
    big = (fix(127.99), fix(-128.0), fix(127.9))        # << 8: the ends of the 8.24 amplitude register
    lead(be, sc, st["leaves"], base, (-0.5, -0.49, -1.5), big, cutoff=2.5, q=1.0, mix=(1.0, 0.5, 0.5), pan=1.5)
    lead(be, sc, st["leaves"], base, (0.2, 0.21, 0.7), (big[1], big[0], big[1]), cutoff=4.0, q=0.3, mix=(-1.0, 1.0, 1.0), pan=-1.75,
         vol=fix(100.0))
    lead(be, sc, st["leaves"], base, (0.9, 0.0, -0.9), (big[0], big[0], big[0]), cutoff=0.5, q=8.0, pan=fix(127.9), vol=fix(-3.0))
    lead(be, sc, st["leaves"], base, (0.0, 0.5, 1.0), (0.1, 0.1, 0.1), pan=0.999)          # (one inside the range, below the clamp)
    got = []
    for frames in ([64] * 2, [64] * 8, [64, 17, 64], [64] * 8):
        snap(be, walk(sc, frames), got)
    # a pan ramp from beyond the clamp to inside it, all amplitudes still at the limits
    be.unit_write(st["leaves"][0][4], PAN, fix(0.2), 0, 600 << 8)
    for _ in range(3):
        snap(be, walk(sc, [64] * 8), got)
    return got


@gpu
def test_fixed_point_outside_the_musical_range(oracle_lib, monkeypatch):
    env(monkeypatch)
    got = both(oracle_lib, "loud", loud_script, max_batch=8)
    want = [(0, 0, 0, 4)] + [(1, 4, 0, 0)] * 3 + [(1, 3, 0, 1), (1, 4, 1, 0), (1, 4, 0, 0)]
    # (the pan ramp: written at frame 1 233, bound 1 233 + 256 + 600 = 2 089 - beyond the start of the batch at 1 745, not
    # of the one at 2 257)
    assert [quad(i) for _a, _n, i, _g, _s in got] == want
    # the filter's state did overflow: the loud voices' output is not a scaled copy of the quiet scene's
    assert max(int(np.abs(a).max()) for a, *_ in got) > 1 << 28


# -- 4. glides and handover --
GLIDE_BATCH = 8         # fragments
GLIDE_DURS = (1000, 612, 800, 700, 900)


def glides_script(be):
    be.noise.value = 0x4242
    sc = synth.Scene(be)
    sc.root()
    st = sc.add_bus_group()
    sc.add_voices(6, O3, group=st, total=16)
    dl = sc.add_group()
    sc.add_voices(3, O3, group=dl, total=16)
    v = st["leaves"] + dl["leaves"]
    got = []
    one = [64] * GLIDE_BATCH
    snap(be, walk(sc, one), got)                        # 0: births
    snap(be, walk(sc, one), got)                        # 1: quiet
    be.unit_write(v[0][1], P, fix(2.4), 0, 1000 << 8)   # pitch glides of two octaves and more on oscillators 1 and 2:
    be.unit_write(v[0][2], P, fix(-3.1), 0, 900 << 8)   # ... across mip levels, up and down
    be.unit_write(v[1][0], A, fix(0.02), 0, 612 << 8)   # an amplitude ramp that ends 36 frames into a fragment of the next batch
    be.unit_write(v[2][3], Q, fix(0.4), 0, 800 << 8)    # a q ramp
    be.unit_write(v[3][4], VOL, fix(0.3), 0, 700 << 8)  # a volume ramp
    be.unit_write(v[4][4], PAN, fix(1.4), 0, 900 << 8)  # a pan ramp that crosses a2s_pan_over on its way
    be.unit_write(v[5][0], P, fix(-0.7), 128, 0)        # a start offset, no duration
    for _ in range(6):                                  # 2: the records; 3 - 7: gliding, then at rest
        snap(be, walk(sc, one), got)
    # to the general kernel from what k_leaf_osc3filtpan stored - d1 / d2, every ramper - and back
    be.unit_write(v[0][0], A, fix(0.1), 30, 400 << 8)
    be.unit_write(v[2][3], Q, fix(2.0), 0, 0)
    be.unit_write(v[4][4], PAN, fix(-0.3), 10, 0)
    be.unit_write(v[6][1], PHASE, 12345)
    snap(be, walk(sc, one), got)                        # 8
    snap(be, walk(sc, [64, 40, 64]), got)               # 9
    snap(be, walk(sc, one), got)                        # 10
    return got


def check_glides(got):
    span = 64 * GLIDE_BATCH
    t_write = 2 * span
    assert (t_write + 612) % 64 == 36
    want = [(0, 0, 0, 9), (1, 9, 0, 0), (1, 3, 0, 6)]
    for k in range(3, 8):       # a2amd_unit_write's bound: the write's frame + 64 + duration + 192
        want.append((1, 9, sum(t_write + 256 + d > k * span for d in GLIDE_DURS), 0))
    assert [w[2] for w in want[3:]] == [5, 3, 0, 0, 0]
    # (the amplitude ramp of batch 8: written at frame 4 096, bound 4 096 + 256 + 400 = 4 752 - beyond the start of batch 9 at
    # 4 608, not of batch 10 at 4 776)
    want += [(1, 5, 0, 4), (1, 9, 1, 0), (1, 9, 0, 0)]
    assert [quad(i) for _a, _n, i, _g, _s in got] == want
    for k, (_a, _n, i, gen, _s) in enumerate(got):
        assert i.class_voices == 9, (k, i)
        assert gen.general_voices == i.record_voices and gen.n_moving_listed == 0, (k, gen)


@gpu
def test_glides_and_handover(oracle_lib, monkeypatch):
    env(monkeypatch)
    check_glides(both(oracle_lib, "glides", glides_script, max_batch=GLIDE_BATCH))


# -- 5. births and deaths --
@gpu
def test_births_and_deaths(oracle_lib, monkeypatch):
    env(monkeypatch)

    def script(be):
        be.noise.value = 0xbeef
        sc = synth.Scene(be)
        sc.root()
        st = sc.add_bus_group()
        sc.add_voices(6, O3, group=st, total=16)
        got = []
        one = [64] * 4
        snap(be, walk(sc, one), got)                    # 0: births
        snap(be, walk(sc, one), got)                    # 1: 6 quiet
        for u in st["leaves"].pop(2):
            be.unit_deinit(u)
        snap(be, walk(sc, one), got)                    # 2: the dying voice is listed to the end of its batch
        snap(be, walk(sc, one), got)                    # 3: 5 quiet
        sc.add_voices(2, O3, group=st, total=16)        # two births: the slot is used again
        snap(be, walk(sc, one), got)                    # 4
        snap(be, walk(sc, one), got)                    # 5: 7 quiet
        snap(be, walk(sc, [64, 21, 64]), got)           # 6
        return got

    got = both(oracle_lib, "births", script, max_batch=4)
    want = [(0, 6, 0, 6), (1, 6, 6, 0), (1, 6, 5, 1), (1, 5, 5, 0), (1, 7, 5, 2), (1, 7, 7, 0), (1, 7, 7, 0)]
    assert [(i.launched, i.class_voices, i.quiet_voices, i.record_voices) for _a, _n, i, _g, _s in got] == want


# -- 6. class edges --
EDGES = {"third oscillator replaces": dict(third_flags=0), "two-channel filter": dict(filt_ch=2),
         "panmix not wired": dict(pan_wired=0), "four oscillators": dict(extra_osc=True)}


def edge_script(how):
    def script(be):
        be.noise.value = 0xed9e
        sc = synth.Scene(be)
        sc.root()
        st = sc.add_bus_group()
        sc.add_voices(2, "osc-pan", group=st, total=8)  # (something audible whatever the edge does)
        base = (sc.wave_ids[3], sc.wave_ids[8], sc.wave_ids[14])
        for k in range(3):
            lead(be, sc, st["leaves"], base, (-0.5 + 0.2 * k, -0.49, -1.5), (0.2, 0.15, 0.1), pan=0.3 * k - 0.3, **EDGES[how])
        got = []
        for frames in ([64] * 2, [64] * 8, [64, 17, 64]):
            snap(be, walk(sc, frames), got)
        return got
    return script


@gpu
@pytest.mark.parametrize("how", sorted(EDGES))
def test_class_edges(oracle_lib, monkeypatch, how):
    """a chain one step outside the class is CLS_GENERIC (A2AMD_CLS_CHECK, the suite's setting, classifies every voice at
    every rebuild): never counted, never launched for, the same audio"""
    env(monkeypatch)
    got = both(oracle_lib, ("edge", how), edge_script(how), max_batch=8)
    for k, (_a, _n, i, gen, _s) in enumerate(got):
        assert tuple(getattr(i, f) for f in FIELDS) == (0,) * 8, (k, i)
        assert gen.general_voices == 0, (k, gen)        # (general LEAVES stand on their own segment, not on the exception list)


@gpu
def test_an_oscillator_switched_to_noise_leaves_the_class(oracle_lib, monkeypatch):
    env(monkeypatch)

    def script(be):
        be.noise.value = 0x5eed
        sc = synth.Scene(be)
        sc.root()
        st = sc.add_bus_group()
        sc.add_voices(3, O3, group=st, total=8)
        got = []
        one = [64] * 4
        snap(be, walk(sc, one), got)                    # 0: births
        snap(be, walk(sc, one), got)                    # 1: 3 quiet
        be.unit_write(st["leaves"][1][2], W, sc.noise_id)
        for _ in range(3):                              # 2 - 4: the noise voice is a general leaf
            snap(be, walk(sc, one), got)
        be.unit_write(st["leaves"][1][2], W, sc.wave_ids[6])
        for _ in range(3):                              # 5: the write; then of the class again
            snap(be, walk(sc, one), got)
        return got

    got = both(oracle_lib, "noise", script, max_batch=4)
    infos = [i for _a, _n, i, _g, _s in got]
    assert [(i.launched, i.class_voices, i.quiet_voices, i.record_voices) for i in infos[:5]] == [
        (0, 3, 0, 3), (1, 3, 3, 0), (1, 2, 2, 0), (1, 2, 2, 0), (1, 2, 2, 0)]
    # (back on a wave: of the class again once no batch of its has a window off the mip-mapped waves)
    assert all(i.class_voices in (2, 3) and i.quiet_voices >= 2 and i.launched == 1 for i in infos[5:]), infos[5:]
    assert infos[-1].class_voices == 3 and infos[-1].quiet_voices == 3, infos[-1]


# -- 7. A/B --
@gpu
def test_switched_off_is_the_same_audio(oracle_lib, monkeypatch):
    """A2AMD_NO_FAST=1024: no class, no launch - every lead the general kernel's, as before the class existed"""
    env(monkeypatch, no_fast=1024)
    check_shapes(both(oracle_lib, ("shapes", 65), shapes_script(65)), 65, 0, off=True)
    got = both(oracle_lib, "glides", glides_script, max_batch=GLIDE_BATCH)
    for k, (_a, _n, i, _g, _s) in enumerate(got):
        assert tuple(getattr(i, f) for f in FIELDS) == (0,) * 8, (k, i)


# -- 8. a cutoff sweeping in repeated fragments --
@gpu
def test_sweep_stand_in(oracle_lib, monkeypatch):
    """a2amd_fragment_repeat with one lead's cutoff ramping: that voice has the stand-in run (a column of the sweep table)
    and is the general kernel's; the others stay the kernel's"""
    env(monkeypatch)
    dur = 10 * 64 + 20

    def script(be):
        be.noise.value = 0xc0ffee
        sc = synth.Scene(be)
        sc.root()
        sc.add_voices(3, O3, total=8)
        got = []

        def batch(walked, repeats):
            if is_gpu(be):
                walk(sc, [64] * walked)
                be.fragment_repeat(64, repeats)
            else:
                walk(sc, [64] * (walked + repeats))
            snap(be, (walked + repeats) * 64, got)

        batch(8, 0)                                     # 0: births
        batch(1, 7)                                     # 1: repeats, nothing sweeps
        be.unit_write(sc.leaves[1][3], CUT, fix(4.0), 0, dur << 8)
        batch(1, 7)                                     # 2: the write's record
        batch(0, 8)                                     # 3: repeats alone, the ramp ends in here: the stand-in
        batch(0, 8)                                     # 4: at rest
        return got

    got = both(oracle_lib, "sweep", script, max_batch=8)
    assert [quad(i) for _a, _n, i, _g, _s in got] == [(0, 0, 0, 3), (1, 3, 0, 0), (1, 2, 0, 1), (1, 2, 0, 1), (1, 3, 0, 0)]
    sweeps = [s for *_x, s in got]
    assert (sweeps[3].filters, sweeps[3].standin_voices) == (1, 1), sweeps[3]
    assert (sweeps[4].filters, sweeps[4].standin_voices) == (0, 0), sweeps[4]
    assert [g.general_voices for _a, _n, _i, g, _s in got] == [3, 0, 1, 1, 0]


# -- 9. neighbours --
@gpu
def test_two_oscillator_neighbours_are_left_alone(oracle_lib, monkeypatch):
    """2 x wtosc-filter12-panmix voices on their own quiet kernel (A2AMD_O2F_MIN=1) beside the new class: a2amd_last_batch()'s
    o2f_* fields are what they are without the new voices"""
    env(monkeypatch, o2f_min=1)
    names = ("o2f_launched", "o2f_voices", "o2f_vpg", "o2f_max_vpg", "o2f_class", "o2f_listed")

    def script(nlead):
        def run(be):
            be.noise.value = 0xabc
            sc = synth.Scene(be)
            sc.root()
            st = sc.add_bus_group()
            sc.add_voices(4, "osc2-filter-pan", group=st, total=16)
            sc.add_voices(nlead, O3, group=st, total=16)
            got = []
            for frames in ([64] * 4, [64] * 4, [64, 17, 64], [64] * 4):
                snap(be, walk(sc, frames), got)
            return got
        return run

    with_leads = both(oracle_lib, ("neighbours", 5), script(5), max_batch=4)
    without = both(oracle_lib, ("neighbours", 0), script(0), max_batch=4)
    for k, (a, b) in enumerate(zip(with_leads, without)):
        assert [getattr(a[3], n) for n in names] == [getattr(b[3], n) for n in names], k
        assert (a[2].class_voices, b[2].class_voices) == (5, 0), k
    assert [quad(g[2]) for g in with_leads] == [(0, 0, 0, 5)] + [(1, 5, 0, 0)] * 3
    # (the neighbours' own quiet kernel was reached: launched for the class from the first batch on, as without the leads)
    assert [(g[3].o2f_launched, g[3].o2f_class) for g in with_leads] == [(1, 4)] * 4


# -- 10. the fixture --
@gpu
@pytest.mark.parametrize("batch", [16, 64])
def test_fixture_reaches_the_kernel(lead3, monkeypatch, batch):
    """lead3 replayed: hash-equal to the reference in every fragment; six voices of the class in every batch behind the
    births; a lead is the kernel's exactly in the batches the trace leaves it without a record, the general kernel's in
    the others - at 64 fragments a batch that is every batch but the last, short one"""
    env(monkeypatch)
    voices = lead_voices(lead3)
    free = record_free(lead3, voices, batch)
    quiet = [sum(col) for col in zip(*(free[v] for v in sorted(voices)))]
    cfg = lead3.config
    be = make_gpu(cfg["samplerate"], cfg["basepitch"], cfg["channels"], max_batch=batch)
    infos = []
    render = be.render

    def spy(*a, **kw):
        out = render(*a, **kw)
        infos.append(be.last_batch_osc3filt())
        return out

    be.render = spy
    out = replay(lead3, be, batch=batch, check_noise=True)
    be.close()
    want = np.load(os.path.join(GOLDEN, "lead3.hash.npy"))
    got = fnv1a_fragments(out)
    assert len(got) == len(want) == 1500
    bad = np.nonzero(got != want)[0]
    assert not bad.size, bad[:4]
    assert len(infos) == len(quiet) == (94 if batch == 16 else 24)
    print("batches in which the kernel rendered:", sum(i.launched for i in infos), "of", len(infos))
    for k, (i, nq) in enumerate(zip(infos, quiet)):
        assert (i.launched, i.quiet_voices, i.record_voices) == (int(nq > 0), nq, 6 - nq), (k, i, nq)
        assert i.class_voices == 6, (k, i)
    assert sum(i.launched for i in infos) == (69 if batch == 16 else 1)


# -- 11. device VM --
@gpu
def test_a_voice_the_device_vm_runs_is_not_of_the_class(oracle_lib, monkeypatch):
    """5 quiet leads and one lead handed to the device VM with the looping program test_device_vm.py uses (for { +p .01;
    d 3; -p .01; d 3 } on the first oscillator's pitch: a ramp every 144 frames): from its adoption on the voice is the
    general kernel's - never in class_voices - in the batches in which its VM writes and in those in which it sleeps, and
    the audio is the oracle's, which gets the same writes and windows as calls (made by the host copy of the
    interpreter).  Should a2amd_vm_adopt refuse the chain, the refusal is asserted and the voice stays of the class."""
    from test_device_vm import FILTER12, MSDUR, PANMIX, R_SEG, R_WRITE, WTOSC, VmState, asm, fx, trace_host
    from audiality2_amd.replay import a2amd_vm_state
    env(monkeypatch)
    monkeypatch.delenv("A2AMD_NO_VM", raising=False)
    code, n = asm(("ADD", 5, 0, fx(.01)), ("DELAY", 0, 0, fx(3)), ("ADD", 5, 0, fx(-.01)), ("DELAY", 0, 0, fx(3)), ("JUMP", 0, 0))
    pitch = fix(0.5)
    plan = [[64]] * 12 + [[64] * 4] * 2                 # the batches behind the one in which the voice is adopted
    nfr = sum(len(b) for b in plan)

    def state():
        st = VmState()
        st.state = 1                                    # A2_WAITING
        st.waketime = ((128 + 20) << 8) | 0x40          # frame 20.25 of the first fragment behind the adoption
        st.r[5] = pitch
        return st

    def scene(be):
        sc = synth.Scene(be)
        sc.root()
        st = sc.add_bus_group()
        sc.add_voices(5, O3, group=st, total=16)
        x = lead(be, sc, [], (sc.wave_ids[4], sc.wave_ids[9], sc.wave_ids[2]), (pitch, 0.49, -0.5), (0.1, 0.1, 0.1), pan=0.25)
        return sc, st, x

    def walk1(be, sc, st, x_calls):
        """Scene.walk for this tree, the voice x by x_calls(): calls, or the default map"""
        be.fragment(64)
        be.unit_process(sc.rootv[0], 0, 64)
        be.unit_process(st["units"][0], 0, 64)
        for units in st["leaves"]:
            for u in units:
                be.unit_process(u, 0, 64)
        x_calls()
        be.inline_end(st["units"][0])
        for u in st["units"][1:]:
            be.unit_process(u, 0, 64)
        be.inline_end(sc.rootv[0])
        be.unit_process(sc.rootv[1], 0, 64)
        be.unit_process(sc.rootv[2], 0, 64)

    def whole(be, x):
        def calls():
            for u in x:
                be.unit_process(u, 0, 64)
        return calls

    # the GPU
    be = make_gpu(max_batch=4)
    sc, st, x = scene(be)
    got, infos = [], []
    walk1(be, sc, st, whole(be, x))
    got.append(be.render(64))
    infos.append(be.last_batch_osc3filt())
    walk1(be, sc, st, whole(be, x))
    prog = be.vm_program(0x5150, list(code))
    assert prog >= 0
    adopted = be.vm_adopt(x[0], prog, a2amd_vm_state.from_buffer_copy(state()), {5: (x[0], 1)}, 64 << 8, MSDUR, check=False)
    print("a2amd_vm_adopt:", adopted)
    if adopted != 0:
        assert adopted == -4, adopted                   # A2AMD_EUNSUPPORTED: the chain stays the engine's
    got.append(be.render(64))
    infos.append(be.last_batch_osc3filt())
    for frames in plan:
        for _ in frames:
            walk1(be, sc, st, (lambda: be.mark_default(x)) if adopted == 0 else whole(be, x))
        got.append(be.render(sum(frames)))
        infos.append(be.last_batch_osc3filt())
    be.close()

    # the oracle: the VM's writes and windows as calls
    ora = make_oracle(oracle_lib)
    sc, st, x = scene(ora)
    recs = {}
    if adopted == 0:
        kinds = [WTOSC, WTOSC, WTOSC, FILTER12, PANMIX]
        for frag, op, unit, reg, value, dur, start in trace_host(code, n, state(), [5], [(0, 1)], kinds, [64] * nfr, now=128 << 8):
            recs.setdefault(frag, []).append((op, unit, reg, value, dur, start))
        assert sum(1 for f in range(12) if f in recs) in range(3, 10)       # one-fragment batches with writes, and without

    def vm_calls(f):
        def calls():
            if f not in recs:
                whole(ora, x)()
            for op, unit, reg, value, dur, start in recs.get(f, ()):
                if op == R_SEG:
                    for u in x:
                        ora.unit_process(u, dur & 0xffff, dur >> 16)
                else:
                    assert op == R_WRITE
                    ora.unit_write(x[unit], reg, value, start, dur)
        return calls

    want = []
    for _ in range(2):
        walk1(ora, sc, st, whole(ora, x))
        want.append(ora.render(64))
    f = 0
    for frames in plan:
        for _ in frames:
            walk1(ora, sc, st, vm_calls(f))
            f += 1
        want.append(ora.render(sum(frames)))
    ora.close()
    for k, (a, w) in enumerate(zip(got, want)):
        assert first_diff(a, w) is None, f"batch {k}: (ch, frame, gpu, oracle) = {first_diff(a, w)}"
    cls = 5 if adopted == 0 else 6
    assert [(i.launched, i.class_voices, i.quiet_voices, i.record_voices) for i in infos] == [(0, 6, 0, 6)] + [(1, cls, cls, 0)] * (1 + len(plan))
