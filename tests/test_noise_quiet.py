"""k_leaf_noisepan: settled wtosc (noise) -> panmix voices of a batch with device-seeded fragments in a quiet kernel
of their own (a2amd_noisepan.hip) - its arithmetic on the CPU against the sample loop of wtosc.c:140-150, the
rendering bit for bit against the oracle walked fragment by fragment, and who rendered what
(a2amd_last_batch_noise)."""
import ctypes
import os
import re

import numpy as np
import pytest

from audiality2_amd import synth
from conftest import ROOT, make_gpu, make_oracle
from test_gpu_parity import first_diff
from test_noise_repeat import M32, SEED0, lcg

B23 = 1 << 23


# ---- CPU ---------------------------------------------------------------------------------
def _window(lib):
    lib.a2amd_noise_window.restype = ctypes.c_uint32
    lib.a2amd_noise_window.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint,
                                       ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)]
    buf, after = (ctypes.c_int32 * 64)(), ctypes.c_uint32(0)

    def window(seed, phase, dphase, held, frames):
        n = lib.a2amd_noise_window(seed, phase, dphase, held, frames, buf, ctypes.byref(after))
        return list(buf[:frames]), n, after.value

    return window


def window_by_sample(seed, phase, dphase, held, frames):
    """wtosc.c:140-150, frame by frame, with a2_Noise (a2_dsp.h:37-42): the samples held, the draws, the generator
    word afterwards"""
    out, n = [], 0
    for _ in range(frames):
        nph = (phase + dphase) & ((1 << 64) - 1)
        if dphase >= B23 or ((nph ^ phase) >> 23):
            seed = (seed * 1566083941 + 1) & M32
            v = (((seed * (seed >> 16)) & M32) >> 16)
            held = (v - (1 << 32) if v & 0x80000000 else v) - 32767
            n += 1
        phase = nph
        out.append(held)
    return out, n, seed


def test_header_and_exports(gpu_lib):
    text = open(os.path.join(ROOT, "include", "a2amd_noisepan.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(a2amd_[a-z_0-9]+)\s*\(", text)))
    assert syms == ["a2amd_last_batch_noise", "a2amd_noise_window"]
    for s in syms:
        assert hasattr(gpu_lib, s), f"liba2amd.so lacks {s}"
    assert '#include "a2amd_noisepan.h"' in open(os.path.join(ROOT, "include", "a2amd.h")).read()


def test_noise_window_equals_the_sample_loop(gpu_lib):
    window = _window(gpu_lib)
    dphases = [1, 255, 0x594d, B23 // 3, B23 // 2, B23 - 2, B23 - 1, B23, B23 + 1, 2 * B23, 0x165373c, M32]
    phases = [0, 1, B23 - 1, B23 - 2, 5 * B23 - 1, 5 * B23, 5 * B23 + 1, 1000 * B23 - 3, (1 << 32) - 1, (1 << 32),
              (1 << 40) + B23 - 1, 977 * B23 - 0x594d]
    rng = np.random.default_rng(3)
    checked = 0
    for d in dphases:
        for ph in phases:
            for frames in range(1, 65):
                seed, held = int(rng.integers(0, 1 << 32)), int(rng.integers(-40000, 40000))
                want = window_by_sample(seed, ph, d, held, frames)
                got = window(seed, ph, d, held, frames)
                assert got == want, (seed, ph, d, held, frames)
                assert got[0][-1] == want[0][-1]        # (the sample held afterwards)
                checked += 1
    assert checked == len(dphases) * len(phases) * 64
    for _ in range(500):
        ph, d = int(rng.integers(0, 1 << 48)), int(rng.integers(1, 1 << 25))
        seed, held, frames = int(rng.integers(0, 1 << 32)), int(rng.integers(-40000, 40000)), int(rng.integers(1, 65))
        assert window(seed, ph, d, held, frames) == window_by_sample(seed, ph, d, held, frames), (seed, ph, d, held, frames)


def test_consecutive_windows_telescope(gpu_lib):
    window = _window(gpu_lib)
    rng = np.random.default_rng(4)
    for d in [1, 0x594d, 22861, B23 // 3, B23 - 1, B23, 3 * B23] + [int(x) for x in rng.integers(1, 1 << 25, 40)]:
        for _ in range(6):
            ph, seed, held = int(rng.integers(0, 1 << 48)), int(rng.integers(0, 1 << 32)), int(rng.integers(-40000, 40000))
            whole = window(seed, ph, d, held, 64)
            a = window(seed, ph, d, held, 23)
            b = window(a[2], ph + 23 * d, d, a[0][-1], 41)
            assert (a[0] + b[0], a[1] + b[1], b[2]) == whole, (seed, ph, d, held)


# ---- GPU ---------------------------------------------------------------------------------
def p2i(tab, pitch):
    """a2_P2I, pitch.c:57-67"""
    n, octave = pitch & 0xffff, pitch >> 16
    dph = ((int(tab[2 * (n >> 10) + 1]) * (n & 0x3ff)) & M32) >> 2
    return ((dph + int(tab[2 * (n >> 10)])) & M32) >> ((7 - octave) & 31)


def noise_pitch(k):
    """synth.Scene.add_voices' pitch for noise voice number k"""
    return synth.fix(((k * 7) % 31) / 3.0 - 2.0)


class QuietScene:
    """noise_scene's shape (test_noise_repeat.py): noise voices under two delay-bus groups and under the root, wave
    voices between them in walk order; n_pan noise-pan voices in three blocks, two noise-filter-pan voices and one
    voice with two noise oscillators beside them.  pan_ks / other_ks: the voice numbers synth took the pitches from."""

    def __init__(self, be, n_pan):
        self.be = be
        sc = self.sc = synth.Scene(be)
        sc.root()
        g1, g2 = sc.add_group(), sc.add_group()
        loud = min(64, n_pan + 40)
        na, nb = n_pan // 3, n_pan // 3
        self.pan, self.pan_ks, self.other_ks = [], [], []

        def noise(n, chain, group, k0):
            sc.nvoices = k0             # (the voice number decides pitch, pan and phase: the blocks start where we say)
            sc.add_voices(n, chain, group=group, total=loud)
            dst = sc.leaves if group is None else group["leaves"]
            (self.pan_ks if chain == "noise-pan" else self.other_ks).extend(range(k0, k0 + n))
            if chain == "noise-pan" and n:
                self.pan.extend(dst[-n:])

        sc.add_voices(6, "osc-pan", group=g1, total=loud)
        noise(na, "noise-pan", g1, 31)
        sc.add_voices(3, "osc2-pan", group=g1, total=loud)
        sc.add_voices(2, "osc-filter-pan", group=g2, total=loud)
        noise(nb, "noise-pan", g2, 31 + na)
        noise(1, "noise-filter-pan", g2, 17)        # (6.5 octaves up and more: a draw in every frame)
        noise(1, "noise-filter-pan", g2, 2)         # (2.67 octaves up: a draw every few frames)
        sc.nvoices = 200
        sc.add_voices(5, "osc-pan", total=loud)
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
        noise(n_pan - na - nb, "noise-pan", None, 0)     # (voice number 0: two octaves down, the sparsest)
        sc.nvoices = 300
        sc.add_voices(2, "osc-filter-pan", total=loud)
        self.n_pan, self.n_other = n_pan, 3

    def increments(self, ks):
        tab, base = self.be.get_pitch_table(), synth.basepitch_for(48000)
        return [p2i(tab, noise_pitch(k) + base) for k in ks]


def regimes(ds):
    return (sum(d >= B23 for d in ds), sum((1 << 17) <= d < B23 for d in ds), sum(d * 64 * 5 < B23 for d in ds))


def run_plan(be, repeat, n_pan, short=False):
    """the batch plan; per batch (audio, noise word, a2amd_last_batch_noise or None, repeat-only?)"""
    be.noise.value = SEED0
    q = QuietScene(be, n_pan)
    sc = q.sc
    if repeat:
        ds = q.increments(q.pan_ks + q.other_ks)
        assert all(regimes(ds)), regimes(ds)
        if n_pan >= 31:
            assert all(regimes(q.increments(q.pan_ks))), regimes(q.increments(q.pan_ks))
        # the sparsest noise-pan voice draws less than once in five fragments
        assert min(q.increments(q.pan_ks)) * 64 * 5 < B23
    got = []

    def rest(n, frames=64):
        if repeat:
            be.fragment_repeat_noise(frames, n)
        else:
            for _ in range(n):
                sc.walk(frames)

    def snap(frames, only):
        a = be.render(frames)
        got.append((a, be.noise.value, be.last_batch_noise() if repeat else None, only))

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
    rest(8)
    snap(8 * 64, True)
    for _ in range(3):                  # one fragment each: the sparse oscillator's held sample crosses through OW_NOISE
        rest(1)
        snap(64, True)
    rest(2)
    be.noise.value = lcg(be.noise.value, 11)
    rest(5)                             # two stretches in one batch
    snap(7 * 64, True)
    rest(6, 37)
    snap(6 * 37, True)
    rest(16)
    snap(16 * 64, True)
    # the state the quiet kernel stored goes back to the window kernels: a pitch write and a pan write
    be.unit_write(q.pan[0][0], 1, synth.fix(6.75))
    be.unit_write(q.pan[-1][1], 1, synth.fix(0.4))
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


def oracle_plan(oracle_lib, n_pan, short):
    """the oracle's side of the plan, rendered once per size"""
    if (n_pan, short) not in _oracle:
        _oracle[n_pan, short] = run_plan(make_oracle(oracle_lib), False, n_pan, short)[0]
    return _oracle[n_pan, short]


def compare(got, want):
    assert len(got) == len(want)
    for k, ((a, na, _i, _o), (b, nb, _j, _p)) in enumerate(zip(got, want)):
        assert first_diff(a, b) is None, f"batch {k}: (ch, frame, gpu, oracle) = {first_diff(a, b)}"
        assert na == nb, f"batch {k}: noise word {na:#x} against the oracle's {nb:#x}"
        assert np.abs(a).max() > 0


SIZES = [(1, False), (70, False), (2100, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_pan,short", SIZES)
def test_quiet_kernel_matches_the_oracle(oracle_lib, monkeypatch, n_pan, short):
    monkeypatch.delenv("A2AMD_NOISE_QUIET", raising=False)
    got, q = run_plan(make_gpu(max_batch=16), True, n_pan, short)
    compare(got, oracle_plan(oracle_lib, n_pan, short))
    for k, (_a, _n, bi, only) in enumerate(got):
        assert bi.class_voices == n_pan, k
        if only:
            assert (bi.quiet_launched, bi.quiet_voices, bi.standin_voices) == (1, n_pan, q.n_other), k
        else:
            assert (bi.quiet_launched, bi.quiet_voices, bi.standin_voices) == (0, 0, 0), k


@pytest.mark.gpu
@pytest.mark.parametrize("n_pan,short", SIZES[:2])
def test_switched_off_routes_as_before(oracle_lib, monkeypatch, n_pan, short):
    """A2AMD_NOISE_QUIET=0: no class, no launch, the stand-in for every noise voice - and the same audio"""
    monkeypatch.setenv("A2AMD_NOISE_QUIET", "0")
    got, q = run_plan(make_gpu(max_batch=16), True, n_pan, short)
    compare(got, oracle_plan(oracle_lib, n_pan, short))
    for k, (_a, _n, bi, only) in enumerate(got):
        assert (bi.quiet_launched, bi.quiet_voices, bi.class_voices) == (0, 0, 0), k
        assert bi.standin_voices == (n_pan + q.n_other if only else 0), k


@pytest.mark.gpu
def test_general_kernel_takes_everything(oracle_lib, monkeypatch):
    monkeypatch.delenv("A2AMD_NOISE_QUIET", raising=False)
    monkeypatch.setenv("A2AMD_NO_FAST", "255")
    got, q = run_plan(make_gpu(max_batch=16), True, 70)
    compare(got, oracle_plan(oracle_lib, 70, False))
    for k, (_a, _n, bi, only) in enumerate(got):
        assert (bi.quiet_launched, bi.quiet_voices, bi.class_voices) == (0, 0, 0), k
        assert bi.standin_voices == (70 + q.n_other if only else 0), k


def _both(oracle_lib, script):
    """script(be, repeat) -> [(audio, noise word, info)] on the GPU with repeats and on the oracle walked"""
    res = []
    for repeat in (True, False):
        be = make_gpu(max_batch=16) if repeat else make_oracle(oracle_lib)
        res.append(script(be, repeat))
        be.close()
    for k, ((a, na, _i), (b, nb, _j)) in enumerate(zip(*res)):
        assert first_diff(a, b) is None, f"batch {k}: (ch, frame, gpu, oracle) = {first_diff(a, b)}"
        assert na == nb, f"batch {k}: noise word {na:#x} against the oracle's {nb:#x}"
    return [i for _a, _n, i in res[0]]


def _tools(be, sc, repeat, got):
    def rest(n):
        if repeat:
            be.fragment_repeat_noise(64, n)
        else:
            for _ in range(n):
                sc.walk(64)

    def snap(frames):
        got.append((be.render(frames), be.noise.value, be.last_batch_noise() if repeat else None))

    return rest, snap


@pytest.mark.gpu
def test_ramping_amplitude_keeps_the_stand_in(oracle_lib, monkeypatch):
    """a 700-frame amplitude ramp on a noise-pan voice: the window kernels' while it lasts, the quiet kernel's after"""
    monkeypatch.delenv("A2AMD_NOISE_QUIET", raising=False)

    def script(be, repeat):
        be.noise.value = SEED0
        q = QuietScene(be, 9)
        got = []
        rest, snap = _tools(be, q.sc, repeat, got)
        be.unit_write(q.pan[4][0], 2, synth.fix(0.3), 0, 700 << 8)
        q.sc.walk(64)
        rest(7)
        snap(8 * 64)            # frames 0 .. 511
        rest(8)
        snap(8 * 64)            # 512 .. 1023: the ramp ends at 700
        rest(8)
        snap(8 * 64)            # settled
        rest(3)
        snap(3 * 64)
        return got

    infos = _both(oracle_lib, script)
    assert [(i.quiet_launched, i.quiet_voices, i.standin_voices) for i in infos] == [(0, 0, 0), (1, 8, 4), (1, 9, 3), (1, 9, 3)]


@pytest.mark.gpu
def test_mode_switch_and_death(oracle_lib, monkeypatch):
    monkeypatch.delenv("A2AMD_NOISE_QUIET", raising=False)

    def script(be, repeat):
        be.noise.value = SEED0
        q = QuietScene(be, 7)
        sc = q.sc
        got = []
        rest, snap = _tools(be, sc, repeat, got)
        sc.walk(64)
        rest(3)
        snap(4 * 64)
        rest(8)
        snap(8 * 64)                                    # 7 quiet
        # a wave voice becomes a noise voice ...
        wave = q.waves[1]
        be.unit_write(wave[0], 0, sc.noise_id)
        sc.walk(64)
        rest(3)
        snap(4 * 64)
        rest(8)
        snap(8 * 64)                                    # 8 quiet
        # ... and a wave voice again: k_leaf_oscpan's
        be.unit_write(wave[0], 0, sc.wave_ids[3])
        sc.walk(64)
        rest(3)
        snap(4 * 64)
        rest(8)
        snap(8 * 64)                                    # 7 quiet
        # a noise-pan voice dies between two batches of repeats (a fragment walked by calls follows the kill)
        dead = q.pan[2]
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
    assert [(i.quiet_launched, i.quiet_voices, i.class_voices, i.standin_voices) for i in infos] == [
        (0, 0, 7, 0), (1, 7, 7, 3), (0, 0, 8, 0), (1, 8, 8, 3), (0, 0, 7, 0), (1, 7, 7, 3), (0, 0, 7, 0), (1, 6, 6, 3)]      # (a dying voice is listed to the end of its batch)
