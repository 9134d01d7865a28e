"""a2amd_fragment_repeat_noise: stretches of default windows with settled noise oscillators, their
generator words made on the device (a2amd_noise.hip) - the arithmetic on the CPU, the rendering bit for
bit against the oracle driven fragment by fragment through Scene.walk()."""
import ctypes
import os
import re

import numpy as np
import pytest

from audiality2_amd import synth
from conftest import ROOT, make_gpu, make_oracle

A, M32 = 1566083941, 0xFFFFFFFF
EUNSUPPORTED, ESTATE = -4, -5
SEED0 = 0x2545F491


def lcg(s, n=1):
    for _ in range(n):
        s = (s * A + 1) & M32
    return s


def _arith(lib):
    lib.a2amd_noise_jump.restype = ctypes.c_uint32
    lib.a2amd_noise_jump.argtypes = [ctypes.c_uint32, ctypes.c_uint64]
    lib.a2amd_noise_draws.restype = ctypes.c_uint64
    lib.a2amd_noise_draws.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint]
    return lib


# ---- CPU ---------------------------------------------------------------------------------
def test_header_and_exports(gpu_lib):
    text = open(os.path.join(ROOT, "include", "a2amd_noise.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(a2amd_[a-z_0-9]+)\s*\(", text)))
    assert syms == ["a2amd_fragment_repeat_noise", "a2amd_noise_draws", "a2amd_noise_jump"]
    for s in syms:
        assert hasattr(gpu_lib, s), f"liba2amd.so lacks {s}"
    assert '#include "a2amd_noise.h"' in open(os.path.join(ROOT, "include", "a2amd.h")).read()


def test_noise_jump_equals_the_loop(gpu_lib):
    lib = _arith(gpu_lib)
    rng = np.random.default_rng(1)
    for _ in range(300):
        s, n = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 100001))
        assert lib.a2amd_noise_jump(s, n) == lcg(s, n), (s, n)
    for s, n in ((0, 0), (M32, 1), (0, 100000), (12345, 1)):
        assert lib.a2amd_noise_jump(s, n) == lcg(s, n)
    for _ in range(300):
        s = int(rng.integers(0, 1 << 32))
        a, b = int(rng.integers(0, 1 << 40)), int(rng.integers(0, 1 << 40))
        assert lib.a2amd_noise_jump(lib.a2amd_noise_jump(s, a), b) == lib.a2amd_noise_jump(s, a + b), (s, a, b)
    assert lib.a2amd_noise_jump(77, (1 << 40)) == lib.a2amd_noise_jump(lib.a2amd_noise_jump(77, (1 << 39)), (1 << 39))


def draws_by_sample(phase, dphase, frames):
    """wtosc.c:142-143, frame by frame: a draw when the increment is at least 1 << 23 or the step changes
    the phase above bit 23"""
    n = 0
    for _ in range(frames):
        nph = (phase + dphase) & ((1 << 64) - 1)
        if dphase >= (1 << 23) or ((nph ^ phase) >> 23):
            n += 1
        phase = nph
    return n


def test_noise_draws_equals_the_sample_loop(gpu_lib):
    lib = _arith(gpu_lib)
    B = 1 << 23
    dphases = [1, 255, 0x594d, B // 3, B // 2, B - 2, B - 1, B, B + 1, 2 * B, 0x165373c, M32]
    phases = [0, 1, B - 1, B - 2, 5 * B - 1, 5 * B, 5 * B + 1, 1000 * B - 3, (1 << 32) - 1, (1 << 32), (1 << 40) + B - 1,
              977 * B - 0x594d]
    checked = 0
    for d in dphases:
        for ph in phases:
            for frames in range(1, 65):
                assert lib.a2amd_noise_draws(ph, d, frames) == draws_by_sample(ph, d, frames), (ph, d, frames)
                checked += 1
    rng = np.random.default_rng(2)
    for _ in range(500):
        ph, d = int(rng.integers(0, 1 << 48)), int(rng.integers(1, 1 << 25))
        frames = int(rng.integers(1, 65))
        assert lib.a2amd_noise_draws(ph, d, frames) == draws_by_sample(ph, d, frames), (ph, d, frames)
    assert checked == len(dphases) * len(phases) * 64


# ---- GPU ---------------------------------------------------------------------------------
def first_diff(a, b):
    if a.shape != b.shape:
        return ("shape", a.shape, b.shape)
    bad = np.argwhere(a != b)
    if not len(bad):
        return None
    ch, fr = bad[np.argmin(bad[:, 1])]
    return int(ch), int(fr), int(a[ch, fr]), int(b[ch, fr])


def noise_scene(be, n_pan, n_filt):
    """root; two delay-bus groups with wave and noise voices; under the root wave voices, a voice with two
    noise oscillators, one whose amplitude ramps, more wave voices - noise between waves in walk order"""
    sc = synth.Scene(be)
    sc.root()
    g1, g2 = sc.add_group(), sc.add_group()
    loud = min(64, n_pan + n_filt + 32)
    sc.add_voices(6, "osc-pan", group=g1, total=loud)
    sc.add_voices(n_pan, "noise-pan", group=g1, total=loud)
    sc.add_voices(3, "osc2-pan", group=g1, total=loud)
    sc.add_voices(4, "osc-filter-pan", group=g2, total=loud)
    sc.add_voices(n_filt, "noise-filter-pan", group=g2, total=loud)
    sc.add_voices(5, "osc-pan", total=loud)
    key = sc._key()
    two = [be.unit_init(key, synth.K_WTOSC, 0, 0, 1, 0), be.unit_init(key, synth.K_WTOSC, synth.PROCADD, 0, 1, 0),
           be.unit_init(key, synth.K_PANMIX, synth.PROCADD, 1, 2, 1)]
    for j, o in enumerate(two[:2]):
        be.unit_write(o, 0, sc.noise_id)
        be.unit_write(o, 1, synth.fix(7.0 if j else 2.25))
        be.unit_write(o, 2, synth.fix(0.05))
    be.unit_write(two[2], 1, synth.fix(-0.25))
    sc.leaves.append(two)
    sc.add_voices(1, "noise-pan", total=loud)
    sc.ramped = sc.leaves[-1]
    be.unit_write(sc.ramped[0], 2, synth.fix(0.2), 0, 9000 << 8)       # an amplitude ramp of 9 000 frames
    sc.add_voices(4, "osc-filter-pan", total=loud)
    sc.two = two
    return sc


def batch(be, sc, n, repeat):
    """one fragment walked by calls, n more: through fragment_repeat_noise, or walked as well"""
    sc.walk(64)
    if repeat:
        be.fragment_repeat_noise(64, n)
    else:
        for _ in range(n):
            sc.walk(64)
    return be.render((n + 1) * 64)


SIZES = {"small": (1, 1), "wide": (2100, 1300)}


@pytest.mark.gpu
@pytest.mark.parametrize("size,win,nofast", [("small", "0", "0"), ("small", "1", "0"), ("small", "1", "255"),
                                             ("wide", "1", "0"), ("wide", "0", "0")])
def test_parity_with_the_oracle(oracle_lib, monkeypatch, size, win, nofast):
    """(win: the window kernels or k_leaf_recs; nofast=255: every voice through the general kernel)"""
    monkeypatch.setenv("A2AMD_WIN", win)
    monkeypatch.setenv("A2AMD_NO_FAST", nofast)
    plan = [15, 1, 7, 15] if size == "small" else [15, 1, 6]
    res = []
    for repeat in (True, False):
        be = make_gpu(max_batch=16) if repeat else make_oracle(oracle_lib)
        be.noise.value = SEED0
        sc = noise_scene(be, *SIZES[size])
        got = []
        for k, n in enumerate(plan):
            got.append((batch(be, sc, n, repeat), be.noise.value))
            if k == 1:      # (interleaving: host-side draws between two buffers, as a RAND would make)
                be.noise.value = lcg(be.noise.value, 3)
        res.append(got)
        be.close()
    for k, ((a, na), (b, nb)) in enumerate(zip(*res)):
        assert first_diff(a, b) is None, f"batch {k}: (ch, frame, gpu, oracle) = {first_diff(a, b)}"
        assert na == nb, f"batch {k}: noise word {na:#x} against the oracle's {nb:#x}"
        assert np.abs(a).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("win", ["1", "0"])
def test_whole_batches_of_repeats_and_hand_back(oracle_lib, monkeypatch, win):
    """Batches that are repeats only (no record of their own for any noise voice), then fragments driven by
    calls again: a pitch write on a noise oscillator, a wave oscillator switched to noise and back."""
    monkeypatch.setenv("A2AMD_WIN", win)
    res = []
    for repeat in (True, False):
        be = make_gpu(max_batch=8) if repeat else make_oracle(oracle_lib)
        be.noise.value = SEED0
        sc = noise_scene(be, 5, 4)
        got = []

        def rest(n):
            if repeat:
                be.fragment_repeat_noise(64, n)
            else:
                for _ in range(n):
                    sc.walk(64)

        def snap(frames):
            got.append((be.render(frames), be.noise.value))

        sc.walk(64)
        rest(3)
        snap(4 * 64)
        rest(8)                 # a batch of repeats alone
        snap(8 * 64)
        be.noise.value = lcg(be.noise.value, 11)
        rest(2)
        rest(5)                 # two stretches in one batch
        snap(7 * 64)
        # a pitch write on a noise oscillator, in a fragment driven by calls
        be.unit_write(sc.two[1], 1, synth.fix(3.5))
        noisy = sc.groups[0]["leaves"][6]
        be.unit_write(noisy[0], 1, synth.fix(6.75))
        sc.walk(64)
        rest(7)
        snap(8 * 64)
        # a wave oscillator becomes a noise oscillator (the host rebuilds its phase from the device's) ...
        wave_voice = sc.leaves[1]
        be.unit_write(wave_voice[0], 0, sc.noise_id)
        sc.walk(64)
        rest(6)
        snap(7 * 64)
        # ... and a wave oscillator again
        be.unit_write(wave_voice[0], 0, sc.wave_ids[3])
        sc.walk(64)
        rest(7)
        snap(8 * 64)
        rest(8)
        snap(8 * 64)
        res.append(got)
        be.close()
    for k, ((a, na), (b, nb)) in enumerate(zip(*res)):
        assert first_diff(a, b) is None, f"batch {k}: (ch, frame, gpu, oracle) = {first_diff(a, b)}"
        assert na == nb, f"batch {k}: noise word {na:#x} against the oracle's {nb:#x}"


@pytest.mark.gpu
def test_refusals_leave_the_recording_alone(oracle_lib):
    gpu, ora = make_gpu(max_batch=8), make_oracle(oracle_lib)
    scs = []
    for be in (gpu, ora):
        be.noise.value = SEED0
        scs.append(noise_scene(be, 3, 2))
    sg, so = scs
    lib, word = gpu.lib, ctypes.c_uint32(0)

    def refused(n=3):
        word.value = gpu.noise.value
        rc = lib.a2amd_fragment_repeat_noise(gpu.ctx, 64, n, ctypes.byref(word))
        assert word.value == gpu.noise.value
        return rc

    def both(f):
        for be, sc in ((gpu, sg), (ora, so)):
            f(be, sc)

    def same(frames):
        a, b = gpu.render(frames), ora.render(frames)
        assert first_diff(a, b) is None, first_diff(a, b)
        assert gpu.noise.value == ora.noise.value

    # no fragment walked by calls yet: nobody's place in the walk is known
    assert refused() == ESTATE
    both(lambda be, sc: sc.walk(64))
    # plain fragment_repeat still refuses noise
    assert lib.a2amd_fragment_repeat(gpu.ctx, 64, 3) == EUNSUPPORTED
    # a pitch ramp in flight on a noise oscillator
    both(lambda be, sc: be.unit_write(sc.two[0], 1, synth.fix(4.0), 0, 400 << 8))
    assert refused() == EUNSUPPORTED
    both(lambda be, sc: [sc.walk(64) for _ in range(3)])
    same(4 * 64)
    # ... still in flight after fragments walked by calls (400 frames: seven of them and one to settle)
    both(lambda be, sc: sc.walk(64))
    assert refused() == EUNSUPPORTED
    both(lambda be, sc: [sc.walk(64) for _ in range(7)])
    same(8 * 64)
    both(lambda be, sc: sc.walk(64))
    gpu.fragment_repeat_noise(64, 4)
    [so.walk(64) for _ in range(4)]
    same(5 * 64)
    # a noise voice born since the last walked fragment
    both(lambda be, sc: sc.add_voices(1, "noise-pan", total=40))
    assert refused() == ESTATE
    both(lambda be, sc: [sc.walk(64) for _ in range(2)])
    same(2 * 64)
    # KEEP / replay of a batch with device-seeded windows
    both(lambda be, sc: sc.walk(64))
    gpu.fragment_repeat_noise(64, 2)
    [so.walk(64) for _ in range(2)]
    with pytest.raises(RuntimeError, match="device-seeded"):
        gpu.render(3 * 64, phases=15 | 16)
    gpu.render(3 * 64, phases=4)           # (upload only)
    assert lib.a2amd_replay(gpu.ctx, 1) == EUNSUPPORTED
    a = gpu.render(3 * 64, phases=1 | 2 | 8)
    b = ora.render(3 * 64)
    assert first_diff(a, b) is None, first_diff(a, b)
    assert gpu.noise.value == ora.noise.value
    # ... and after it replay has nothing to run
    assert lib.a2amd_replay(gpu.ctx, 1) < 0
    # a write to a noise voice between two stretches belongs to a fragment walked by calls
    both(lambda be, sc: sc.walk(64))
    gpu.fragment_repeat_noise(64, 2)
    [so.walk(64) for _ in range(2)]
    both(lambda be, sc: be.unit_write(sc.two[0], 2, synth.fix(0.08)))
    assert refused() == ESTATE
    both(lambda be, sc: sc.walk(64))
    same(4 * 64)
    gpu.close()
    ora.close()
