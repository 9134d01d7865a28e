"""k_leaf_oscbare (a2amd_oscbare.hip): bare `struct { wtosc }` voices - one oscillator wired straight into channel 0 of
its parent's bus - in a quiet kernel of their own in the batches in which they carry no record, gliding or not; and the
mono groups `inline 0 1; panmix 1 > 2` that usually hold them on k_bus_driver.  Every rendering bit for bit against the
oracle's render of the same calls, batch by batch, and every batch with who rendered what (a2amd_last_batch_bare,
a2amd_last_batch_buses): a test that names a kernel proves the kernel rendered."""
import ctypes
import os
import re

import numpy as np
import pytest

from audiality2_amd import synth
from audiality2_amd.replay import Trace, a2amd_vm_state, replay
from conftest import GOLDEN, ROOT, fnv1a_fragments, make_gpu, make_oracle
from test_gpu_parity import first_diff, is_gpu, last_batch

fix = synth.fix


# ---- CPU ---------------------------------------------------------------------------------
def test_header_and_exports(gpu_lib):
    text = open(os.path.join(ROOT, "include", "a2amd_oscbare.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(a2amd_[a-z_0-9]+)\s*\(", text)))
    assert syms == ["a2amd_last_batch_bare"]
    for s in syms:
        assert hasattr(gpu_lib, s), f"liba2amd.so lacks {s}"
    assert '#include "a2amd_oscbare.h"' in open(os.path.join(ROOT, "include", "a2amd.h")).read()


# ---- GPU ---------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def snap(be, frames, got):
    """render, and - on the GPU - who rendered what: (audio, noise word, bare info, bus info, batch info)"""
    a = be.render(frames)
    on = is_gpu(be)
    got.append((a, be.noise.value, be.last_batch_bare() if on else None, be.last_batch_buses() if on else None,
                last_batch(be) if on else None))


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
        assert first_diff(g[0], w[0]) is None, f"batch {k}: (ch, frame, gpu, oracle) = {first_diff(g[0], w[0])}"
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
    compare(got, _oracle[key])
    return got


def auto_vpw(n, forced=None):
    """launch_leaves' voices per wavefront: A2AMD_VPW when set, else one wavefront per SIMD before the lanes fill"""
    return min(max(forced if forced is not None else (n + 1023) // 1024, 1), 64)


# -- 1. shapes and buses --
def split_bare(n):
    """n bare voices over (root, mono group, stereo group, nested mono group, delay group): in list order - sorted by
    bus, the buses in the order of their owners' birth - a 64-voice wavefront of the 130-voice scene spans the root's
    stereo bus (1), a mono bus (40) and a stereo bus (23 of 30), and its last wavefront holds 2 voices"""
    root = 1 if n >= 1 else 0
    rest = n - root
    m1 = rest * 40 // 129
    st = rest * 30 // 129
    m2 = rest * 20 // 129
    return root, m1, st, m2, rest - m1 - st - m2


def shapes_scene(be, nbare):
    be.noise.value = 0x12345
    sc = synth.Scene(be)
    sc.root()
    nroot, n1, nst, n2, ndl = split_bare(nbare)
    total = nbare + 12
    m1 = sc.add_mono_group(pan=0.3)
    sc.add_voices(n1, "osc", group=m1, total=total)
    st = sc.add_bus_group()
    sc.add_voices(nst, "osc", group=st, total=total)
    sc.add_voices(5, "osc-pan", group=st, total=total)
    m2 = sc.add_mono_group(parent=st, pan=-0.55, xinsert=True)
    sc.add_voices(n2, "osc", group=m2, total=total)
    dl = sc.add_group()
    sc.add_voices(ndl, "osc", group=dl, total=total)
    sc.add_voices(3, "osc-pan", group=dl, total=total)
    sc.add_voices(nroot, "osc", total=total)
    return sc


SHAPE_BATCHES = [[64], [64], [64] * 8, [64] * 64, [64, 17, 1, 64, 17, 1, 64], [64] * 8]


def shapes_script(nbare):
    def script(be):
        sc = shapes_scene(be, nbare)
        got = []
        for frames in SHAPE_BATCHES:
            snap(be, walk(sc, frames), got)
        return got
    return script


def check_shapes(got, nbare, vpw, off=False):
    for k, (_a, _n, bi, bus, gen) in enumerate(got):
        first = k == 0
        if off:
            assert (bi.launched, bi.class_voices, bi.quiet_voices, bi.record_voices) == (0, 0, 0, 0), (k, bi)
        elif first:      # (births: every voice carries its records)
            assert (bi.launched, bi.class_voices, bi.quiet_voices, bi.gliding_voices, bi.record_voices) == (0, nbare, 0, 0, nbare), (k, bi)
            assert gen.general_voices == nbare, (k, gen)
        else:
            assert (bi.launched, bi.class_voices, bi.quiet_voices, bi.gliding_voices, bi.record_voices, bi.vpw) == (
                1, nbare, nbare, 0, 0, vpw), (k, bi)
            assert gen.general_voices == 0, (k, gen)
        assert bi.mono_drivers == 2, (k, bi)
        if not first:
            # root, the two mono groups and the stereo group on k_bus_driver, the delay group on k_bus_fbdchain
            assert (bus.driver_voices, bus.fbd_voices, bus.generic_voices) == (4, 1, 0), (k, bus)


@gpu
@pytest.mark.parametrize("vpw", [None, 1, 3, 64])
def test_shapes_and_buses(oracle_lib, monkeypatch, vpw):
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    if vpw is None:
        monkeypatch.delenv("A2AMD_VPW", raising=False)
    else:
        monkeypatch.setenv("A2AMD_VPW", str(vpw))
    got = both(oracle_lib, ("shapes", 130), shapes_script(130))
    check_shapes(got, 130, auto_vpw(130, vpw))


@gpu
@pytest.mark.parametrize("nbare", [1, 63, 64, 65])
def test_list_lengths_around_a_wavefront(oracle_lib, monkeypatch, nbare):
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    monkeypatch.setenv("A2AMD_VPW", "64")
    got = both(oracle_lib, ("shapes", nbare), shapes_script(nbare))
    check_shapes(got, nbare, 64)


@gpu
def test_bare_voices_reach_channel_0_only(oracle_lib, monkeypatch):
    """a stereo group holding only bare voices, its pan at rest in the middle: channel 1 of all it feeds is silent"""
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    monkeypatch.delenv("A2AMD_VPW", raising=False)

    def script(be):
        sc = synth.Scene(be)
        sc.root()
        st = sc.add_bus_group()
        sc.add_voices(7, "osc", group=st, total=16)
        got = []
        for frames in ([64], [64] * 8, [64] * 3):
            snap(be, walk(sc, frames), got)
        return got

    got = both(oracle_lib, "ch0", script)
    for k, (a, _n, bi, bus, _g) in enumerate(got):
        assert np.abs(a[0]).max() > 0 and not a[1].any(), k
        assert (bi.launched, bi.quiet_voices) == ((0, 0) if k == 0 else (1, 7)), (k, bi)
        assert bi.mono_drivers == 0 and bus.generic_voices == (2 if k == 0 else 0), (k, bi, bus)      # (births: records)


# -- 2. waves --
def waves_script(be):
    be.noise.value = 0x777
    sc = synth.Scene(be)
    sc.root()
    m = sc.add_mono_group(pan=0.2)
    n = np.arange(1000)
    odd = (np.sin(n * 2.0 * np.pi * 3 / 1000) * 30000.0).astype(np.int16)
    sizes, data = synth.wave_pyramid(odd)
    w_odd = be.wave_upload(0x900, synth.WMIPWAVE, synth.LOOPED, 1000, sizes + [0] * (synth.MIPLEVELS - len(sizes)), data)
    n = np.arange(2800)
    shot = (np.sin(n * 2.0 * np.pi / 70) * 28000.0 * (1.0 - n / 2800.0)).astype(np.int16)
    sizes, data = synth.wave_pyramid(shot, looped=False)
    w_shot = be.wave_upload(0x901, synth.WMIPWAVE, 0, 256, sizes + [0] * (synth.MIPLEVELS - len(sizes)), data)

    def voice(wave, pitch, amp=0.2):
        u = be.unit_init(sc._key(), synth.K_WTOSC, synth.PROCADD, 0, 1, 1)
        if wave is not None:
            be.unit_write(u, 0, wave)
        be.unit_write(u, 1, fix(pitch))
        be.unit_write(u, 2, fix(amp))
        m["leaves"].append([u])
        return u

    sc.add_voices(3, "osc", group=m, total=16)          # the built-in looped cycles (mip level 3 at these pitches)
    v_odd = voice(w_odd, 0.4)                           # 1 000 samples: the modulo wrap
    v_shot = voice(w_shot, 0.0)                         # a one-shot wave, 1.4 samples a frame: over near frame 2 000
    v_high = voice(sc.wave_ids[1], 3.3)                 # mip levels further up: the phase's low bits dropped every fragment
    v_out = voice(sc.wave_ids[2], 8.5)                  # beyond A2D_MAXPHINC at the last level: silence, the phase runs
    v_none = voice(None, 0.0, 0.0)                      # never given a wave ...
    be.unit_write(v_none, 2, fix(0.3), 0, 3000 << 8)    # ... an amplitude ramp running all the same
    got = []
    snap(be, walk(sc, [64]), got)
    snap(be, walk(sc, [64] * 48), got)                  # the one-shot wave ends in here
    snap(be, walk(sc, [64] * 8), got)
    snap(be, walk(sc, [64, 30, 64]), got)
    # what the kernel stored is what the general kernel goes on from: the ramp that ran unheard, the phases
    be.unit_write(v_none, 0, sc.wave_ids[5])
    be.unit_write(v_out, 1, fix(0.25))
    for u in (v_odd, v_shot, v_high):
        be.unit_write(u, 2, fix(0.1), 100, 0)
    snap(be, walk(sc, [64] * 4), got)
    snap(be, walk(sc, [64] * 8), got)
    return got


@gpu
def test_waves(oracle_lib, monkeypatch):
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    monkeypatch.delenv("A2AMD_VPW", raising=False)
    got = both(oracle_lib, "waves", waves_script)
    want = [(0, 0, 0, 8), (1, 8, 1, 0), (1, 8, 1, 0), (1, 8, 0, 0), (1, 3, 0, 5), (1, 8, 0, 0)]
    # (gliding: the voice without a wave, 3 000 frames from frame 0 on - by the host's bound until frame 3 256: the batches
    # that begin at frames 64 and 3 136)
    assert [(i.launched, i.quiet_voices, i.gliding_voices, i.record_voices) for _a, _n, i, _b, _g in got] == want
    for _a, _n, i, bus, _g in got[1:]:
        assert i.class_voices == 8 and i.mono_drivers == 1 and bus.generic_voices == 0


# -- 3. glides and handover --
GLIDE_BATCH = 8         # fragments


def glides_script(be):
    be.noise.value = 0x4242
    sc = synth.Scene(be)
    sc.root()
    m = sc.add_mono_group(pan=-0.3)
    sc.add_voices(9, "osc", group=m, total=16)
    st = sc.add_bus_group()
    sc.add_voices(4, "osc", group=st, total=16)
    v = [units[0] for units in m["leaves"]]
    got = []
    one = [64] * GLIDE_BATCH
    snap(be, walk(sc, one), got)                        # 0: births
    snap(be, walk(sc, one), got)                        # 1: quiet
    be.unit_write(v[0], 2, fix(0.5), 0, 1300 << 8)      # an amplitude ramp longer than two batches
    be.unit_write(v[1], 2, fix(0.02), 0, 612 << 8)      # ... one that ends 36 frames into a fragment of the next batch
    be.unit_write(v[2], 1, fix(2.4), 0, 1000 << 8)      # a pitch glide of two octaves and more: across mip levels
    be.unit_write(v[3], 1, fix(-0.7), 128, 0)           # a start offset, no duration
    for _ in range(6):                                  # 2: the records; 3 - 7: gliding, then at rest
        snap(be, walk(sc, one), got)
    be.unit_write(v[0], 2, fix(0.1), 30, 400 << 8)      # back to the general kernel from what k_leaf_oscbare stored
    be.unit_write(v[2], 1, fix(0.0), 0, 0)
    be.unit_write(m["leaves"][5][0], 3, 12345)
    snap(be, walk(sc, one), got)                        # 8
    snap(be, walk(sc, one), got)                        # 9
    return got


def check_glides(got):
    span = 64 * GLIDE_BATCH
    t_write = 2 * span
    durs = (1300, 612, 1000)
    want = [(0, 0, 0, 13), (1, 13, 0, 0), (1, 9, 0, 4)]
    for k in range(3, 8):       # a2amd_unit_write's bound: the write's frame + 64 + duration + 192
        want.append((1, 13, sum(t_write + 256 + d > k * span for d in durs), 0))
    assert [w[2] for w in want[3:]] == [3, 2, 1, 0, 0]
    want += [(1, 10, 0, 3), (1, 13, 1, 0)]
    assert [(i.launched, i.quiet_voices, i.gliding_voices, i.record_voices) for _a, _n, i, _b, _g in got] == want
    for k, (_a, _n, i, bus, gen) in enumerate(got):
        assert i.class_voices == 13 and i.mono_drivers == 1, (k, i)
        assert gen.general_voices == i.record_voices and gen.n_moving_listed == 0, (k, gen)
        if k:
            assert bus.generic_voices == 0, (k, bus)


@gpu
def test_glides_and_handover(oracle_lib, monkeypatch):
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    monkeypatch.delenv("A2AMD_VPW", raising=False)
    check_glides(both(oracle_lib, "glides", glides_script, max_batch=GLIDE_BATCH))


# -- 4. births, deaths, waves changed --
@gpu
def test_births_deaths_and_waves_changed(oracle_lib, monkeypatch):
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    monkeypatch.delenv("A2AMD_VPW", raising=False)

    def script(be):
        be.noise.value = 0xbeef
        sc = synth.Scene(be)
        sc.root()
        m = sc.add_mono_group(pan=0.6)
        sc.add_voices(6, "osc", group=m, total=16)
        got = []
        one = [64] * 4
        snap(be, walk(sc, one), got)                    # 0: births
        snap(be, walk(sc, one), got)                    # 1: 6 quiet
        dead = m["leaves"].pop(2)
        be.unit_deinit(dead[0])
        snap(be, walk(sc, one), got)                    # 2: the dying voice is listed to the end of its batch
        snap(be, walk(sc, one), got)                    # 3: 5 quiet
        sc.add_voices(2, "osc", group=m, total=16)      # two births: the slot is used again
        snap(be, walk(sc, one), got)                    # 4
        snap(be, walk(sc, one), got)                    # 5: 7 quiet
        be.unit_write(m["leaves"][0][0], 0, sc.wave_ids[9])
        be.unit_write(m["leaves"][1][0], 0, sc.noise_id)
        snap(be, walk(sc, one), got)                    # 6: two voices with records
        snap(be, walk(sc, one), got)                    # 7: the noise voice has a record in every window
        snap(be, walk(sc, [64, 21, 64]), got)           # 8
        return got

    got = both(oracle_lib, "births", script, max_batch=4)
    want = [(0, 6, 0, 6), (1, 6, 6, 0), (1, 6, 5, 1), (1, 5, 5, 0), (1, 7, 5, 2), (1, 7, 7, 0), (1, 7, 5, 2), (1, 7, 6, 1),
            (1, 7, 6, 1)]
    assert [(i.launched, i.class_voices, i.quiet_voices, i.record_voices) for _a, _n, i, _b, _g in got] == want


# -- 5. A/B --
@gpu
def test_switched_off_is_the_same_audio(oracle_lib, monkeypatch):
    """A2AMD_NO_FAST=256: no class, no launch - every bare voice the general kernel's, as before the class existed"""
    monkeypatch.setenv("A2AMD_NO_FAST", "256")
    monkeypatch.delenv("A2AMD_VPW", raising=False)
    check_shapes(both(oracle_lib, ("shapes", 130), shapes_script(130)), 130, 0, off=True)
    got = both(oracle_lib, "glides", glides_script, max_batch=GLIDE_BATCH)
    for k, (_a, _n, i, _b, _g) in enumerate(got):
        assert (i.launched, i.class_voices, i.quiet_voices, i.gliding_voices, i.record_voices) == (0, 0, 0, 0, 0), (k, i)
        assert i.mono_drivers == 1, (k, i)


# -- 6. mono drivers --
def mono_script(be):
    be.noise.value = 0x99
    sc = synth.Scene(be)
    sc.root()
    a = sc.add_mono_group(pan=0.25)                     # inline 0 1; panmix+ 1 > 2
    b = sc.add_mono_group(pan=1.5, xinsert=True)        # inline 0 1; panmix 1 2; xinsert+ 2 >, the pan beyond +1: the clamp
    c = sc.add_bus_group()
    d = sc.add_mono_group(parent=c, pan=-1.75)
    e = sc.add_mono_group()                             # its pan never written
    for g, n in ((a, 5), (b, 4), (d, 3), (e, 2)):
        sc.add_voices(n, "osc", group=g, total=16)
    sc.add_voices(3, "osc-pan", group=c, total=16)
    got = []
    one = [64] * 8
    snap(be, walk(sc, one), got)                        # 0: births
    for _ in range(3):                                  # 1 - 3: at rest; 2 and 3 live on what the drivers zeroed
        snap(be, walk(sc, one), got)
    be.unit_write(a["units"][1], 1, fix(-0.9), 0, 700 << 8)     # a pan glide
    be.unit_write(b["units"][1], 0, fix(0.5), 0, 900 << 8)      # ... and a volume glide on the three-unit shape
    for _ in range(4):                                  # 4: the records; 5, 6: ramping; 7: at rest
        snap(be, walk(sc, one), got)
    be.unit_write(d["units"][1], 1, fix(0.4), 128, 0)   # a start offset, no duration
    snap(be, walk(sc, one), got)                        # 8: that owner with the general kernel
    snap(be, walk(sc, [64, 40, 64]), got)               # 9: back on k_bus_driver
    snap(be, walk(sc, one), got)                        # 10
    return got


@gpu
def test_mono_drivers(oracle_lib, monkeypatch):
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    monkeypatch.delenv("A2AMD_VPW", raising=False)
    got = both(oracle_lib, "mono", mono_script, max_batch=8)
    buses = [b for _a, _n, _i, b, _g in got]
    # six owners: root, a, b, c, d, e
    for k in (1, 2, 3, 7, 10):
        assert (buses[k].driver_voices, buses[k].generic_voices, buses[k].fbd_voices, buses[k].consume) == (6, 0, 0, 3), (k, buses[k])
    assert [buses[k].driver_ramping for k in (2, 3, 7, 10)] == [0, 0, 0, 0]
    assert (buses[4].driver_voices, buses[4].generic_voices) == (4, 2), buses[4]
    # (the host's bound, a2amd_bus.h: the write's frame 2 048 + 256 + 700 / 900 frames - batches 5 and 6 begin at 2 560 and 3 072)
    for k, n in ((5, 2), (6, 1)):
        assert (buses[k].driver_voices, buses[k].driver_ramping, buses[k].generic_voices, buses[k].consume) == (6, n, 0, 3), (k, buses[k])
    assert (buses[8].driver_voices, buses[8].generic_voices) == (5, 1), buses[8]
    assert (buses[9].driver_voices, buses[9].driver_ramping, buses[9].generic_voices) == (6, 0, 0), buses[9]
    for k, (_a, _n, i, _b, _g) in enumerate(got):
        assert i.mono_drivers == 4 and i.class_voices == 14, (k, i)
        assert (i.launched, i.quiet_voices) == ((0, 0) if k == 0 else (1, 14)), (k, i)


@gpu
def test_mono_drivers_switched_off(oracle_lib, monkeypatch):
    """A2AMD_NO_FAST=4: every bus owner the general kernel's, mono or not - the same audio"""
    monkeypatch.setenv("A2AMD_NO_FAST", "4")
    monkeypatch.delenv("A2AMD_VPW", raising=False)
    got = both(oracle_lib, "mono", mono_script, max_batch=8)
    for k, (_a, _n, i, bus, _g) in enumerate(got):
        assert i.mono_drivers == 0 and bus.driver_voices == 0 and bus.generic_voices == 6 and bus.consume == 0, (k, i, bus)


# -- 7. replay --
@gpu
def test_state_travels_through_replays(oracle_lib, monkeypatch):
    """A record-free batch of quiet bare voices under a mono group, kept and re-run by a2amd_replay: what the kernel
    stores at the end of one run is what the next begins with - the batches behind the replays equal the oracle's."""
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    monkeypatch.delenv("A2AMD_VPW", raising=False)
    one = [64] * 8

    def scene(be):
        sc = synth.Scene(be)
        sc.root()
        m = sc.add_mono_group(pan=0.1)
        sc.add_voices(20, "osc", group=m, total=32)
        return sc

    ora = make_oracle(oracle_lib)
    sc = scene(ora)
    want = [ora.render(walk(sc, one)) for _ in range(6)]
    ora.close()

    be = make_gpu(max_batch=8)
    sc = scene(be)
    infos = []

    def info():
        infos.append(be.last_batch_bare())

    a0 = be.render(walk(sc, one))
    info()
    a1 = be.render(walk(sc, one), phases=15 | 16)       # kept ...
    info()
    be.lib.a2amd_replay.argtypes = [ctypes.c_void_p, ctypes.c_uint]
    be.lib.a2amd_replay.restype = ctypes.c_int
    assert be.lib.a2amd_replay(be.ctx, 2) == 0          # ... run twice more, unheard ...
    info()
    a4 = be.render(8 * 64)                              # ... and once more, heard: the fifth batch
    info()
    a5 = be.render(walk(sc, one))                       # walked by calls again
    info()
    be.close()
    for k, (a, w) in enumerate(((a0, want[0]), (a1, want[1]), (a4, want[4]), (a5, want[5]))):
        assert first_diff(a, w) is None, f"{k}: (ch, frame, gpu, oracle) = {first_diff(a, w)}"
        assert np.abs(a).max() > 0
    assert [(i.launched, i.quiet_voices, i.record_voices) for i in infos] == [(0, 0, 20)] + [(1, 20, 0)] * 4


# -- 8. device VM --
@gpu
def test_a_voice_the_device_vm_runs_is_not_of_the_class(oracle_lib, monkeypatch):
    """20 quiet bare voices and one bare voice handed to the device VM with the looping program test_device_vm.py uses for
    `wtosc; panmix` (for { +p .01; d 3; -p .01; d 3 }: a pitch ramp every 144 frames): from its adoption on the voice is
    the general kernel's - never in class_voices - in the batches in which its VM writes and in those in which it sleeps
    (one-fragment batches: about every second one), and the audio is the oracle's, which gets the same writes and windows
    as calls (made by the host copy of the interpreter).  Should a2amd_vm_adopt refuse the chain, the refusal is asserted
    and the voice stays of the class."""
    from test_device_vm import MSDUR, R_SEG, R_WRITE, WTOSC, VmState, asm, fx, trace_host
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    monkeypatch.delenv("A2AMD_VPW", raising=False)
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
        m = sc.add_mono_group(pan=-0.2)
        sc.add_voices(20, "osc", group=m, total=32)
        x = be.unit_init(sc._key(), synth.K_WTOSC, synth.PROCADD, 0, 1, 1)
        be.unit_write(x, 0, sc.wave_ids[4])
        be.unit_write(x, 1, pitch)
        be.unit_write(x, 2, fix(0.25))
        return sc, m, x

    def walk1(be, sc, m, x_calls):
        """Scene.walk for this tree, the voice x by x_calls(): calls, or the default map"""
        be.fragment(64)
        be.unit_process(sc.rootv[0], 0, 64)
        be.unit_process(m["units"][0], 0, 64)
        for units in m["leaves"]:
            be.unit_process(units[0], 0, 64)
        x_calls()
        be.inline_end(m["units"][0])
        be.unit_process(m["units"][1], 0, 64)
        be.inline_end(sc.rootv[0])
        be.unit_process(sc.rootv[1], 0, 64)
        be.unit_process(sc.rootv[2], 0, 64)

    # the GPU
    be = make_gpu(max_batch=4)
    sc, m, x = scene(be)
    got, infos = [], []
    walk1(be, sc, m, lambda: be.unit_process(x, 0, 64))
    got.append(be.render(64))
    infos.append(be.last_batch_bare())
    walk1(be, sc, m, lambda: be.unit_process(x, 0, 64))
    prog = be.vm_program(0x5150, list(code))
    assert prog >= 0
    adopted = be.vm_adopt(x, prog, a2amd_vm_state.from_buffer_copy(state()), {5: (x, 1)}, 64 << 8, MSDUR, check=False)
    print("a2amd_vm_adopt:", adopted)
    if adopted != 0:
        assert adopted == -4, adopted                   # A2AMD_EUNSUPPORTED: the chain stays the engine's
    got.append(be.render(64))
    infos.append(be.last_batch_bare())
    for frames in plan:
        for _ in frames:
            walk1(be, sc, m, (lambda: be.mark_default([x])) if adopted == 0 else (lambda: be.unit_process(x, 0, 64)))
        got.append(be.render(sum(frames)))
        infos.append(be.last_batch_bare())
    be.close()

    # the oracle: the VM's writes and windows as calls
    ora = make_oracle(oracle_lib)
    sc, m, x = scene(ora)
    recs = {}
    if adopted == 0:
        for frag, op, _unit, reg, value, dur, start in trace_host(code, n, state(), [5], [(0, 1)], [WTOSC], [64] * nfr, now=128 << 8):
            recs.setdefault(frag, []).append((op, reg, value, dur, start))
        assert sum(1 for f in range(12) if f in recs) in range(3, 10)       # one-fragment batches with writes, and without

    def vm_calls(f):
        def calls():
            if f not in recs:
                ora.unit_process(x, 0, 64)
            for op, reg, value, dur, start in recs.get(f, ()):
                if op == R_SEG:
                    ora.unit_process(x, dur & 0xffff, dur >> 16)
                else:
                    assert op == R_WRITE
                    ora.unit_write(x, reg, value, start, dur)
        return calls

    want = []
    for _ in range(2):
        walk1(ora, sc, m, lambda: ora.unit_process(x, 0, 64))
        want.append(ora.render(64))
    f = 0
    for frames in plan:
        for _ in frames:
            walk1(ora, sc, m, vm_calls(f))
            f += 1
        want.append(ora.render(sum(frames)))
    ora.close()
    for k, (a, w) in enumerate(zip(got, want)):
        assert first_diff(a, w) is None, f"batch {k}: (ch, frame, gpu, oracle) = {first_diff(a, w)}"
    cls = 20 if adopted == 0 else 21
    assert [(i.launched, i.class_voices, i.quiet_voices, i.record_voices) for i in infos] == [(0, 21, 0, 21)] + [(1, cls, cls, 0)] * (1 + len(plan))


# -- 9. a song --
@gpu
def test_a_song_goes_through_both_paths(monkeypatch):
    """k2intro in batches of 7 fragments, hash-equal to the fixture, with some batch in which k_leaf_oscbare rendered and
    some batch with mono owners on k_bus_driver's lists.  1 100 fragments, not 700: the song's first bare voices and its
    first mono group are born in fragment 719 (the trace's first `wtosc+ 0>1` and `inline 0 1; panmix+ 1>2` chains) - the
    first 700 fragments hold none, and the two assertions could not be met by any implementation."""
    nfr = 1100
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    monkeypatch.delenv("A2AMD_VPW", raising=False)
    tr = Trace(os.path.join(GOLDEN, "k2intro.trace.xz"))
    cfg = tr.config
    be = make_gpu(cfg["samplerate"], cfg["basepitch"], cfg["channels"], max_batch=7)
    infos = []
    render = be.render

    def spy(*a, **kw):
        out = render(*a, **kw)
        infos.append(be.last_batch_bare())
        return out

    be.render = spy
    out = replay(tr, be, batch=7, check_noise=True, max_fragments=nfr)
    be.close()
    want = np.load(os.path.join(GOLDEN, "k2intro.hash.npy"))[:nfr]
    got = fnv1a_fragments(out)
    assert nfr - 100 < len(got) <= nfr
    bad = np.nonzero(got != want[:len(got)])[0]
    assert not bad.size, bad[:4]
    print("batches with bare voices:", sum(i.class_voices > 0 for i in infos), "with quiet ones:", sum(i.quiet_voices > 0 for i in infos),
          "with mono drivers:", sum(i.mono_drivers > 0 for i in infos), "of", len(infos))
    assert any(i.launched and i.quiet_voices > 0 for i in infos)
    assert any(i.mono_drivers > 0 for i in infos)
