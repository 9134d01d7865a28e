"""k_bus_fbdpan (a2amd_fast.hip): the delay chains that end in a wired panmix - `inline 0 2; fbdelay 2 2 x 1..4; panmix+ 2 > 2`,
the master section of most songs - against the oracle, with the proof that the kernel was reached
(a2amd_last_batch_fbdpan, include/a2amd_fbdpan.h; a2amd_last_batch_buses, include/a2amd_bus.h).

Every GPU test renders one script on the oracle and on the GPU, compares the audio batch by batch and asserts, batch by
batch, who rendered the bus owners.  The expected counts are tables written down from the script - which write lands in
front of which batch, how long its ramp is - by the frame arithmetic spelled out at each table; none is a recording of
what the library said.  Batches are 10 fragments, one of them 37 frames; six osc-pan leaves in every group.

The tests without the gpu mark check the interface, that `add_group(tail="panmix")` builds the chain, and on the oracle
alone that each script does what it is built for (the rampers restated in test_gpu_bus_paths.py: Ramper, driver_model).

The song.  The issue that asked for this kernel wanted k2intro replayed in batches of 64 fragments, in a window with at
least 8 batches in which the master voice carries no record.  The trace has no such window: a cut window lands on the
master every 61 fragments (3 906 frames: the wake-up of a voice that idles, core.c:1195), so at 64 fragments a batch 69
of its 71 batches carry a record on the master and are the general kernel's - test_song_premise states that as a fact
of the fixture.  The reach of the kernel is therefore shown at 16 fragments a batch, where three batches in four are
record-free (30 of the window's 40), and the replay at 64 is kept for the other half of the claim: every batch the
general kernel's, the audio the reference's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from audiality2_amd import synth
from audiality2_amd.replay import (T_DEINIT, T_FRAGMENT, T_INIT, T_PROCESS, T_WAVEDROP, T_WRITE, Trace, a2amd_bus_info,
                                   a2amd_fbdpan_batch_info, replay)
from conftest import GOLDEN, ROOT, fnv1a_fragments, make_gpu, make_oracle
from test_gpu_bus_paths import Ramper, bound_ramping, driver_model, first_diff, frag_plan, render_async, run_script  # noqa: F401

fix = synth.fix
PAN, VOL = 1, 0
BUFSIZE = 131072
FRAGS = 10
GAINS = (0.4, 0.3, 0.35)
BUS = ("driver_voices", "driver_ramping", "driver_windows_dropped", "fbd_voices", "generic_voices")
FP = ("launched", "class_voices", "quiet_voices", "gliding_voices", "record_voices", "max_delays")


def counts(bi, names):
    return tuple(int(getattr(bi, n)) for n in names)


def tap_frames(ms):
    return int(fix(ms) * 48000 / 65536000)


def rounds(taps):
    """fragments per round of the delay kernels for a chain with these taps (ms)"""
    frames = [tap_frames(ms) for triple in taps for ms in triple]
    assert all(64 <= t <= BUFSIZE - 64 for t in frames)
    return min(min(frames), BUFSIZE - max(frames)) // 64


def pan_group(sc, taps, vol=None, pan=None, parent=None, mid_add=False):
    be = sc.be
    g = sc.add_group(fb=list(taps), gains=GAINS, delays=len(taps), mid_add=mid_add, parent=parent, tail="panmix")
    if vol is not None:
        be.unit_write(g["units"][-1], VOL, fix(vol))
    if pan is not None:
        be.unit_write(g["units"][-1], PAN, fix(pan))
    return g


def spy(be, pinfo, render=None):
    """a render that also collects a2amd_last_batch_fbdpan()"""
    def r(frames):
        out = render(frames) if render else be.render(frames)
        pinfo.append(be.last_batch_fbdpan())
        return out
    return r


@pytest.fixture(scope="module")
def oracle_memo(oracle_lib):
    """one oracle render per script, shared by the tests that need it, read-only"""
    memo = {}

    def get(key, script):
        if key not in memo:
            ora = make_oracle(oracle_lib)
            memo[key] = script(ora)
            ora.close()
            for w in memo[key]:
                w.setflags(write=False)
        return memo[key]
    return get


def on_gpu(script, max_batch=FRAGS, use_async=False):
    """the script on the GPU: (audio, a2amd_bus_info per batch, a2amd_fbdpan_batch_info per batch)"""
    gpu = make_gpu(max_batch=max_batch)
    info, pinfo = [], []
    got = script(gpu, info=info, render=spy(gpu, pinfo, (lambda frames: render_async(gpu, frames)) if use_async else None))
    gpu.close()
    return got, info, pinfo


# ---------------------------------------------------------------------------
# the interface
# ---------------------------------------------------------------------------
def test_abi(gpu_lib):
    text = open(os.path.join(ROOT, "include", "a2amd_fbdpan.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(a2amd_[a-z_0-9]+)\s*\(", text))) == ["a2amd_last_batch_fbdpan"]
    assert '#include "a2amd_fbdpan.h"' in open(os.path.join(ROOT, "include", "a2amd.h")).read()
    assert hasattr(gpu_lib, "a2amd_last_batch_fbdpan")      # (gpu_lib: liba2amd.so loaded, no device needed)
    assert C.sizeof(a2amd_fbdpan_batch_info) == 32
    assert C.sizeof(a2amd_bus_info) == 28                   # seven words, as before this class
    assert [n for n, _ in a2amd_fbdpan_batch_info._fields_] == list(FP) + ["reserved"]
    # NULL arguments are refused, not dereferenced
    gpu_lib.a2amd_last_batch_fbdpan.restype = C.c_int
    gpu_lib.a2amd_last_batch_fbdpan.argtypes = [C.c_void_p, C.c_void_p]
    assert gpu_lib.a2amd_last_batch_fbdpan(None, None) != 0


class Recorder:
    """a backend that writes down the unit_init calls"""
    def __init__(self):
        self.inits, self.writes = [], []

    def wave_upload(self, *a):
        return 0

    def unit_init(self, key, kind, flags, nin, nout, wired, **kw):
        self.inits.append((key, kind, flags, nin, nout, wired))
        return len(self.inits) - 1

    def unit_write(self, unit, reg, value, start=0, dur=0, transpose=0):
        self.writes.append((unit, reg, value))


def test_scene_builds_the_chain():
    K = synth
    for delays, mid_add, adding in ((1, False, set()), (2, False, set()), (4, [1, 3], {1, 3})):
        rec = Recorder()
        sc = synth.Scene(rec, nwaves=1)
        g = sc.add_group(delays=delays, mid_add=mid_add, tail="panmix")
        key = rec.inits[0][0]
        want = [(key, K.K_INLINE, 0, 0, 2, 0)]
        want += [(key, K.K_FBDELAY, K.PROCADD if i in adding else 0, 2, 2, 0) for i in range(delays)]
        want += [(key, K.K_PANMIX, K.PROCADD, 2, 2, 1)]
        assert rec.inits == want
        assert g["units"] == list(range(delays + 2)) and sc.groups == [g]
        # every delay gets its three taps and three gains, the panmix nothing
        assert sorted({u for u, _r, _v in rec.writes}) == list(range(1, delays + 1))
        assert all(sorted(r for u, r, _v in rec.writes if u == d) == [0, 1, 2, 4, 5, 6] for d in range(1, delays + 1))
    # the default is the wired-delay chain, as before
    rec = Recorder()
    g = synth.Scene(rec, nwaves=1).add_group(delays=3, mid_add=True)
    assert [(k, f, w) for _key, k, f, _i, _o, w in rec.inits] == \
        [(K.K_INLINE, 0, 0), (K.K_FBDELAY, 0, 0), (K.K_FBDELAY, K.PROCADD, 0), (K.K_FBDELAY, K.PROCADD, 1)]
    with pytest.raises(ValueError):
        synth.Scene(Recorder(), nwaves=1).add_group(tail="xinsert")


# ---------------------------------------------------------------------------
# 1. settled (and 4: the same scene with the class switched off)
# ---------------------------------------------------------------------------
S_BATCHES = 6
S_TAPS = {
    "P1": [(2.1, 3.0, 4.0)],                                                            # 100 frames: rounds of 1 fragment
    "P2": [(4.2, 5.0, 6.3), (4.5, 5.5, 7.0)],                                           # 201 frames: of 3
    "P4": [(14.0, 15.0, 17.0), (16.0, 14.5, 19.0), (15.0, 18.0, 21.0), (14.2, 20.0, 16.0)],     # 672 frames: the whole batch
}
S_GAINS = {"P1": (0.8, 0.5), "P2": (0.6, 1.4), "P4": (1.2, -0.3)}       # volume, pan: P2's beyond +1 - clamped at rest
# Bus owners: the root and the bus group Bg (drivers); P1 and P4 under the root, P2 under Bg (depth 2): the class; W, a
# wired chain of two delays.  Every write is made before batch 0, which carries the births: all six owners have records.
# The pan-tailed owners' panmix writes are within the host's bound until frame 256; batch 1 begins at frame 640.
# (launched, class, quiet, gliding, record, max_delays) and (driver, ramping, dropped, fbd, generic):
S_FP0, S_FP = (1, 3, 0, 0, 3, 4), (1, 3, 3, 0, 0, 4)
S_BUS = (2, 0, 0, 1, 0)
S_BUS_OFF = (2, 0, 0, 1, 3)     # A2AMD_NO_FAST=512: the three are general bus owners


def s_plan():
    return frag_plan(S_BATCHES, FRAGS, short=(2, 4))


def s_script(be, render=None, info=None):
    sc = synth.Scene(be, nwaves=4)
    sc.root()
    g = {"P1": pan_group(sc, S_TAPS["P1"], *S_GAINS["P1"])}
    g["Bg"] = sc.add_bus_group()
    g["P2"] = pan_group(sc, S_TAPS["P2"], *S_GAINS["P2"], parent=g["Bg"])
    g["P4"] = pan_group(sc, S_TAPS["P4"], *S_GAINS["P4"], mid_add=[1])
    g["W"] = sc.add_group()
    for name in ("P1", "Bg", "P2", "P4", "W"):
        sc.add_voices(6, chain="osc-pan", group=g[name], total=32)
    assert not sc.leaves
    return run_script(be, sc, s_plan(), render=render, info=info)


def test_settled_script_does_what_it_is_built_for(oracle_memo):
    assert [rounds(S_TAPS[n]) for n in ("P1", "P2", "P4")] == [1, 3, 10]
    assert FRAGS % 3 != 0 and rounds(S_TAPS["P4"]) >= FRAGS
    assert all(v != 1.0 for v, _p in S_GAINS.values())
    assert sorted(abs(p) > 1.0 for _v, p in S_GAINS.values()) == [False, False, True]
    plan = s_plan()
    for vol, pan in S_GAINS.values():
        ws = [(0, VOL, fix(vol), 0, 0), (0, PAN, fix(pan), 0, 0)]
        assert not any(bound_ramping(plan, ws, b) for b in range(1, S_BATCHES))
        model = driver_model(plan, ws)
        assert not any(running for _b, _f, running, _c, _e in model)
        assert all(clamp == (abs(pan) > 1.0) for _b, _f, _r, clamp, _e in model)
    want = oracle_memo("s", s_script)
    assert all(w.any() for w in want)
    assert [w.shape[1] for w in want] == [sum(b) for b in plan]


@pytest.mark.gpu
def test_settled_chains_match_oracle_and_are_the_kernels(oracle_memo, monkeypatch):
    """One, two and four delays (the second of the four adding) in rounds of 1, 3 and 10 fragments, gains computed once,
    the clamp on at rest for P2; one chain under a bus group.  From batch 1 on nobody carries a record: the buses clean
    themselves and the root stores the host's buffer.  From batch 2 on the batches run from a captured graph."""
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    want = oracle_memo("s", s_script)
    got, info, pinfo = on_gpu(s_script, use_async=True)
    for b in range(S_BATCHES):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {pinfo[b]} {info[b]}"
    assert counts(pinfo[0], FP) == S_FP0
    for b in range(1, S_BATCHES):
        assert counts(pinfo[b], FP) == S_FP, f"batch {b}: {pinfo[b]}"
        assert counts(info[b], BUS) == S_BUS, f"batch {b}: {info[b]}"
        assert (info[b].consume, info[b].master_direct) == (3, 1), f"batch {b}: {info[b]}"


@pytest.mark.gpu
def test_class_switched_off_is_the_general_kernel_and_sounds_the_same(oracle_memo, monkeypatch):
    """A2AMD_NO_FAST=512: no voice of the class, the three owners the general kernel's, the wired chain untouched."""
    want = oracle_memo("s", s_script)
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    on, info_on, pinfo_on = on_gpu(s_script)
    monkeypatch.setenv("A2AMD_NO_FAST", "512")
    off, info_off, pinfo_off = on_gpu(s_script)
    for b in range(S_BATCHES):
        assert first_diff(off[b], want[b]) is None, f"batch {b}: {pinfo_off[b]} {info_off[b]}"
        assert first_diff(on[b], off[b]) is None, f"batch {b}"
    for b in range(1, S_BATCHES):
        assert counts(pinfo_on[b], FP) == S_FP and counts(info_on[b], BUS) == S_BUS, f"batch {b}"
        assert counts(pinfo_off[b], FP) == (0, 0, 0, 0, 0, 0), f"batch {b}: {pinfo_off[b]}"
        assert counts(info_off[b], BUS) == S_BUS_OFF, f"batch {b}: {info_off[b]}"
        assert info_off[b].consume == 0


# ---------------------------------------------------------------------------
# 2. gliding
# ---------------------------------------------------------------------------
G_BATCHES, G_WRITE, G_LATE = 8, 2, 4
G_TAPS = {
    "Ga": [(2.1, 3.0, 4.0)],                                            # rounds of 1 fragment
    "Gb": [(4.2, 5.0, 6.3), (4.5, 5.5, 7.0)],                           # of 3
    "Gc": [(5.5, 7.0, 9.0), (6.0, 8.0, 11.0), (5.4, 12.0, 20.0)],       # of 4
    "Gd": [(63.1, 75.6, 100.4), (70.0, 81.0, 90.5)],                    # the whole batch
}


def g_plan():
    return frag_plan(G_BATCHES, FRAGS, short=(3, 6))


def g_writes():
    """group -> its panmix writes (batch, reg, value, start, dur[, behind the group's window of fragment f])"""
    plan = g_plan()
    two = sum(plan[G_WRITE]) + sum(plan[G_WRITE + 1])
    return {
        # ends 21 frames into the fifteenth fragment behind the write: batch 3's fifth
        "Ga": [(G_WRITE, VOL, fix(0.3), 33, ((14 * 64 + 21) << 8) + 77)],
        # at rest beyond +1, then inside over 1 536 frames: the value is inside after half of them, 768 frames behind the
        # write - 128 frames into batch 3, which carries no record: the clamp on in its first fragments, off in its last
        "Gb": [(0, PAN, fix(1.4), 0, 0), (G_WRITE, PAN, fix(0.6), 0, (24 * 64) << 8)],
        # its batch and the next one, whole: over on the batch boundary, the delta stale in the batch behind it
        "Gc": [(G_WRITE, VOL, fix(0.35), 0, two << 8)],
        # behind Gd's last window of batch 4: the timer stays set, batch 5 begins unsettled without a record of its own
        "Gd": [(G_LATE, VOL, fix(0.4), 33, 0, FRAGS - 1)],
    }


# Batches 1 .. 7, (launched, class, quiet, gliding, record, max_delays); t = the frame at which batch 2 begins, a batch is
# 640 frames and batch 3 is 27 short; the host's bound is the ramp's length + 256 (a2amd_bus.h):
#       Ga 917 + 256 = 1173    Gb 1536 + 256 = 1792    Gc 1253 + 256 = 1509    batches 3, 4, 5 begin at t + 640, 1253, 1893
#       Gd is written 576 frames into batch 4: within 0 + 256 of that, which covers the beginning of batch 5 (640) only
#   2: the three written chains carry records.  3: all three within their bounds.  4: Gd carries its record; Gb and Gc.
#   5: Gd.  6, 7: nobody - the rampers are at rest by the end state the kernel stored.
G_FP = [(1, 4, 4, 0, 0, 3), (1, 4, 1, 0, 3, 3), (1, 4, 4, 3, 0, 3), (1, 4, 3, 2, 1, 3), (1, 4, 4, 1, 0, 3), (1, 4, 4, 0, 0, 3),
        (1, 4, 4, 0, 0, 3)]


def g_script(be, ramps=True, render=None, info=None):
    sc = synth.Scene(be, nwaves=4)
    sc.root()
    g = {name: pan_group(sc, taps) for name, taps in G_TAPS.items()}
    for name in g:
        sc.add_voices(6, chain="osc-pan", group=g[name], total=32)
    writes = g_writes() if ramps else {"Gb": g_writes()["Gb"][:1]}
    before = {}
    for name, ws in writes.items():
        for b, reg, value, start, dur, *at in ws:
            if not at:
                before.setdefault(b, []).append((g[name]["units"][-1], reg, value, start, dur))

    def walk(b, f, n):
        sc.walk(n)
        for name, ws in writes.items():
            for wb, reg, value, start, dur, *at in ws:
                if at and (wb, at[0]) == (b, f):
                    be.unit_write(g[name]["units"][-1], reg, value, start, dur)
    return run_script(be, sc, g_plan(), walk=walk, render=render, info=info,
                      before={b: (lambda ws=ws: [be.unit_write(*w) for w in ws]) for b, ws in before.items()})


def test_gliding_script_does_what_it_is_built_for(oracle_memo):
    plan, writes = g_plan(), g_writes()
    assert [rounds(G_TAPS[n]) for n in ("Ga", "Gb", "Gc")] == [1, 3, 4] and rounds(G_TAPS["Gd"]) >= FRAGS
    model = {name: driver_model(plan, ws) for name, ws in writes.items()}
    recs = {name: {w[0] for w in ws if w[0] > 0} for name, ws in writes.items()}
    # Ga's volume ramp is over 21 frames into the fifth fragment of batch 3, a batch without a record
    assert [(b, f, e) for b, f, running, clamp, e in model["Ga"] if e is not None] == [(G_WRITE + 1, 4, 21)]
    assert writes["Ga"][0][3] != 0
    # Gb: clamped and at rest up to the write; in batch 3 the clamp is on in the first fragments and off in the last,
    # the ramp still going
    assert all(clamp and not running for b, f, running, clamp, e in model["Gb"] if b < G_WRITE)
    b3 = [(running, clamp) for b, f, running, clamp, e in model["Gb"] if b == G_WRITE + 1]
    assert b3[0] == (True, True) and b3[-1] == (True, False)
    assert sorted(set(b3), reverse=True) == [(True, True), (True, False)] and b3 == sorted(b3, reverse=True)
    # Gc's is over with the last frame of batch 3, and batch 4 begins on the stale delta
    assert [(b, f) for b, f, running, clamp, e in model["Gc"] if running][-1] == (G_WRITE + 2, 0)
    # Gd: unsettled when batch 5 begins and only then
    assert writes["Gd"][0][4] < 256
    assert [b for b, f, running, clamp, e in model["Gd"] if f == 0 and running] == [G_LATE + 1]
    # every chain begins a batch without a record of its own unsettled: the kernel's ramp path
    for name in writes:
        assert any(running and f == 0 and b not in recs[name] for b, f, running, clamp, e in model[name]), name
    # the table is the host's bound applied to the script, and whoever begins a batch unsettled is within it
    for b in range(1, G_BATCHES):
        quiet = [n for n in writes if b not in recs[n]]
        assert G_FP[b - 1] == (1, 4, len(quiet), sum(bound_ramping(plan, writes[n], b) for n in quiet), 4 - len(quiet), 3), b
        for n in quiet:
            unsettled = next(running for bb, f, running, clamp, e in model[n] if (bb, f) == (b, 0))
            assert not unsettled or bound_ramping(plan, writes[n], b), (b, n)
    # ... and in the last two batches nobody is within a bound or unsettled
    assert all(not running for n in writes for b, f, running, clamp, e in model[n] if b >= G_BATCHES - 2)
    # heard: every batch from the writes on differs from the same scene left alone
    want = oracle_memo("g", g_script)
    flat = oracle_memo("g-flat", lambda be: g_script(be, ramps=False))
    for b in range(G_BATCHES):
        assert want[b].any()
        assert (first_diff(want[b], flat[b]) is not None) == (b >= G_WRITE), b


@pytest.mark.gpu
def test_gliding_chains_match_oracle(oracle_memo, monkeypatch):
    """The kernel's ramp path: a volume ramp that ends inside a fragment, a pan that comes back inside +-1 in the middle
    of a batch, a ramp that ends on a batch boundary (stale delta), a timer left set by a write behind the last window.
    Batches 6 and 7: at rest again by the end state the kernel stored, counted quiet, the audio still equal."""
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    want = oracle_memo("g", g_script)
    got, info, pinfo = on_gpu(g_script, use_async=True)
    for b in range(G_BATCHES):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {pinfo[b]} {info[b]}"
    for b in range(1, G_BATCHES):
        row = G_FP[b - 1]
        assert counts(pinfo[b], FP) == row, f"batch {b}: {pinfo[b]}"
        assert counts(info[b], BUS) == (1, 0, 0, 0, row[4]), f"batch {b}: {info[b]}"
        assert (info[b].consume, info[b].master_direct) == ((3, 1) if row[4] == 0 else (0, 0)), f"batch {b}: {info[b]}"


# ---------------------------------------------------------------------------
# 3. class edges
# ---------------------------------------------------------------------------
E_BATCHES, E_OUT, E_BACK, E_DIE = 8, 3, 5, 6
E_TAPS2 = [(4.2, 5.0, 6.3), (4.5, 5.5, 7.0)]
E_TAPS5 = [(3.0, 4.0, 5.0), (3.5, 4.5, 5.5), (4.0, 5.0, 6.0), (4.5, 5.5, 6.5), (5.0, 6.0, 7.0)]
E_RAW63, E_RAWFAR = 87381, 178870955            # register values of taps of 63 and of 131 072 - 63 frames at 48 kHz
# Bus owners: the root (a driver); E5 (five delays), E63, Efar (a tap one frame out of range at either end), Ex (the
# panmix not wired, an xinsert behind it): general by class, four of them; Eok (two delays) and Edie (one): the class.
# A tap of Eok is written to 43 frames in front of batch 3 - a record, and general by class from that batch on - and
# back to 384 in front of batch 5 - a record again, of the class again; Edie's units are deinitialised in front of
# batch 6, in which the dying voice is still listed, with its record.  Batches 1 .. 7:
E_FP = [(1, 2, 2, 0, 0, 2), (1, 2, 2, 0, 0, 2), (1, 1, 1, 0, 0, 1), (1, 1, 1, 0, 0, 1), (1, 2, 1, 0, 1, 2), (1, 2, 1, 0, 1, 2),
        (1, 1, 1, 0, 0, 2)]
E_GENERIC = [4, 4, 5, 5, 5, 5, 4]


def e_script(be, render=None, info=None):
    sc = synth.Scene(be, nwaves=4)
    sc.root()
    g = {"E5": pan_group(sc, E_TAPS5, 0.7, 0.2), "E63": pan_group(sc, E_TAPS2[:1], 0.7, -0.2),
         "Efar": pan_group(sc, E_TAPS2[:1], 0.9, 0.1)}
    be.unit_write(g["E63"]["units"][1], 0, E_RAW63)
    be.unit_write(g["Efar"]["units"][1], 2, E_RAWFAR)
    k = sc._key()
    ux = [be.unit_init(k, synth.K_INLINE, 0, 0, 2, 0), be.unit_init(k, synth.K_FBDELAY, 0, 2, 2, 0),
          be.unit_init(k, synth.K_PANMIX, 0, 2, 2, 0), be.unit_init(k, synth.K_XINSERT, synth.PROCADD, 2, 2, 1)]
    for reg, ms in enumerate(E_TAPS2[0]):
        be.unit_write(ux[1], reg, fix(ms))
    for reg, gain in enumerate(GAINS):
        be.unit_write(ux[1], 4 + reg, fix(gain))
    be.unit_write(ux[2], VOL, fix(0.8))
    g["Ex"] = dict(units=ux, leaves=[])
    sc.groups.append(g["Ex"])
    g["Eok"] = pan_group(sc, E_TAPS2, 0.75, 0.4)
    g["Edie"] = pan_group(sc, E_TAPS2[:1], 0.85, -0.5)
    for name in g:
        sc.add_voices(6, chain="osc-pan", group=g[name], total=48)

    def die():
        for units in g["Edie"]["leaves"]:
            for u in units:
                be.unit_deinit(u)
        for u in g["Edie"]["units"]:
            be.unit_deinit(u)
        sc.groups.remove(g["Edie"])
    before = {E_OUT: lambda: be.unit_write(g["Eok"]["units"][2], 1, fix(0.9)),
              E_BACK: lambda: be.unit_write(g["Eok"]["units"][2], 1, fix(8.0)),
              E_DIE: die}
    return run_script(be, sc, frag_plan(E_BATCHES, FRAGS, short=(2, 4)), before=before, render=render, info=info)


def r_script(be, render=None, info=None):
    """the shape as the root: inline 0 2; fbdelay 2 2; panmix+ 2 > 2 at depth 0, two bus groups under it"""
    sc = synth.Scene(be, nwaves=4)
    k = sc._key()
    sc.rootv = [be.unit_init(k, synth.K_INLINE, 0, 0, 2, 0), be.unit_init(k, synth.K_FBDELAY, 0, 2, 2, 0),
                be.unit_init(k, synth.K_PANMIX, synth.PROCADD, 2, 2, 1)]
    for reg, ms in enumerate(E_TAPS2[0]):
        be.unit_write(sc.rootv[1], reg, fix(ms))
    for reg, gain in enumerate(GAINS):
        be.unit_write(sc.rootv[1], 4 + reg, fix(gain))
    be.unit_write(sc.rootv[2], VOL, fix(0.8))
    for _ in range(2):
        sc.add_voices(6, chain="osc-pan", group=sc.add_bus_group(), total=16)
    return run_script(be, sc, frag_plan(4, FRAGS, short=(2, 4)), render=render, info=info)


def test_edges_script_does_what_it_is_built_for(oracle_memo):
    assert E_RAW63 * 48000 // 65536000 == 63 and E_RAWFAR * 48000 // 65536000 == BUFSIZE - 63
    assert tap_frames(0.9) == 43 and tap_frames(8.0) == 384 and len(E_TAPS5) == 5
    assert rounds(E_TAPS2) == 3 and rounds(E_TAPS5) >= 1
    for b in range(1, E_BATCHES):
        out = E_OUT <= b < E_BACK
        recs = (b == E_BACK) + (b == E_DIE)
        cls = 2 - out - (b > E_DIE)
        assert E_FP[b - 1][:5] == (1, cls, cls - recs, 0, recs), b
        assert E_GENERIC[b - 1] == 4 + out + recs, b
    assert all(w.any() for w in oracle_memo("e", e_script))
    assert all(w.any() for w in oracle_memo("r", r_script))


@pytest.mark.gpu
def test_class_edges_match_oracle(oracle_memo, monkeypatch):
    """Five delays, a tap of 63 frames, a tap of 131 072 - 63, a panmix that is not wired: the general kernel's by class.
    A tap written below a fragment and back moves a chain out of the class and back; a chain that is deinitialised leaves
    it."""
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    want = oracle_memo("e", e_script)
    got, info, pinfo = on_gpu(e_script)
    for b in range(E_BATCHES):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {pinfo[b]} {info[b]}"
    for b in range(1, E_BATCHES):
        assert counts(pinfo[b], FP) == E_FP[b - 1], f"batch {b}: {pinfo[b]}"
        assert counts(info[b], BUS) == (1, 0, 0, 0, E_GENERIC[b - 1]), f"batch {b}: {info[b]}"
        assert info[b].consume == 0


@pytest.mark.gpu
def test_a_root_of_the_shape_stays_general(oracle_memo, monkeypatch):
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    want = oracle_memo("r", r_script)
    got, info, pinfo = on_gpu(r_script)
    for b in range(len(want)):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {pinfo[b]} {info[b]}"
        assert counts(pinfo[b], FP) == (0, 0, 0, 0, 0, 0), f"batch {b}: {pinfo[b]}"
    for b in range(1, len(want)):
        assert counts(info[b], BUS) == (2, 0, 0, 0, 1), f"batch {b}: {info[b]}"


# ---------------------------------------------------------------------------
# 5. a song
# ---------------------------------------------------------------------------
SONG = "k2intro"
SONG_FRAGS = 10 * 64            # the window: the first N x 64 fragments, N = 10
SONG_BATCH = 16                 # (see the module's docstring: at 64 the trace has fewer than 8 record-free batches in 71)
K_PANMIX, K_FBDELAY, K_INLINE = synth.K_PANMIX, synth.K_FBDELAY, synth.K_INLINE


def song_master(tr):
    """the master voice from the T_INIT records alone: (voice, its unit ids) of the chain inline; fbdelay ...; panmix"""
    chains = {}
    for r in tr.records:
        if r[0] == T_INIT:
            chains.setdefault(r[2], []).append((r[1], r[3]))
    found = [(v, [u for u, _k in us]) for v, us in chains.items()
             if len(us) >= 3 and us[0][1] == K_INLINE and us[-1][1] == K_PANMIX and all(k == K_FBDELAY for _u, k in us[1:-1])]
    assert len(found) == 1, found
    return found[0]


def song_record_free(tr, units, batch, max_fragments):
    """per rendered batch of replay(tr, batch=batch, max_fragments=...): True where the master carries no record - no
    write, init or deinit to its units and every Process of them (0, the fragment's frames)"""
    units = set(units)
    out, free, pending, nfrag, frames = [], True, 0, 0, 0
    for r in tr.records:
        op = r[0]
        if op == T_FRAGMENT:
            if nfrag >= max_fragments:
                break
            if pending and nfrag % batch == 0:
                out.append(free)
                free, pending = True, 0
            frames = r[1]
            pending += frames
            nfrag += 1
        elif op == T_WAVEDROP:
            if pending:
                out.append(free)
                free, pending = True, 0
        elif op in (T_INIT, T_DEINIT, T_WRITE) and r[1] in units:
            free = False
        elif op == T_PROCESS and r[1] in units and (r[2], r[3]) != (0, frames):
            free = False
    if pending:
        out.append(free)
    return out


@pytest.fixture(scope="module")
def song():
    return Trace(os.path.join(GOLDEN, f"{SONG}.trace.xz"))


def test_song_premise(song):
    voice, units = song_master(song)
    assert [song.kinds[u] for u in units] == [K_INLINE, K_FBDELAY, K_PANMIX]
    free = song_record_free(song, units, SONG_BATCH, SONG_FRAGS)
    assert len(free) == SONG_FRAGS // SONG_BATCH
    assert sum(free) >= 8 and free.count(False) >= 1 and not free[0]
    # at 64 fragments a batch - the buffer the issue asked for - the whole trace has fewer than 8 such batches,
    # whatever the window: the cut window every 61 fragments
    whole = song_record_free(song, units, 64, 10 ** 9)
    assert len(whole) == 71 and sum(whole) < 8
    assert not any(song_record_free(song, units, 64, SONG_FRAGS))


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [SONG_BATCH, 64])
def test_song_master_reaches_the_kernel(song, monkeypatch, batch):
    """k2intro's first 640 fragments: the master is the kernel's in every batch the trace leaves it without a record and
    the general kernel's in the others - at 64 fragments a batch that is all of them - and the audio is the reference's."""
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    _voice, units = song_master(song)
    free = song_record_free(song, units, batch, SONG_FRAGS)
    cfg = song.config
    be = make_gpu(cfg["samplerate"], cfg["basepitch"], cfg["channels"], max_batch=batch)
    pinfo = []
    be.render = spy(be, pinfo, be.render)
    out = replay(song, be, batch=batch, check_noise=True, max_fragments=SONG_FRAGS)
    be.close()
    got = fnv1a_fragments(out)
    want = np.load(os.path.join(GOLDEN, f"{SONG}.hash.npy"))[:SONG_FRAGS]
    assert len(got) == SONG_FRAGS
    bad = np.nonzero(got != want)[0]
    assert not bad.size, bad[:4]
    assert len(pinfo) == len(free)
    for b, (f, i) in enumerate(zip(free, pinfo)):
        assert i.class_voices == 1 and i.max_delays == 1, f"batch {b}: {i}"
        if f:
            assert i.quiet_voices + i.gliding_voices == 1 and i.record_voices == 0 and i.launched == 1, f"batch {b}: {i}"
        else:
            assert i.record_voices == 1 and i.quiet_voices == 0, f"batch {b}: {i}"
