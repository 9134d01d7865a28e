"""Delay-chain bus owners whose only records are cut windows keep their fast kernels (include/a2amd_buswin.h): a wired
chain has the windows dropped and stays k_bus_fbdchain's, a pan-tailed chain takes its run to k_bus_fbdpan's windows
launch, which steps volume and pan window by window.  Against the oracle, with the proof of who rendered what
(a2amd_last_batch_bus_windows, a2amd_last_batch_fbdpan, a2amd_last_batch_buses).

A cut group is walked as the engine walks a voice whose VM (or whose parent's) woke inside a fragment: the whole
group - inline, everything below it, the chain behind it - once per window (test_gpu_bus_paths.py: b_script).  The
cuts are [0, 20) [20, 47) [47, 64) in every third fragment of every batch and [0, 20) [20, 37) in the short fragment.
Every GPU test renders one script on the oracle and on the GPU, compares the audio batch by batch and asserts, batch
by batch, who rendered the bus owners.  The expected counts are tables written down from the script by the frame
arithmetic at each table; none is a recording of what the library said.  Batches are 10 fragments, one of them 37
frames; six osc-pan leaves in every group (the cap test: 256 fragments, two leaves).

The tests without the gpu mark check the interface, on the oracle alone that each script does what it is built for
(the rampers restated in test_gpu_bus_paths.py, here with a window as the unit instead of a fragment), and from the
traces alone what a song's master section gets at a player's 64-fragment buffer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from audiality2_amd import synth
from audiality2_amd.replay import (T_DEINIT, T_FRAGMENT, T_INIT, T_PROCESS, T_WAVEDROP, T_WRITE, Trace, a2amd_bus_info,
                                   a2amd_bus_windows_info, a2amd_fbdpan_batch_info, replay)
from conftest import GOLDEN, ROOT, fnv1a_fragments, make_gpu, make_oracle
from test_fbd_pan import pan_group, rounds, song_master, spy
from test_gpu_bus_paths import bound_ramping, driver_model, first_diff, frag_plan, render_async, run_script

fix = synth.fix
PAN, VOL = 1, 0
FRAGS = 10
GAINS = (0.4, 0.3, 0.35)
BUS = ("driver_voices", "driver_ramping", "driver_windows_dropped", "fbd_voices", "generic_voices")
FP = ("launched", "class_voices", "quiet_voices", "gliding_voices", "record_voices", "max_delays")
BW = ("fbd_dropped", "fbdpan_voices", "fbdpan_gliding", "fbdpan_windows", "refused_tiling", "refused_cap", "window_cap",
      "launched")
CAP = 512       # FBW_MAXWIN = 2 * A2D_MAXBATCH (a2amd_device.h)
TAPS1 = [(2.1, 3.0, 4.0)]                                   # 100 frames: rounds of 1 fragment
TAPS3 = [(4.2, 5.0, 6.3), (4.5, 5.5, 7.0)]                  # 201 frames: of 3
TAPSB = [(63.1, 75.6, 100.4), (70.0, 81.0, 90.5)]           # 3 028 frames: the whole batch


def counts(bi, names):
    return tuple(int(getattr(bi, n)) for n in names)


def cuts(f, n):
    """the windows (first frame, frames) of fragment f of a batch, n frames long"""
    if n == 37:
        return [(0, 20), (20, 17)]
    return [(0, 20), (20, 27), (47, 17)] if f % 3 == 0 else [(0, n)]


def gaps(f, n):
    """... with the middle window left out: [0, 20) and [47, 64) do not tile the fragment"""
    return [(0, 20), (47, 17)] if f % 3 == 0 and n == 64 else [(0, n)]


def halves(f, n):
    return [(0, 31), (31, n - 31)]


def cut_walk(sc, cut, windows=cuts):
    """Scene.walk as a run_script walk, with the groups of `cut` (under the root) walked once per window of windows(f, n) -
    and with them everything they hold: a group inside a cut group is walked inside each of its windows, cut the same
    way.  cut: a list of groups, or {id(group): its own windows function}"""
    if not isinstance(cut, dict):
        cut = {id(g): windows for g in cut}
    be = sc.be

    def group(g, a, m):
        be.unit_process(g["units"][0], a, m)
        for sub in g.get("subs", ()):
            group(sub, a, m)
        for units in g["leaves"]:
            for u in units:
                be.unit_process(u, a, m)
        be.inline_end(g["units"][0])
        for u in g["units"][1:]:
            be.unit_process(u, a, m)

    def walk(b, f, n):
        be.fragment(n)
        be.unit_process(sc.rootv[0], 0, n)
        for g in sc.groups:
            for a, m in (cut[id(g)](f, n) if id(g) in cut else [(0, n)]):
                group(g, a, m)
        for units in sc.leaves:
            for u in units:
                be.unit_process(u, 0, n)
        be.inline_end(sc.rootv[0])
        be.unit_process(sc.rootv[1], 0, n)
        be.unit_process(sc.rootv[2], 0, n)
    return walk


def rows(plan, b, windows=cuts):
    """table rows one voice needs in batch b: over its fragments, max(1, windows in the fragment)"""
    return sum(len(windows(f, n)) for f, n in enumerate(plan[b]))


def window_plan(plan, windows=cuts):
    """(the frames of every WINDOW, batch by batch - frag_plan's shape, for driver_model and bound_ramping, which then
    step the rampers window by window as panmix_process22 does; per batch the (fragment, first frame) of each window)"""
    wp = [[m for f, n in enumerate(frags) for _a, m in windows(f, n)] for frags in plan]
    where = [[(f, a) for f, n in enumerate(frags) for a, _m in windows(f, n)] for frags in plan]
    return wp, where


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


def on_gpu(script, max_batch=FRAGS, use_async=True):
    """the script on the GPU: (audio, then per batch a2amd_bus_info, a2amd_fbdpan_batch_info, a2amd_bus_windows_info)"""
    gpu = make_gpu(max_batch=max_batch)
    info, pinfo, winfo = [], [], []
    inner = spy(gpu, pinfo, (lambda frames: render_async(gpu, frames)) if use_async else None)

    def render(frames):
        out = inner(frames)
        winfo.append(gpu.last_batch_bus_windows())
        return out
    got = script(gpu, info=info, render=render)
    gpu.close()
    return got, info, pinfo, winfo


# ---------------------------------------------------------------------------
# the interface
# ---------------------------------------------------------------------------
def test_abi(gpu_lib):
    text = open(os.path.join(ROOT, "include", "a2amd_buswin.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(a2amd_[a-z_0-9]+)\s*\(", text))) == ["a2amd_last_batch_bus_windows"]
    assert '#include "a2amd_buswin.h"' in open(os.path.join(ROOT, "include", "a2amd.h")).read()
    assert hasattr(gpu_lib, "a2amd_last_batch_bus_windows")     # (gpu_lib: liba2amd.so loaded, no device needed)
    assert C.sizeof(a2amd_bus_windows_info) == 32
    assert [n for n, _ in a2amd_bus_windows_info._fields_] == list(BW)
    assert all(t is C.c_uint32 for _n, t in a2amd_bus_windows_info._fields_)
    fields = re.findall(r"uint32_t\s+(\w+);", text[text.index("typedef struct a2amd_bus_windows_info"):])
    assert fields == list(BW)
    # the structs beside it keep their layout
    assert C.sizeof(a2amd_bus_info) == 28 and C.sizeof(a2amd_fbdpan_batch_info) == 32
    # NULL arguments are refused, not dereferenced
    gpu_lib.a2amd_last_batch_bus_windows.restype = C.c_int
    gpu_lib.a2amd_last_batch_bus_windows.argtypes = [C.c_void_p, C.c_void_p]
    assert gpu_lib.a2amd_last_batch_bus_windows(None, None) != 0
    out = a2amd_bus_windows_info()
    assert gpu_lib.a2amd_last_batch_bus_windows(None, C.byref(out)) != 0


# ---------------------------------------------------------------------------
# 1. at rest (and 3: its switches, the gap, the nested chains)
# ---------------------------------------------------------------------------
R_BATCHES = 5
R_GAINS = (0.8, 0.5)        # P's volume and pan, written with the births: within the host's bound until frame 256


def r_plan():
    return frag_plan(R_BATCHES, FRAGS, short=(2, 4))


def r_script(be, windows=cuts, nested=False, render=None, info=None):
    """The root; P, a pan-tailed chain of one delay, and W, a wired chain of two, under it, both cut.  nested: Q (pan-
    tailed, two delays) and V (wired, one delay) inside P - depth 2, cut with it."""
    sc = synth.Scene(be, nwaves=4)
    sc.root()
    g = {"P": pan_group(sc, TAPS1, *R_GAINS), "W": sc.add_group(fb=TAPS3, gains=GAINS, delays=2)}
    if nested:
        g["Q"] = pan_group(sc, TAPS3, 0.9, -0.4, parent=g["P"])
        g["V"] = sc.add_group(fb=TAPS1, gains=GAINS, delays=1, parent=g["P"])
    for name in g:
        sc.add_voices(6, chain="osc-pan", group=g[name], total=32)
    assert not sc.leaves
    return run_script(be, sc, r_plan(), walk=cut_walk(sc, [g["P"], g["W"]], windows) if windows else None,
                      render=render, info=info)


# Batches 1 .. 4 (batch 0 carries the births: every owner has other records than windows, nobody is dropped or windowed).
# Fragments 0, 3, 6 and 9 are cut in three: 10 + 4 x 2 = 18 rows; batch 2 has the short fragment, cut in two: 19.
#   (fbd_dropped, fbdpan_voices, fbdpan_gliding, fbdpan_windows, refused_tiling, refused_cap, window_cap, launched)
R_BW = [(1, 1, 0, 18, 0, 0, CAP, 1), (1, 1, 0, 19, 0, 0, CAP, 1), (1, 1, 0, 18, 0, 0, CAP, 1), (1, 1, 0, 18, 0, 0, CAP, 1)]
R_BUS = (1, 0, 0, 1, 0)         # the root on k_bus_driver, W on k_bus_fbdchain, nobody the general kernel's
R_FP = (1, 1, 0, 0, 1, 1)       # P has a run (record_voices' arithmetic is unchanged) and the windows launch ran


def test_rest_script_does_what_it_is_built_for(oracle_memo):
    """(i) At rest the cut render is the whole-fragment render in every batch: why the runs may be ignored or dropped.
    (iii) The rounds are what the scripts say."""
    assert [rounds(t) for t in (TAPS1, TAPS3)] == [1, 3] and rounds(TAPSB) >= FRAGS
    plan = r_plan()
    assert [rows(plan, b) for b in range(1, R_BATCHES)] == [row[3] for row in R_BW]
    assert [n for frags in plan for n in frags].count(37) == 1 and plan[2][4] == 37 and 4 % 3 != 0
    ws = [(0, VOL, fix(R_GAINS[0]), 0, 0), (0, PAN, fix(R_GAINS[1]), 0, 0)]
    assert not any(bound_ramping(plan, ws, b) for b in range(1, R_BATCHES))
    for nested in (False, True):
        cut = oracle_memo(("r", nested), lambda be: r_script(be, nested=nested))
        whole = oracle_memo(("r-whole", nested), lambda be: r_script(be, windows=None, nested=nested))
        for b in range(R_BATCHES):
            assert cut[b].any()
            assert first_diff(cut[b], whole[b]) is None, (nested, b)
    # the gap is heard: 27 frames of every third fragment are not rendered
    gap = oracle_memo("r-gap", lambda be: r_script(be, windows=gaps))
    cut = oracle_memo(("r", False), lambda be: r_script(be))
    assert all(first_diff(gap[b], cut[b]) is not None for b in range(R_BATCHES))


@pytest.mark.gpu
def test_chains_at_rest_keep_their_kernels_through_cut_windows(oracle_memo, monkeypatch):
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    monkeypatch.delenv("A2AMD_BUS_WINDOWS", raising=False)
    want = oracle_memo(("r", False), lambda be: r_script(be))
    got, info, pinfo, winfo = on_gpu(r_script)
    for b in range(R_BATCHES):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {winfo[b]} {pinfo[b]} {info[b]}"
    assert counts(winfo[0], BW) == (0, 0, 0, 0, 0, 0, CAP, 0)
    for b in range(1, R_BATCHES):
        assert counts(winfo[b], BW) == R_BW[b - 1], f"batch {b}: {winfo[b]}"
        assert counts(info[b], BUS) == R_BUS, f"batch {b}: {info[b]}"
        assert (info[b].consume, info[b].master_direct) == (3, 1), f"batch {b}: {info[b]}"
        assert counts(pinfo[b], FP) == R_FP, f"batch {b}: {pinfo[b]}"


@pytest.mark.gpu
def test_windows_that_leave_a_gap_are_refused(oracle_memo, monkeypatch):
    """[0, 20) and [47, 64) only, on the pan-tailed and on the wired chain: windows only, but no tiling - both are the
    general kernel's, which renders the windows it is given."""
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    monkeypatch.delenv("A2AMD_BUS_WINDOWS", raising=False)
    want = oracle_memo("r-gap", lambda be: r_script(be, windows=gaps))
    got, info, pinfo, winfo = on_gpu(lambda be, **kw: r_script(be, windows=gaps, **kw))
    for b in range(R_BATCHES):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {winfo[b]} {pinfo[b]} {info[b]}"
    for b in range(1, R_BATCHES):
        assert counts(winfo[b], BW) == (0, 0, 0, 0, 2, 0, CAP, 0), f"batch {b}: {winfo[b]}"
        assert counts(info[b], BUS) == (1, 0, 0, 0, 2), f"batch {b}: {info[b]}"
        assert counts(pinfo[b], FP) == (1, 1, 0, 0, 1, 1), f"batch {b}: {pinfo[b]}"       # (launched: it skipped P)
        assert info[b].consume == 0


@pytest.mark.gpu
def test_a_class_switched_off_is_neither_dropped_nor_windowed(oracle_memo, monkeypatch):
    """A2AMD_NO_FAST=512: P is a general bus owner by class, W still has its windows dropped.  =32: the other way round."""
    monkeypatch.delenv("A2AMD_BUS_WINDOWS", raising=False)
    want = oracle_memo(("r", False), lambda be: r_script(be))
    monkeypatch.setenv("A2AMD_NO_FAST", "512")
    got, info, pinfo, winfo = on_gpu(r_script)
    for b in range(R_BATCHES):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {winfo[b]} {info[b]}"
    for b in range(1, R_BATCHES):
        assert counts(winfo[b], BW) == (1, 0, 0, 0, 0, 0, CAP, 0), f"batch {b}: {winfo[b]}"
        assert counts(info[b], BUS) == (1, 0, 0, 1, 1), f"batch {b}: {info[b]}"
        assert counts(pinfo[b], FP) == (0, 0, 0, 0, 0, 0), f"batch {b}: {pinfo[b]}"
    monkeypatch.setenv("A2AMD_NO_FAST", "32")
    got, info, pinfo, winfo = on_gpu(r_script)
    for b in range(R_BATCHES):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {winfo[b]} {info[b]}"
    for b in range(1, R_BATCHES):
        assert counts(winfo[b], BW) == (0, 1, 0, R_BW[b - 1][3], 0, 0, CAP, 1), f"batch {b}: {winfo[b]}"
        assert counts(info[b], BUS) == (1, 0, 0, 0, 1), f"batch {b}: {info[b]}"
        assert counts(pinfo[b], FP) == R_FP, f"batch {b}: {pinfo[b]}"


@pytest.mark.gpu
def test_bus_windows_switch_is_the_general_kernel_and_sounds_the_same(oracle_memo, monkeypatch):
    """A2AMD_BUS_WINDOWS set: every bus owner with records is the general kernel's, as before the routing existed."""
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    want = oracle_memo(("r", False), lambda be: r_script(be))
    monkeypatch.setenv("A2AMD_BUS_WINDOWS", "1")
    got, info, pinfo, winfo = on_gpu(r_script)
    for b in range(R_BATCHES):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {winfo[b]} {info[b]}"
        assert counts(winfo[b], BW) == (0, 0, 0, 0, 0, 0, CAP, 0), f"batch {b}: {winfo[b]}"
    for b in range(1, R_BATCHES):
        assert counts(info[b], BUS) == (1, 0, 0, 0, 2), f"batch {b}: {info[b]}"
        assert counts(pinfo[b], FP) == (1, 1, 0, 0, 1, 1), f"batch {b}: {pinfo[b]}"       # (launched: it skipped P)
        assert (info[b].consume, info[b].master_direct) == (0, 0)


@pytest.mark.gpu
def test_chains_at_depth_two_under_a_cut_pan_tailed_chain(oracle_memo, monkeypatch):
    """Q (pan-tailed) and V (wired) inside P, all cut with P: the windows launches of depth 2 and 1 in that order."""
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    monkeypatch.delenv("A2AMD_BUS_WINDOWS", raising=False)
    want = oracle_memo(("r", True), lambda be: r_script(be, nested=True))
    got, info, pinfo, winfo = on_gpu(lambda be, **kw: r_script(be, nested=True, **kw))
    for b in range(R_BATCHES):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {winfo[b]} {pinfo[b]} {info[b]}"
    for b in range(1, R_BATCHES):
        # W and V dropped; P and Q windowed, each with the batch's rows
        assert counts(winfo[b], BW) == (2, 2, 0, 2 * R_BW[b - 1][3], 0, 0, CAP, 1), f"batch {b}: {winfo[b]}"
        assert counts(info[b], BUS) == (1, 0, 0, 2, 0), f"batch {b}: {info[b]}"
        assert counts(pinfo[b], FP) == (1, 2, 0, 0, 2, 2), f"batch {b}: {pinfo[b]}"
        assert (info[b].consume, info[b].master_direct) == (3, 1), f"batch {b}: {info[b]}"


# ---------------------------------------------------------------------------
# 2. gliding
# ---------------------------------------------------------------------------
G_BATCHES, G_WRITE = 8, 2
G_TAPS = {"Ha": TAPS1, "Hb": TAPS3, "Hc": TAPSB}        # rounds of 1 and of 3 fragments, the whole batch
# Frames from the beginning of batch 2, in front of which the ramps are written.  Batch 2 is 640 frames; batch 3 has the
# short fragment (3, 4): its fragments begin at 0, 64, 128, 192, 256, 293, 357, 421, 485, 549 and it is 613 frames.
#   Ha (a): the volume ramp ends in batch 4, fragment 3 (cut), frame 30 - 10 frames into the middle window [20, 47):
#           640 + 613 + 3 x 64 + 30 = 1475
#   Hb (b): the pan, at rest at 1.4, goes to 0.6: inside +-1 after half of the ramp.  Half = 640 + 3 x 64 + 5 = 837,
#           5 frames into the first window of batch 3's fragment 3 (cut): the clamp is on for [0, 20) and off for
#           [20, 47).  The whole = 1674 = 640 + 613 + 6 x 64 + 37: over in batch 4, fragment 6 (cut), inside [20, 47)
#   Hc (c): the volume ramp ends with frame 20 of batch 3's fragment 6 (cut, begins at 357), the boundary between
#           [0, 20) and [20, 47): 640 + 357 + 20 = 1017.  The window [20, 47) begins with timer 0 and the stale delta
G_LEN = {"Ha": 1475, "Hb": 1674, "Hc": 1017}
G_DIFF = {"Ha": 4, "Hb": 4, "Hc": 3}    # the batch in which the cut render must differ from the whole-fragment one


def g_plan():
    return frag_plan(G_BATCHES, FRAGS, short=(3, 4))


def g_writes():
    """group -> its panmix writes (batch, reg, value, start, dur), made in front of the batch"""
    return {
        "Ha": [(G_WRITE, VOL, fix(0.3), 33, (G_LEN["Ha"] << 8) + 77)],
        "Hb": [(0, PAN, fix(1.4), 0, 0), (G_WRITE, PAN, fix(0.6), 0, G_LEN["Hb"] << 8)],
        "Hc": [(G_WRITE, VOL, fix(0.35), 0, G_LEN["Hc"] << 8)],
    }


# Batches 1 .. 7.  All three chains are cut in every batch; batch 2 carries the three writes: general.  With t the frame
# at which batch 2 begins, the host's bound is the ramp's length + 256 (a2amd_bus.h):
#       Ha 1475 + 256 = 1731    Hb 1674 + 256 = 1930    Hc 1017 + 256 = 1273    batches 3 .. 6 begin at t + 640, 1253, 1893, 2533
#   3: all three (640).  4: all three (1253 < 1273).  5: Hb (1893 < 1930).  6, 7: nobody - at rest by the end state the
#   kernel stored.  Rows a voice: 18, in batch 3 (the short fragment) 19.
#   (fbd_dropped, fbdpan_voices, fbdpan_gliding, fbdpan_windows, refused_tiling, refused_cap, window_cap, launched)
G_BW = [(0, 3, 0, 54, 0, 0, CAP, 1), (0, 0, 0, 0, 0, 0, CAP, 0), (0, 3, 3, 57, 0, 0, CAP, 1), (0, 3, 3, 54, 0, 0, CAP, 1),
        (0, 3, 1, 54, 0, 0, CAP, 1), (0, 3, 0, 54, 0, 0, CAP, 1), (0, 3, 0, 54, 0, 0, CAP, 1)]


def g_script(be, only=None, windows=cuts, render=None, info=None):
    """only: the one chain whose ramp is written (the others stay at rest; Hb's pan stays at 1.4)"""
    sc = synth.Scene(be, nwaves=4)
    sc.root()
    g = {name: pan_group(sc, taps) for name, taps in G_TAPS.items()}
    for name in g:
        sc.add_voices(6, chain="osc-pan", group=g[name], total=32)
    before = {}
    for name, ws in g_writes().items():
        for b, reg, value, start, dur in ws:
            if b == 0 or only in (None, name):
                before.setdefault(b, []).append((g[name]["units"][-1], reg, value, start, dur))
    return run_script(be, sc, g_plan(), walk=cut_walk(sc, list(g.values()), windows) if windows else None, render=render,
                      info=info, before={b: (lambda ws=ws: [be.unit_write(*w) for w in ws]) for b, ws in before.items()})


def test_gliding_script_does_what_it_is_built_for(oracle_memo):
    plan, writes = g_plan(), g_writes()
    wplan, where = window_plan(plan)
    assert [sum(b) for b in wplan] == [sum(b) for b in plan]
    start3 = [sum(plan[3][:f]) for f in range(FRAGS)]
    assert start3[6] == 357 and sum(plan[3]) == 613 and sum(plan[2]) == 640
    assert G_LEN == {"Ha": 640 + 613 + 3 * 64 + 30, "Hb": 2 * (640 + 3 * 64 + 5), "Hc": 640 + 357 + 20}
    assert G_LEN["Hb"] == 640 + 613 + 6 * 64 + 37
    # (the model's windows are the windows: a row per window, as k_bus_fbdpan's thread 0 steps them)
    model = {name: driver_model(wplan, ws) for name, ws in writes.items()}
    # (a) over 10 frames into the middle window of batch 4's fragment 3
    ends = [(b, where[b][w], e) for b, w, running, clamp, e in model["Ha"] if e is not None]
    assert ends == [(G_WRITE + 2, (3, 20), 10)]
    # (b) clamped and at rest up to the write; in batch 3 the clamp is on in the first windows and off in the last, and
    # goes off between the first and the second window of fragment 3; the ramp ends inside the middle window of batch 4's
    # fragment 6 (the pan's own end: the model reports the volume's, so Hb's pan is run as a volume)
    assert all(clamp and not running for b, w, running, clamp, e in model["Hb"] if b < G_WRITE)
    b3 = [(where[3][w], running, clamp) for b, w, running, clamp, e in model["Hb"] if b == G_WRITE + 1]
    assert all(running for _at, running, _c in b3)
    assert [c for (f, _a), _r, c in b3 if f == 3] == [True, False, False]
    assert [c for _at, _r, c in b3] == sorted((c for _at, _r, c in b3), reverse=True)
    as_vol = driver_model(wplan, [(G_WRITE, VOL, fix(0.6), 0, G_LEN["Hb"] << 8)])
    assert [(b, where[b][w], e) for b, w, running, clamp, e in as_vol if e is not None] == [(G_WRITE + 2, (6, 20), 17)]
    # (c) no window is longer than what is left of the ramp - it ends with the last frame of [0, 20) of batch 3's
    # fragment 6 - and the window behind it begins unsettled (the stale delta), the one behind that at rest
    assert not any(e is not None for b, w, running, clamp, e in model["Hc"])
    assert [(b, where[b][w]) for b, w, running, clamp, e in model["Hc"] if running][-1] == (G_WRITE + 1, (6, 20))
    # the table is the host's bound applied to the script; whoever begins a batch unsettled is within it
    recs = {name: {w[0] for w in ws if w[0] > 0} for name, ws in writes.items()}
    for b in range(1, G_BATCHES):
        mine = [n for n in writes if b not in recs[n]]
        assert G_BW[b - 1] == (0, len(mine), sum(bound_ramping(plan, writes[n], b) for n in mine), len(mine) * rows(plan, b),
                               0, 0, CAP, int(bool(mine))), b
        for n in mine:
            unsettled = next(running for bb, w, running, clamp, e in model[n] if (bb, w) == (b, 0))
            assert not unsettled or bound_ramping(plan, writes[n], b), (b, n)
    # every chain begins a batch without a write unsettled: the windows launch's ramp path
    for n in writes:
        assert any(running and w == 0 and b not in recs[n] for b, w, running, clamp, e in model[n]), n
    # ... and in the last two batches nobody is within a bound or unsettled
    assert all(not running for n in writes for b, w, running, clamp, e in model[n] if b >= G_BATCHES - 2)
    assert G_BW[-2][2] == G_BW[-1][2] == 0
    # (ii) heard: with its ramp's end inside a cut fragment - not on its last frame - each chain's cut render differs from
    # its whole-fragment render in that batch: a window that is longer than what is left of the ramp stretches the rest
    # over its own length (a2_PrepareRamper's last branch), 27 or 17 frames where the whole fragment takes 64.  A kernel
    # that ignored the windows would render the whole-fragment audio.  (Elsewhere the windows move a delta by an LSB at
    # the most: not asserted either way.)
    for n in writes:
        cut = oracle_memo(("g", n), lambda be: g_script(be, only=n))
        whole = oracle_memo(("g-whole", n), lambda be: g_script(be, only=n, windows=None))
        assert first_diff(cut[G_DIFF[n]], whole[G_DIFF[n]]) is not None, n
        for b in range(G_WRITE):        # (at rest: no difference)
            assert first_diff(cut[b], whole[b]) is None, (n, b)
    assert all(w.any() for w in oracle_memo("g", g_script))


@pytest.mark.gpu
def test_gliding_chains_through_cut_windows_match_oracle(oracle_memo, monkeypatch):
    """The windows launch's ramp path: a volume ramp that ends inside a middle window, a pan that comes back inside +-1
    between two windows of a fragment, a ramp that ends on a window boundary (stale delta, timer 0).  Batches 6 and 7: at
    rest again by the end state the kernel stored - the runs are ignored - the audio still equal."""
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    monkeypatch.delenv("A2AMD_BUS_WINDOWS", raising=False)
    want = oracle_memo("g", g_script)
    got, info, pinfo, winfo = on_gpu(g_script)
    for b in range(G_BATCHES):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {winfo[b]} {pinfo[b]} {info[b]}"
    for b in range(1, G_BATCHES):
        row = G_BW[b - 1]
        general = 3 - row[1]
        assert counts(winfo[b], BW) == row, f"batch {b}: {winfo[b]}"
        assert counts(info[b], BUS) == (1, 0, 0, 0, general), f"batch {b}: {info[b]}"
        assert counts(pinfo[b], FP) == (1, 3, 0, 0, 3, 2), f"batch {b}: {pinfo[b]}"
        assert (info[b].consume, info[b].master_direct) == ((3, 1) if not general else (0, 0)), f"batch {b}: {info[b]}"


# ---------------------------------------------------------------------------
# 4. the cap
# ---------------------------------------------------------------------------
C_BATCHES, C_FRAGS = 3, 256
# Written with the births, in front of batch 0: longer than the three batches, so batches 1 and 2 begin within the bound
C_RAMP = (0, VOL, fix(0.25), 0, (4 * C_FRAGS * 64) << 8)


def thirds(f, n):
    return [(0, 20), (20, 27), (47, n - 47)]


def c_script(be, render=None, info=None):
    """C2, cut in two in every fragment: 2 x 256 = 512 rows, the cap - taken.  C3, cut in three: 768 - refused."""
    sc = synth.Scene(be, nwaves=4)
    sc.root()
    c2, c3 = pan_group(sc, TAPS1), pan_group(sc, TAPS3)
    for g in (c2, c3):
        sc.add_voices(2, chain="osc-pan", group=g, total=8)
        be.unit_write(g["units"][-1], *C_RAMP[1:])
    return run_script(be, sc, frag_plan(C_BATCHES, C_FRAGS), walk=cut_walk(sc, {id(c2): halves, id(c3): thirds}),
                      render=render, info=info)


def test_cap_script_does_what_it_is_built_for(oracle_memo):
    plan = frag_plan(C_BATCHES, C_FRAGS)
    assert rows(plan, 1, halves) == CAP == 2 * C_FRAGS and rows(plan, 1, thirds) == 768 > CAP
    assert all(bound_ramping(plan, [C_RAMP], b) for b in (1, 2))
    model = driver_model(window_plan(plan, halves)[0], [C_RAMP])
    assert all(running for b, w, running, clamp, e in model if b > 0 or w > 0)
    assert all(w.any() for w in oracle_memo("c", c_script))


@pytest.mark.gpu
def test_a_run_at_the_cap_is_taken_and_one_beyond_it_refused(oracle_memo, monkeypatch):
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    monkeypatch.delenv("A2AMD_BUS_WINDOWS", raising=False)
    want = oracle_memo("c", c_script)
    got, info, pinfo, winfo = on_gpu(c_script, max_batch=C_FRAGS, use_async=False)
    for b in range(C_BATCHES):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {winfo[b]} {pinfo[b]} {info[b]}"
    for b in (1, 2):
        assert counts(winfo[b], BW) == (0, 1, 1, CAP, 0, 1, CAP, 1), f"batch {b}: {winfo[b]}"
        assert counts(info[b], BUS) == (1, 0, 0, 0, 1), f"batch {b}: {info[b]}"
        assert counts(pinfo[b], FP) == (1, 2, 0, 0, 2, 2), f"batch {b}: {pinfo[b]}"


# ---------------------------------------------------------------------------
# 5. the songs
# ---------------------------------------------------------------------------
SONG_FRAGS, SONG_BATCH = 10 * 64, 64
# at 64 fragments a batch, the master's batches: (delays, batches, no record, windows only, a write / init)
SONGS = {"k2intro": (1, 71, 2, 68, 1), "fmtest3": (2, 59, 1, 57, 1)}
NONE, WINDOWS, WRITES = 0, 1, 2


def song_master_batches(tr, units, batch, max_fragments):
    """per rendered batch of replay(tr, batch=batch, max_fragments=...), what the master carries: WRITES - a T_INIT,
    T_DEINIT or T_WRITE on one of its units; else WINDOWS - a T_PROCESS of one of them other than (0, the fragment's
    frames); else NONE.  (test_fbd_pan.py: song_record_free, which tells NONE from the rest.)"""
    units = set(units)
    out, what, pending, nfrag, frames = [], NONE, 0, 0, 0
    for r in tr.records:
        op = r[0]
        if op == T_FRAGMENT:
            if nfrag >= max_fragments:
                break
            if pending and nfrag % batch == 0:
                out.append(what)
                what, pending = NONE, 0
            frames = r[1]
            pending += frames
            nfrag += 1
        elif op == T_WAVEDROP:
            if pending:
                out.append(what)
                what, pending = NONE, 0
        elif op in (T_INIT, T_DEINIT, T_WRITE) and r[1] in units:
            what = WRITES
        elif op == T_PROCESS and r[1] in units and (r[2], r[3]) != (0, frames):
            what = max(what, WINDOWS)
    if pending:
        out.append(what)
    return out


@pytest.fixture(scope="module")
def songs():
    return {name: Trace(os.path.join(GOLDEN, f"{name}.trace.xz")) for name in SONGS}


@pytest.mark.parametrize("name", sorted(SONGS))
def test_song_premise(songs, name):
    """From the trace alone: at a player's buffer nearly every batch of a song's master is windows only."""
    tr = songs[name]
    delays, batches, none, windows, writes = SONGS[name]
    _voice, units = song_master(tr)
    assert len(units) == delays + 2
    whole = song_master_batches(tr, units, SONG_BATCH, 10 ** 9)
    assert (len(whole), whole.count(NONE), whole.count(WINDOWS), whole.count(WRITES)) == (batches, none, windows, writes)
    head = song_master_batches(tr, units, SONG_BATCH, SONG_FRAGS)
    assert head == [WRITES] + [WINDOWS] * 9


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SONGS))
def test_song_master_keeps_its_kernel_at_a_players_buffer(songs, monkeypatch, name):
    """The first 640 fragments in batches of 64: batch 0 carries the births, in batches 1 .. 9 the master's run is windows
    only and the windows launch renders it; the audio is the reference's."""
    monkeypatch.delenv("A2AMD_NO_FAST", raising=False)
    monkeypatch.delenv("A2AMD_BUS_WINDOWS", raising=False)
    tr = songs[name]
    cfg = tr.config
    be = make_gpu(cfg["samplerate"], cfg["basepitch"], cfg["channels"], max_batch=SONG_BATCH)
    pinfo, winfo = [], []
    inner = spy(be, pinfo, be.render)

    def render(frames):
        out = inner(frames)
        winfo.append(be.last_batch_bus_windows())
        return out
    be.render = render
    out = replay(tr, be, batch=SONG_BATCH, check_noise=True, max_fragments=SONG_FRAGS)
    be.close()
    got = fnv1a_fragments(out)
    want = np.load(os.path.join(GOLDEN, f"{name}.hash.npy"))[:SONG_FRAGS]
    assert len(got) == SONG_FRAGS
    bad = np.nonzero(got != want)[0]
    assert not bad.size, bad[:4]
    assert len(winfo) == SONG_FRAGS // SONG_BATCH
    assert winfo[0].fbdpan_voices == 0, winfo[0]
    for b in range(1, len(winfo)):
        w, p = winfo[b], pinfo[b]
        assert p.class_voices == 1 and p.max_delays == SONGS[name][0], f"batch {b}: {p}"
        assert (w.fbdpan_voices, w.refused_tiling, w.refused_cap, w.launched) == (1, 0, 0, 1), f"batch {b}: {w}"
