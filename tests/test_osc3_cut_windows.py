"""Three-oscillator subtractive leads whose only records of a batch are cut windows keep their class (include/a2amd_osc3win.h):
k_leaf_osc3filtpan_win, the windows launch, renders them and steps every ramper window by window, as the reference's
Process(offset, frames) calls do.  Every rendering bit for bit against the oracle's render of the same calls, batch by batch,
and every batch with who rendered what: a2amd_last_batch_osc3filt_windows, a2amd_last_batch_osc3filt and
a2amd_last_batch().general_voices.

A cut group is walked as the engine walks a voice whose VM (or whose parent's) woke inside a fragment: the whole group once
per window (test_bus_cut_windows.py: cut_walk).  Batches are 10 fragments at the most.  The expected counts are written down
from the scripts - who is cut, who is written, the host's bound for a glide (the write's frame + 256 + the ramp's frames) -
none is a recording of what the library said.

The tests without the gpu mark check the interface, from the trace alone what the fixture's leads carry batch by batch, and on
the oracle alone that the gliding scripts do what they are built for: a kernel that ignored the windows could not pass."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from audiality2_amd import synth
from audiality2_amd.replay import T_DEINIT, T_FRAGMENT, T_INIT, T_PROCESS, T_WAVEDROP, T_WRITE, Trace, replay
from conftest import GOLDEN, ROOT, fnv1a_fragments, make_gpu, make_oracle
from test_bus_cut_windows import cut_walk, cuts, gaps, halves, rows
from test_gpu_parity import first_diff, is_gpu, last_batch
from test_osc3_filt import (A, CUT, FIELDS, O3, P, PAN, Q, RECORD_BATCHES, VOL, W, auto_vpg, both, env, lead, lead_voices,
                            record_free, snap)

fix = synth.fix
WFIELDS = ("launched", "window_voices", "gliding_voices", "windows", "refused_tiling", "vpg", "workgroups", "reserved")
FRAGS = 10
SPAN = 64 * FRAGS


def counts(info, names):
    return tuple(int(getattr(info, n)) for n in names)


def wsnap(be, frames, got):
    """test_osc3_filt.snap, and behind its five the windows info: (audio, noise word, osc3filt info, batch info, sweep info,
    windows info)"""
    snap(be, frames, got)
    got[-1] = got[-1] + (be.last_batch_osc3filt_windows() if is_gpu(be) else None,)


def run(be, plan, walks, before=None):
    """walks[b](b, f, n) (or one walk for every batch) through plan, a render and a wsnap per batch; before[b](): the writes
    made in front of batch b"""
    got = []
    for b, frags in enumerate(plan):
        if before and b in before:
            before[b]()
        walk = walks[b] if isinstance(walks, (list, tuple)) else walks
        for f, n in enumerate(frags):
            walk(b, f, n)
        wsnap(be, sum(frags), got)
    return got


def old(i):
    return counts(i, ("launched", "class_voices", "quiet_voices", "gliding_voices", "record_voices"))


def new(w):
    return counts(w, ("launched", "window_voices", "gliding_voices", "windows", "refused_tiling"))


def check(got, want):
    """want, per batch: ((launched, class, quiet, gliding, record) of the old info, (launched, window voices, gliding, windows,
    refused) of the windows info, general_voices)"""
    assert len(got) == len(want)
    for b, ((_a, _n, i, gen, _s, w), (wi, ww, wgen)) in enumerate(zip(got, want)):
        assert old(i) == wi, f"batch {b}: {i}"
        assert new(w) == ww, f"batch {b}: {w}"
        assert gen.general_voices == wgen, f"batch {b}: {gen.general_voices}"
        assert w.reserved == 0 and i.reserved == 0
        if not w.launched:
            assert (w.vpg, w.workgroups) == (0, 0), f"batch {b}: {w}"


def bound(t_write, durs, t_batch):
    """voices the host's bound holds gliding at a batch that begins at frame t_batch: a2amd_unit_write's write frame + 64 +
    duration + 192"""
    return sum(t_write + 256 + d > t_batch for d in durs)


# ---- CPU ---------------------------------------------------------------------------------
def test_abi(gpu_lib):
    from audiality2_amd.replay import a2amd_osc3filt_batch_info, a2amd_osc3filt_windows_info
    text = open(os.path.join(ROOT, "include", "a2amd_osc3win.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(a2amd_[a-z_0-9]+)\s*\(", text))) == ["a2amd_last_batch_osc3filt_windows"]
    assert '#include "a2amd_osc3win.h"' in open(os.path.join(ROOT, "include", "a2amd.h")).read()
    assert hasattr(gpu_lib, "a2amd_last_batch_osc3filt_windows")
    assert C.sizeof(a2amd_osc3filt_windows_info) == 32
    assert [n for n, _ in a2amd_osc3filt_windows_info._fields_] == list(WFIELDS)
    assert all(t is C.c_uint32 for _n, t in a2amd_osc3filt_windows_info._fields_)
    fields = re.findall(r"uint32_t\s+(\w+);", text[text.index("typedef struct a2amd_osc3filt_windows_info"):])
    assert fields == list(WFIELDS)
    # the struct beside it keeps its layout
    assert C.sizeof(a2amd_osc3filt_batch_info) == 32 and [n for n, _ in a2amd_osc3filt_batch_info._fields_] == list(FIELDS)
    # NULL arguments are refused, not dereferenced
    gpu_lib.a2amd_last_batch_osc3filt_windows.restype = C.c_int
    gpu_lib.a2amd_last_batch_osc3filt_windows.argtypes = [C.c_void_p, C.c_void_p]
    assert gpu_lib.a2amd_last_batch_osc3filt_windows(None, None) != 0
    out = a2amd_osc3filt_windows_info()
    assert gpu_lib.a2amd_last_batch_osc3filt_windows(None, C.byref(out)) != 0


@pytest.fixture(scope="module")
def lead3():
    return Trace(os.path.join(GOLDEN, "lead3.trace.xz"))


FREE, WINDOWS, RECORDS = "F", "W", "R"


def window_batches(tr, voices, batch):
    """per voice, per rendered batch of replay(tr, batch=batch): FREE - no record (record_free's arithmetic); WINDOWS - no
    write, init or deinit, and the Process calls of every one of its units tile each fragment: starting at frame 0, each
    where the last one ended, none empty, ending at the fragment's frames; RECORDS - anything else.  And the most windows
    any voice has in a fragment."""
    owner = {u: v for v, us in voices.items() for u in us}
    out = {v: [] for v in voices}
    state = {v: FREE for v in voices}
    at = {}                         # unit -> the frame its next window of the open fragment must start at
    nwin = {}                       # unit -> its windows in the open fragment
    most = 0
    pending, nfrag, frames = 0, 0, 0

    def end_fragment():
        nonlocal most
        for u, a in at.items():
            v = owner[u]
            if a != frames:
                state[v] = RECORDS
            elif nwin[u] > 1 and state[v] == FREE:
                state[v] = WINDOWS
            most = max(most, nwin[u])
        at.clear()
        nwin.clear()

    def close():
        for v in voices:
            out[v].append(state[v])
            state[v] = FREE

    for r in tr.records:
        op = r[0]
        if op == T_FRAGMENT:
            end_fragment()
            if pending and nfrag % batch == 0:
                close()
                pending = 0
            frames = r[1]
            pending += frames
            nfrag += 1
        elif op == T_WAVEDROP:
            if pending:
                end_fragment()
                close()
                pending = 0
        elif op in (T_INIT, T_DEINIT, T_WRITE) and r[1] in owner:
            state[owner[r[1]]] = RECORDS
        elif op == T_PROCESS and r[1] in owner:
            u = r[1]
            if r[2] != at.get(u, 0) or r[3] == 0:
                state[owner[u]] = RECORDS
            at[u] = r[2] + r[3]
            nwin[u] = nwin.get(u, 0) + 1
    end_fragment()
    if pending:
        close()
    return out, most


# at 64 fragments a batch: batch 0 the births, batch 1 Glide3's writes (fragment 75), batch 23 record-free
WIN64 = [0, 3] + [6] * 21 + [0]


def win16():
    w = [0] * 94
    for b in RECORD_BATCHES[1:]:
        w[b] = 6
    return w


def test_fixture_premise(lead3):
    voices = lead_voices(lead3)
    assert len(voices) == 6
    for batch, want in ((64, WIN64), (16, win16())):
        cls, most = window_batches(lead3, voices, batch)
        free = record_free(lead3, voices, batch)
        for v in voices:        # (the same arithmetic as record_free where it says "free")
            assert [c == FREE for c in cls[v]] == free[v], (batch, v)
        per_batch = [sum(c == WINDOWS for c in col) for col in zip(*(cls[v] for v in sorted(voices)))]
        assert per_batch == want, (batch, per_batch)
        assert most == 2, (batch, most)
    assert sum(WIN64) == 129 and sum(win16()) == 144 and 4 not in RECORD_BATCHES
    # batch 4 at 16 fragments a batch: Glide3's writes land there - those three carry records, the Lead3 voices none
    cls, _most = window_batches(lead3, voices, 16)
    assert sorted(cls[v][4] for v in voices) == [FREE] * 3 + [RECORDS] * 3


# -- 1. at rest: different windows in one workgroup --
def rest_plan():
    plan = [[64] * FRAGS for _ in range(4)]
    plan[2][4] = 37
    return plan


def rest_script(windows=None):
    """7 leads in a stereo bus group cut by `cuts`, 3 in a second one cut by `halves`, 2 under the root, uncut.  windows:
    one function for both groups instead"""
    def script(be):
        be.noise.value = 0x3c3c
        sc = synth.Scene(be)
        sc.root()
        ga, gb = sc.add_bus_group(), sc.add_bus_group()
        sc.add_voices(7, O3, group=ga, total=16)
        sc.add_voices(3, O3, group=gb, total=16)
        sc.add_voices(2, O3, total=16)
        return run(be, rest_plan(), cut_walk(sc, {id(ga): windows or cuts, id(gb): windows or halves}))
    return script


def rest_want(b):
    plan = rest_plan()
    return 7 * rows(plan, b) + 3 * rows(plan, b, halves)


@pytest.mark.gpu
@pytest.mark.parametrize("vpg", [64, 3, 1])
def test_at_rest_different_windows_in_one_workgroup(oracle_lib, monkeypatch, vpg):
    env(monkeypatch, vpg=vpg)
    assert [rest_want(b) for b in range(1, 4)] == [7 * 18 + 3 * 20, 7 * 19 + 3 * 20, 7 * 18 + 3 * 20]
    got = both(oracle_lib, "rest", rest_script(), max_batch=FRAGS)
    want = [((0, 12, 0, 0, 12), (0, 0, 0, 0, 0), 12)]
    want += [((1, 12, 2, 0, 10), (1, 10, 0, rest_want(b), 0), 0) for b in range(1, 4)]
    check(got, want)
    for b in range(1, 4):
        i, w = got[b][2], got[b][5]
        assert (w.vpg, w.workgroups) == (vpg, (10 + vpg - 1) // vpg), (b, w)
        assert (i.vpg, i.workgroups) == (vpg, (12 + vpg - 1) // vpg), (b, i)


@pytest.mark.gpu
def test_at_rest_launch_shape_by_count(oracle_lib, monkeypatch):
    """no A2AMD_F2VPW: a 256th of the window voices a workgroup, at least one"""
    env(monkeypatch)
    got = both(oracle_lib, "rest", rest_script(), max_batch=FRAGS)
    check(got, [((0, 12, 0, 0, 12), (0, 0, 0, 0, 0), 12)] +
          [((1, 12, 2, 0, 10), (1, 10, 0, rest_want(b), 0), 0) for b in range(1, 4)])
    for b in range(1, 4):
        w = got[b][5]
        assert (w.launched, w.window_voices, w.vpg, w.workgroups) == (1, 10, auto_vpg(10), 10), (b, w)


# -- 2. gliding through windows --
G_WRITE = 2                     # the batch in front of which the ramps are written
G_BATCHES = 8
G_T = G_WRITE * SPAN
# frames.  Every ramp is at least three batches (1 920 frames) long and ends 30 frames into a cut fragment, 10 frames into its
# middle window [20, 47): the amplitude's in fragment 3 of batch 5, q's in fragment 0, the volume's in 6, the pan's in 9, the
# pitch's (the first oscillator's; the other's is 200 frames shorter) in fragment 0 of batch 6
G_DURS = {"pitch": 4 * SPAN + 30, "amp": 3 * SPAN + 3 * 64 + 30, "q": 3 * SPAN + 30, "vol": 3 * SPAN + 6 * 64 + 30,
          "pan": 3 * SPAN + 9 * 64 + 30}
G_KINDS = sorted(G_DURS)


def glide_writes(be, leads, only=None):
    d = G_DURS
    ws = {"pitch": [(leads[0][1], P, fix(2.4), 0, d["pitch"] << 8),         # two octaves and more: across mip levels, up
                    (leads[0][2], P, fix(-3.1), 0, (d["pitch"] - 200) << 8)],   # ... and down
          "amp": [(leads[1][0], A, fix(0.02), 0, d["amp"] << 8)],
          "q": [(leads[2][3], Q, fix(0.4), 0, d["q"] << 8)],
          "vol": [(leads[3][4], VOL, fix(0.3), 0, d["vol"] << 8)],
          "pan": [(leads[4][4], PAN, fix(1.4), 0, d["pan"] << 8)]}           # crosses a2s_pan_over on its way
    for kind in G_KINDS:
        if only in (None, kind):
            for w in ws[kind]:
                be.unit_write(*w)


def glide_script(only=None, windows=cuts):
    """one lead per ramper kind in a cut stereo group.  only: the one kind that is written; windows=None: uncut"""
    def script(be):
        be.noise.value = 0x6117
        sc = synth.Scene(be)
        sc.root()
        g = sc.add_bus_group()
        sc.add_voices(5, O3, group=g, total=16)
        walk = cut_walk(sc, [g] if windows else [], windows or cuts)
        return run(be, [[64] * FRAGS] * G_BATCHES, walk, before={G_WRITE: lambda: glide_writes(be, g["leaves"], only)})
    return script


# Where the reference's cut render differs from its whole-fragment render behind the write, by ramper kind.  Measured on the
# oracle; True for every kind: a window that does not divide what is left of a ramp evenly computes another delta
# (a2_PrepareRamper's division, a2_dsp.h:137), and one longer than the rest stretches it (:146).
G_DIFFERS = {"pitch": True, "amp": True, "q": True, "vol": True, "pan": True}


def test_gliding_script_does_what_it_is_built_for(oracle_lib):
    assert (G_T + G_DURS["amp"]) == 5 * SPAN + 3 * 64 + 30 and cuts(3, 64)[1] == (20, 27)
    assert all(d >= 3 * SPAN for d in G_DURS.values())
    # the bound's table of test 2: the bounds are 1 280 + 256 + the ramp - q 3 486, amp 3 678, vol 3 870, pan 4 062, pitch 4 126.
    # All five up to batch 5 (it begins at 3 200), volume, pan and pitch at batch 6 (3 840), nobody at batch 7 (4 480)
    assert [bound(G_T, G_DURS.values(), b * SPAN) for b in range(3, 8)] == [5, 5, 5, 3, 0]

    def on_oracle(script):
        ora = make_oracle(oracle_lib)
        got = script(ora)
        ora.close()
        return [g[0] for g in got]

    for kind in G_KINDS:
        cut = on_oracle(glide_script(only=kind))
        whole = on_oracle(glide_script(only=kind, windows=None))
        for b in range(G_WRITE):        # (at rest: a window changes nothing)
            assert first_diff(cut[b], whole[b]) is None, (kind, b)
        differs = [b for b in range(G_WRITE, G_BATCHES) if first_diff(cut[b], whole[b]) is not None]
        print(kind, "cut render differs from the whole-fragment render in batches", differs)
        assert bool(differs) == G_DIFFERS[kind], (kind, differs)
        assert all(b > G_WRITE for b in differs[-1:]), (kind, differs)     # (... in a batch behind the write)


@pytest.mark.gpu
def test_gliding_through_windows(oracle_lib, monkeypatch):
    env(monkeypatch)
    got = both(oracle_lib, "glide", glide_script(), max_batch=FRAGS)
    r = rows([[64] * FRAGS], 0)
    assert r == 18
    want = [((0, 5, 0, 0, 5), (0, 0, 0, 0, 0), 5), ((0, 5, 0, 0, 5), (1, 5, 0, 5 * r, 0), 0),
            ((0, 5, 0, 0, 5), (0, 0, 0, 0, 0), 5)]      # the write batch: the general kernel's
    for b in range(3, G_BATCHES):
        want.append(((0, 5, 0, 0, 5), (1, 5, bound(G_T, G_DURS.values(), b * SPAN), 5 * r, 0), 0))
    check(got, want)


# -- 3. handover in every direction --
H_WRITE = 4
H_T = H_WRITE * SPAN
# the cutoff ramp ends inside batch 4; the others run through batches 5 and 6 into 7
H_CUT = 500
H_DURS = {"amp": 1500, "q": 1700, "pan": 1600, "pitch": 1400}


def w17(f, n):
    return [(0, 5), (5, 12)] if n == 17 else cuts(f, n)


def handover_plan():
    plan = [[64] * FRAGS for _ in range(8)]
    plan[6][5] = 17
    return plan


def handover_script(be):
    """4 leads in a cut group, 1 under the root.  Batches: births, windows, whole fragments, windows, a write to three of
    the four (the general kernel's; the fourth stays with the windows launch), windows, windows with the 17-frame fragment
    cut as (0, 5) (5, 12), whole fragments"""
    be.noise.value = 0x4a4d
    sc = synth.Scene(be)
    sc.root()
    g = sc.add_bus_group()
    sc.add_voices(4, O3, group=g, total=16)
    sc.add_voices(1, O3, total=16)
    v = g["leaves"]
    cut, whole, cut17 = cut_walk(sc, [g]), cut_walk(sc, []), cut_walk(sc, [g], w17)

    def writes():
        be.unit_write(v[0][3], CUT, fix(4.0), 0, H_CUT << 8)                # a cutoff ramp that ends in this batch
        be.unit_write(v[0][0], A, fix(0.03), 30, H_DURS["amp"] << 8)
        be.unit_write(v[1][3], Q, fix(0.5), 0, H_DURS["q"] << 8)
        be.unit_write(v[1][4], PAN, fix(-1.3), 0, H_DURS["pan"] << 8)
        be.unit_write(v[2][1], P, fix(1.9), 0, H_DURS["pitch"] << 8)
        be.unit_write(v[2][4], VOL, fix(0.4), 10, 0)                        # (no duration: no bound)
    return run(be, handover_plan(), [cut, cut, whole, cut, cut, cut, cut17, whole], before={H_WRITE: writes})


@pytest.mark.gpu
def test_handover_in_every_direction(oracle_lib, monkeypatch):
    env(monkeypatch)
    got = both(oracle_lib, "handover", handover_script, max_batch=FRAGS)
    plan = handover_plan()
    assert H_CUT < SPAN and rows(plan, 6, w17) == 19 and sum(plan[6]) == SPAN - 47
    # gliding by the bound at batches 5, 6, 7: voice 0 (amp: 2 560 + 256 + 1 500 = 4 316), voice 1 (q 4 516, pan 4 416), voice 2
    # (pitch 4 216); the batches begin at 3 200, 3 840 and 4 433
    glide = [sum(H_T + 256 + d > t for d in (H_DURS["amp"], H_DURS["q"], H_DURS["pitch"])) for t in (5 * SPAN, 6 * SPAN, 7 * SPAN - 47)]
    assert glide == [3, 3, 1]
    want = [((0, 5, 0, 0, 5), (0, 0, 0, 0, 0), 5),
            ((1, 5, 1, 0, 4), (1, 4, 0, 4 * 18, 0), 0),
            ((1, 5, 5, 0, 0), (0, 0, 0, 0, 0), 0),
            ((1, 5, 1, 0, 4), (1, 4, 0, 4 * 18, 0), 0),
            ((1, 5, 1, 0, 4), (1, 1, 0, 18, 0), 3),
            ((1, 5, 1, 0, 4), (1, 4, glide[0], 4 * 18, 0), 0),
            ((1, 5, 1, 0, 4), (1, 4, glide[1], 4 * 19, 0), 0),
            ((1, 5, 5, glide[2], 0), (0, 0, 0, 0, 0), 0)]
    check(got, want)


# -- 4. window edges --
def ones(f, n):
    """fragment 0 of a batch in one-frame windows; fragments 1, 4, 7: (0, 1) (1, n - 2) (n - 1, 1); 2, 5, 8: halves"""
    if n < 3:
        return [(0, n)]
    if f == 0:
        return [(k, 1) for k in range(n)]
    if f % 3 == 1:
        return [(0, 1), (1, n - 2), (n - 1, 1)]
    return halves(f, n) if f % 3 == 2 and n > 31 else [(0, n)]


def edges_plan():
    plan = [[64] * FRAGS for _ in range(6)]
    plan[2][4] = 1              # a one-frame fragment, where the others have three windows
    plan[4][0] = 37             # 37 one-frame windows
    return plan


def edges_script(be):
    """the wave cases of test_osc3_filt.py::test_waves - looped and mip-mapped further up, the 1 000-sample wave (the modulo
    wrap), a one-shot wave that ends near frame 2 000, no wave, a pitch out of range - at each oscillator position, in a cut
    group"""
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
    base = (sc.wave_ids[3], sc.wave_ids[8], sc.wave_ids[14])
    kinds = [(sc.wave_ids[1], 3.3), (w_odd, 0.4), (w_shot, 0.0), (None, 0.0), (sc.wave_ids[2], 8.5)]
    for pos in range(3):
        for k, (wv, pitch) in enumerate(kinds):
            waves, pitches = list(base), [-0.5 + 0.1 * k, -0.49 + 0.1 * k, -1.5 + 0.1 * k]
            waves[pos], pitches[pos] = wv, pitch
            lead(be, sc, st["leaves"], waves, pitches, (0.2, 0.15, 0.1), cutoff=1.0 + 0.3 * k, q=2.0 + pos,
                 mix=(1.0, 0.2 * pos, 0.1 * k), pan=((3 * pos + k) % 7 - 3) / 4.0)
    lead(be, sc, st["leaves"], (None, None, None), (0.0, 0.0, 0.0), (0.2, 0.2, 0.2))        # nothing plays: a row of zeros

    def writes():       # what the windows launch stored is what the general kernel goes on from, and back
        be.unit_write(st["leaves"][-1][0], W, sc.wave_ids[5])
        for units in st["leaves"][:15:4]:
            be.unit_write(units[1], A, fix(0.05), 100, 0)
    return run(be, edges_plan(), cut_walk(sc, [st], ones), before={4: writes})


@pytest.mark.gpu
def test_window_edges(oracle_lib, monkeypatch):
    env(monkeypatch)
    plan = edges_plan()
    # the one-shot waves end 2 000 frames in: batch 3 begins at 1 857 (batch 2 has the one-frame fragment), frame 143 is in
    # its fragment 2, cut in halves - inside a window
    assert sum(sum(b) for b in plan[:3]) == 3 * SPAN - 63 and len(ones(0, 64)) == 64 and ones(4, 1) == [(0, 1)]
    assert ones(1, 64) == [(0, 1), (1, 62), (63, 1)] and len(ones(0, 37)) == 37
    got = both(oracle_lib, "edges", edges_script, max_batch=FRAGS)
    r = [rows(plan, b, ones) for b in range(6)]
    assert r[1] == 64 + 3 * 3 + 3 * 2 + 3 and r[2] == r[1] - 2 and r[4] == r[1] - 27
    want = [((0, 16, 0, 0, 16), (0, 0, 0, 0, 0), 16)]
    for b in range(1, 6):
        written = 5 if b == 4 else 0
        want.append(((0, 16, 0, 0, 16), (1, 16 - written, 0, (16 - written) * r[b], 0), written))
    check(got, want)


# -- 5. nesting --
def nested_script(be):
    """G, a stereo group cut by `cuts`, with 2 leads; S inside it - depth 2, cut with it - with 3"""
    be.noise.value = 0x2e57
    sc = synth.Scene(be)
    sc.root()
    g = sc.add_bus_group()
    s = sc.add_bus_group(parent=g)
    sc.add_voices(2, O3, group=g, total=16)
    sc.add_voices(3, O3, group=s, total=16)
    return run(be, rest_plan(), cut_walk(sc, [g]))


@pytest.mark.gpu
def test_leads_at_depth_two_inside_a_cut_group(oracle_lib, monkeypatch):
    env(monkeypatch)
    got = both(oracle_lib, "nested", nested_script, max_batch=FRAGS)
    plan = rest_plan()
    want = [((0, 5, 0, 0, 5), (0, 0, 0, 0, 0), 5)]
    want += [((0, 5, 0, 0, 5), (1, 5, 0, 5 * rows(plan, b), 0), 0) for b in range(1, 4)]
    check(got, want)


# -- 6. refused --
@pytest.mark.gpu
def test_windows_that_leave_a_gap_are_refused(oracle_lib, monkeypatch):
    """[0, 20) and [47, 64) only: windows only, but no tiling - the general kernel's, which renders the windows it is given
    (both groups cut that way: ten runs refused in every batch behind the births)"""
    env(monkeypatch)
    got = both(oracle_lib, "gap", rest_script(windows=gaps), max_batch=FRAGS)
    want = [((0, 12, 0, 0, 12), (0, 0, 0, 0, 0), 12)]
    want += [((1, 12, 2, 0, 10), (0, 0, 0, 0, 10), 10)] * 3
    check(got, want)


@pytest.mark.gpu
def test_windows_and_a_write_in_one_batch_are_the_general_kernels(oracle_lib, monkeypatch):
    env(monkeypatch)

    def script(be):
        be.noise.value = 0x3c3d
        sc = synth.Scene(be)
        sc.root()
        g = sc.add_bus_group()
        sc.add_voices(3, O3, group=g, total=16)
        v = g["leaves"]
        return run(be, [[64] * FRAGS] * 4, cut_walk(sc, [g]),
                   before={2: lambda: (be.unit_write(v[1][4], PAN, fix(0.5), 7, 0), be.unit_write(v[2][3], Q, fix(1.5)))})

    got = both(oracle_lib, "write", script, max_batch=FRAGS)
    want = [((0, 3, 0, 0, 3), (0, 0, 0, 0, 0), 3), ((0, 3, 0, 0, 3), (1, 3, 0, 54, 0), 0),
            ((0, 3, 0, 0, 3), (1, 1, 0, 18, 0), 2), ((0, 3, 0, 0, 3), (1, 3, 0, 54, 0), 0)]
    check(got, want)


# -- 7. A/B --
@pytest.mark.gpu
def test_switched_off_is_the_old_routing_and_the_same_audio(oracle_lib, monkeypatch):
    """A2AMD_NO_FAST=2048: no windows launch - every lead with a run is the general kernel's, as before.  =1024: no class."""
    env(monkeypatch, no_fast=2048)
    for key, script in (("rest", rest_script()), ("glide", glide_script())):
        got = both(oracle_lib, key, script, max_batch=FRAGS)
        for b, (_a, _n, i, gen, _s, w) in enumerate(got):
            assert counts(w, WFIELDS) == (0,) * 8, (key, b, w)
            assert gen.general_voices == i.record_voices, (key, b, gen.general_voices, i)
    got = both(oracle_lib, "rest", rest_script(), max_batch=FRAGS)
    assert [old(g[2]) for g in got] == [(0, 12, 0, 0, 12)] + [(1, 12, 2, 0, 10)] * 3
    env(monkeypatch, no_fast=1024)
    got = both(oracle_lib, "rest", rest_script(), max_batch=FRAGS)
    for b, (_a, _n, i, gen, _s, w) in enumerate(got):
        assert counts(w, WFIELDS) == (0,) * 8 and counts(i, FIELDS) == (0,) * 8, (b, w, i)


# -- 8. the fixture --
@pytest.mark.gpu
@pytest.mark.parametrize("batch", [64, 16])
def test_fixture_keeps_the_class_through_cut_windows(lead3, monkeypatch, batch):
    """lead3 replayed: hash-equal to the reference in every fragment; a lead is the windows launch's exactly in the batches
    the trace leaves it with windows alone, the whole-fragment launch's in those without a record, the general kernel's in
    the others"""
    env(monkeypatch)
    voices = lead_voices(lead3)
    free = record_free(lead3, voices, batch)
    quiet = [sum(col) for col in zip(*(free[v] for v in sorted(voices)))]
    win = WIN64 if batch == 64 else win16()
    cfg = lead3.config
    be = make_gpu(cfg["samplerate"], cfg["basepitch"], cfg["channels"], max_batch=batch)
    infos = []
    render = be.render

    def spy(*a, **kw):
        out = render(*a, **kw)
        infos.append((be.last_batch_osc3filt(), be.last_batch_osc3filt_windows(), last_batch(be)))
        return out

    be.render = spy
    out = replay(lead3, be, batch=batch, check_noise=True)
    be.close()
    want = np.load(os.path.join(GOLDEN, "lead3.hash.npy"))
    got = fnv1a_fragments(out)
    assert len(got) == len(want) == 1500
    bad = np.nonzero(got != want)[0]
    assert not bad.size, bad[:4]
    assert len(infos) == len(quiet) == len(win) == (94 if batch == 16 else 24)
    for k, ((i, w, gen), nq, nw) in enumerate(zip(infos, quiet, win)):
        assert (w.launched, w.window_voices, w.refused_tiling) == (int(nw > 0), nw, 0), (k, w)
        assert gen.general_voices == 6 - nq - nw, (k, gen.general_voices, nq, nw)
        assert (i.launched, i.quiet_voices, i.record_voices) == (int(nq > 0), nq, 6 - nq), (k, i, nq)
        assert i.class_voices == 6, (k, i)
    assert sum(w.window_voices for _i, w, _g in infos) == (144 if batch == 16 else 129)
