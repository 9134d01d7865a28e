"""The launch plan of a small scene that populates every range of the launch lists (a2amd_host.h: LEAF_*, DYN_*,
DepthRange), pinned: the audio against the oracle, and - what the parity suite would not notice, a class launched twice
over an empty list, a launch too few or too many - the kernel launches of every batch and every field of
a2amd_batch_info against tests/golden/launch_plan.json.

The fixture is a recording of this same test body on the library as it was BEFORE the launch lists became one table of
ranges (A2AMD_TEST_RECORD_PLAN=<path> writes it instead of comparing): it is never recorded on the code under test."""
import ctypes
import json
import os

import pytest

from audiality2_amd import synth
from conftest import GOLDEN, make_gpu, make_oracle
from test_gpu_parity import BatchInfo, first_diff, last_batch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "launch_plan.json")
WT = ("osc-pan", "osc2-pan", "osc-filter-pan", "osc2-filter-pan")
BATCHES, BFRAGS, FRAMES = 4, 8, 64       # (the lead-in batch and the three of the plan)


class Stats(ctypes.Structure):
    """a2amd_stats (include/a2amd.h)"""
    _fields_ = [("fragments", ctypes.c_uint64), ("voice_fragments", ctypes.c_uint64), ("records", ctypes.c_uint64),
                ("launches", ctypes.c_uint64), ("last_kernel_ms", ctypes.c_double), ("last_leaf_ms", ctypes.c_double),
                ("live_units", ctypes.c_uint32), ("live_voices", ctypes.c_uint32), ("live_waves", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("timed_leaf_ms", ctypes.c_double), ("timed_all_ms", ctypes.c_double),
                ("timed_batches", ctypes.c_uint64)]


def launches(gpu):
    st = Stats()
    gpu.lib.a2amd_get_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(Stats)]
    gpu.lib.a2amd_get_stats.restype = ctypes.c_int
    assert gpu.lib.a2amd_get_stats(gpu.ctx, ctypes.byref(st)) == 0
    return int(st.launches)


def _plan_scene(be, on_batch=None):
    """Root -> bus group B (depth 1: two thirds of every class), bus group A (depth 1: a quarter) -> delay group D
    (depth 2, inline -> fbdelay -> fbdelay: the rest).  Nothing but the groups mixes into the master bus, so a batch
    without records on a bus owner is a self-cleaning one.
    24 voices of each wavetable class, 6 each of fmmix-pan (six unit kinds) and fm2-pan: the one-launch fm rule.
    A lead-in batch takes the records of the voices' births (every voice carries its initial writes).  Then the three
    batches of the plan: batch 1 untouched, all quiet; before batch 2 control writes with a start offset to two voices
    of every wavetable class (one of them gliding) and to group A's panmix; before batch 3 one voice dies and two are
    born (a list rebuild)."""
    sc = synth.Scene(be)
    sc.root()
    B = sc.add_bus_group()
    A = sc.add_bus_group()
    D = sc.add_group()
    sc.groups.remove(D)         # (add_group puts it under the root: nested in A, it is walked at depth 2)
    A["subs"].append(D)
    by_chain = {}
    for chain in WT:
        for g, n in ((B, 16), (A, 6), (D, 2)):
            sc.add_voices(n, chain=chain, group=g, total=128)
            by_chain.setdefault(chain, []).extend(g["leaves"][-n:])
    for chain in ("fmmix-pan", "fm2-pan"):
        for g, n in ((B, 4), (A, 2)):
            sc.add_voices(n, chain=chain, group=g, total=128)
    chunks = []
    for b in range(BATCHES):
        if b == 2:
            for chain in WT:
                in_b, in_a = by_chain[chain][3], by_chain[chain][18]
                be.unit_write(in_b[0], 1, synth.fix(0.75), 17, 0)           # pitch, at once
                be.unit_write(in_a[0], 2, synth.fix(0.01), 200, 40000)      # amplitude, gliding
                be.unit_write(in_a[-1], 1, synth.fix(-0.5), 33, 0)          # pan
            be.unit_write(A["units"][1], 1, synth.fix(0.25), 33, 0)         # the group voice's pan
        if b == 3:
            victim = by_chain["osc-pan"][5]
            for u in victim:
                be.unit_deinit(u)
            B["leaves"].remove(victim)
            sc.add_voices(1, chain="osc2-pan", group=A, total=128)
            sc.add_voices(1, chain="osc-filter-pan", group=B, total=128)
        for _ in range(BFRAGS):
            sc.walk(FRAMES)
        chunks.append(be.render(BFRAGS * FRAMES))
        if on_batch:
            on_batch()
    return chunks


@pytest.fixture(scope="module")
def plan_want(oracle_lib):
    ora = make_oracle(oracle_lib)
    want = _plan_scene(ora)
    ora.close()
    for w in want:
        w.setflags(write=False)
    return want


# (A2AMD_WIN, A2AMD_O2F_MIN, A2AMD_NO_FAST, A2AMD_RVPW)
PLANS = {
    "windows": ("1", "8", None, None),              # window kernels; the o2f quiet kernel launched
    "recs_all": ("0", "8", None, None),             # records kernels: one launch for the four lists
    "recs_per_kind": ("0", "8", None, "1"),         # records kernels: a launch per list
    "o2f_below_min": ("1", None, None, None),       # 24 < 512 (the default): the whole class on the fourth exception list
    "no_fast": ("1", "8", "11", None),              # wtosc-panmix, wtosc-filter12-panmix, 2 x wtosc-panmix -> general kernel
    "no_recs_kernel": ("1", "8", "64", None),       # every record-carrying leaf voice on the fifth exception list
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_launch_plan_is_the_recorded_one(plan_want, monkeypatch, plan):
    """synth.py has no leaf chain that none of the class predicates accept: the general leaf segment is populated by the
    "no_fast" case alone, where A2AMD_NO_FAST sends three classes there."""
    win, o2f_min, no_fast, rvpw = PLANS[plan]
    for name, val in (("A2AMD_WIN", win), ("A2AMD_O2F_MIN", o2f_min), ("A2AMD_NO_FAST", no_fast), ("A2AMD_RVPW", rvpw)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    gpu = make_gpu(max_batch=BFRAGS)
    got = {"launches": [], "batch_info": []}
    seen = [launches(gpu)]

    def on_batch():
        seen.append(launches(gpu))
        got["launches"].append(seen[-1] - seen[-2])
        bi = last_batch(gpu)
        got["batch_info"].append({n: int(getattr(bi, n)) for n, _ in BatchInfo._fields_})

    out = _plan_scene(gpu, on_batch)
    gpu.close()
    for b in range(BATCHES):
        assert plan_want[b].any()
        assert first_diff(out[b], plan_want[b]) is None, f"batch {b}"
    record = os.environ.get("A2AMD_TEST_RECORD_PLAN")
    if record:
        plans = {}
        if os.path.exists(record):
            with open(record) as f:
                plans = json.load(f)
        plans[plan] = got
        with open(record, "w") as f:
            json.dump(plans, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    with open(FIXTURE) as f:
        want = json.load(f)[plan]
    print(plan, got)
    for b in range(BATCHES):
        assert got["launches"][b] == want["launches"][b], f"batch {b}: kernel launches"
        assert got["batch_info"][b] == want["batch_info"][b], f"batch {b}"
