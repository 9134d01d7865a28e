"""What a delay chain that ends in a panmix costs: `inline 0 2; fbdelay 2 2 ...; panmix+ 2 > 2` owners under the root,
rendered by k_bus_fbdpan (the default) or, with A2AMD_NO_FAST=512 in the environment, by the general kernel as before
the class existed - the second setting must report class_voices 0.  One fragment is walked by calls and rendered ahead
of everything; then every batch goes through a2amd_fragment_repeat and nothing else: no voice has a record.  Per batch:
the a2amd_render() call as driven from Python, and the kernels' HIP-event time with profiling on (no graphs then).

Cells:
  a   one pan-tailed master (one delay) at depth 1 over 60 mixed leaves, 64 fragments a batch: a player's 4 096-frame buffer
  b   256 pan-tailed groups of two delays (fmtest4's taps) over 65 536 osc2-pan leaves, 256 fragments: BASELINE configs[3]
      with the tail
  c   a with the master's volume gliding through every timed batch (one long ramp written ahead of the warm-up)
  d   a walked by calls, with the master and everything below it cut in two windows in one fragment of every batch - what a
      song's root does to its master section once per player's buffer (core.c:1195) - volume and pan at rest: the master's
      run is windows only, k_bus_fbdpan's windows launch renders it (include/a2amd_buswin.h); with A2AMD_BUS_WINDOWS set
      the general kernel, as before the routing existed.  The cut leaves carry records either way
  e   d with the master's volume gliding through every timed batch
LIB (optional, A2AMD_LIB otherwise the tree's): the liba2amd.so to measure - a library from before the class has no
a2amd_last_batch_fbdpan and reports null counts.

usage: [A2AMD_NO_FAST=512] [A2AMD_BUS_WINDOWS=1] tools/fbdpan_timing.py CELL [batches] [warm-up batches] [LIB]  -> one JSON line"""
import ctypes, json, os, sys, time
cell = sys.argv[1] if len(sys.argv) > 1 else "a"
batches = int(sys.argv[2]) if len(sys.argv) > 2 else 12
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 4
if len(sys.argv) > 4:
    os.environ["A2AMD_LIB"] = sys.argv[4]
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import audiality2_amd
from audiality2_amd import synth


class Stats(ctypes.Structure):
    _fields_ = [("fragments", ctypes.c_uint64), ("voice_fragments", ctypes.c_uint64), ("records", ctypes.c_uint64),
                ("launches", ctypes.c_uint64), ("last_kernel_ms", ctypes.c_double), ("last_leaf_ms", ctypes.c_double),
                ("live", ctypes.c_uint32 * 4), ("timed_leaf_ms", ctypes.c_double), ("timed_all_ms", ctypes.c_double),
                ("timed_batches", ctypes.c_uint64)]


def pan_tailed(sc, delays, preset=None):
    """add_group(tail="panmix"), or the same chain by hand on a tree from before the parameter"""
    try:
        g = sc.add_group(delays=delays, tail="panmix")
    except TypeError:
        be, k = sc.be, sc._key()
        u = [be.unit_init(k, synth.K_INLINE, 0, 0, 2, 0)]
        u += [be.unit_init(k, synth.K_FBDELAY, 0, 2, 2, 0) for _ in range(delays)]
        u.append(be.unit_init(k, synth.K_PANMIX, synth.PROCADD, 2, 2, 1))
        g = dict(units=u, leaves=[])
        sc.groups.append(g)
    for i, d in enumerate(g["units"][1:1 + delays]):
        taps, gains = sc.FMTEST4[i % 2] if preset == "fmtest4" else ((63.1, 75.6, 100.4), (0.3, 0.25, 0.25))
        for reg, ms in enumerate(taps):
            sc.be.unit_write(d, reg, synth.fix(ms))
        for reg, gain in enumerate(gains):
            sc.be.unit_write(d, 4 + reg, synth.fix(gain))
    return g


bfrags = 256 if cell == "b" else 64
be = audiality2_amd.open_backend(max_batch=bfrags)
sc = synth.Scene(be)
sc.root()
if cell == "b":
    for g in range(256):
        grp = pan_tailed(sc, 2, preset="fmtest4")
        be.unit_write(grp["units"][-1], 1, synth.fix(((g % 17) - 8) / 16.0))
        sc.add_voices(256, "osc2-pan", group=grp, total=65536)
    master = None
else:
    master = pan_tailed(sc, 1)
    be.unit_write(master["units"][-1], 0, synth.fix(0.8))
    for chain in ("osc-pan", "osc2-pan", "osc-filter-pan"):
        sc.add_voices(20, chain, group=master, total=60)

CUT_FRAGMENT, CUT_AT = 17, 20


def walk_cut(f):
    """Scene.walk(64) with the master - inline, its leaves, the chain behind it - walked once per window in CUT_FRAGMENT"""
    be.fragment(64)
    be.unit_process(sc.rootv[0], 0, 64)
    for a, m in ([(0, CUT_AT), (CUT_AT, 64 - CUT_AT)] if f == CUT_FRAGMENT else [(0, 64)]):
        be.unit_process(master["units"][0], a, m)
        for units in master["leaves"]:
            for u in units:
                be.unit_process(u, a, m)
        be.inline_end(master["units"][0])
        for u in master["units"][1:]:
            be.unit_process(u, a, m)
    be.inline_end(sc.rootv[0])
    be.unit_process(sc.rootv[1], 0, 64)
    be.unit_process(sc.rootv[2], 0, 64)


sc.walk(64)
be.render(64)
rows = []
fp = []
bw = []
for b in range(warm + batches):
    if b == 0 and cell in "ce":
        # one ramp through every batch that follows: this batch carries the record, the others begin unsettled
        be.unit_write(master["units"][-1], 0, synth.fix(0.3), 0, ((warm + batches + 1) * bfrags * 64) << 8)
    if b == warm:
        be.lib.a2amd_set_profiling(be.ctx, 1)
    t0 = time.perf_counter()
    if cell in "de":
        for f in range(bfrags):
            walk_cut(f)
    else:
        be.fragment_repeat(64, bfrags)
    t1 = time.perf_counter()
    out = be.render(64 * bfrags)
    t2 = time.perf_counter()
    if b >= warm:
        rows.append((t1 - t0, t2 - t1))
        if hasattr(be.lib, "a2amd_last_batch_fbdpan"):
            fp.append(be.last_batch_fbdpan())
        if hasattr(be.lib, "a2amd_last_batch_bus_windows"):
            bw.append(be.last_batch_bus_windows())
st = Stats()
be.lib.a2amd_get_stats(be.ctx, ctypes.byref(st))
bus = be.last_batch_buses() if hasattr(be.lib, "a2amd_last_batch_buses") else None
rec = np.array(rows) * 1e3
print(json.dumps({"cell": cell, "no_fast": os.environ.get("A2AMD_NO_FAST", "0"), "bus_windows": os.environ.get("A2AMD_BUS_WINDOWS"), "lib": os.environ.get("A2AMD_LIB", "tree"),
                  "fragments": bfrags, "batches": batches, "render_call_ms_median": float(np.median(rec[:, 1])),
                  "render_call_ms_min": float(rec[:, 1].min()), "render_call_ms_max": float(rec[:, 1].max()),
                  "kernel_ms_per_batch": st.timed_all_ms / max(1, st.timed_batches), "timed_batches": int(st.timed_batches),
                  "class_voices": sorted({int(i.class_voices) for i in fp}) if fp else None,
                  "quiet_voices": sorted({int(i.quiet_voices) for i in fp}) if fp else None,
                  "gliding_voices": sorted({int(i.gliding_voices) for i in fp}) if fp else None,
                  "record_voices": sorted({int(i.record_voices) for i in fp}) if fp else None,
                  "fbdpan_windowed": sorted({int(i.fbdpan_voices) for i in bw}) if bw else None,
                  "fbdpan_windowed_gliding": sorted({int(i.fbdpan_gliding) for i in bw}) if bw else None,
                  "fbdpan_windows": sorted({int(i.fbdpan_windows) for i in bw}) if bw else None,
                  "windows_launched": sorted({int(i.launched) for i in bw}) if bw else None,
                  "fbd_voices": int(bus.fbd_voices) if bus else None, "generic_owners": int(bus.generic_voices) if bus else None,
                  "consume": int(bus.consume) if bus else None, "master_direct": int(bus.master_direct) if bus else None,
                  "peak": int(np.abs(out).max()), "sum": int(out.astype(np.int64).sum())}))
be.close()
