"""What a bare wtosc voice costs: N `struct { wtosc }` voices (synth's chain "osc": one oscillator wired straight into
channel 0 of its parent's bus) under N / 64 mono groups `inline 0 1; panmix+ 1 > 2` under the root.  One fragment is
walked by calls and rendered ahead of everything; then every batch is 64 fragments through a2amd_fragment_repeat and
nothing else - no voice has a record, which is where k_leaf_oscbare renders the voices and k_bus_driver the groups (a
library from before them: k_voices, one voice one serial chain, and the general kernel for every group).  Per batch: the
a2amd_render() call as driven from Python, and the kernels' HIP-event time with profiling on.
LIB: the liba2amd.so to measure (two builds interleaved: one process each).

usage: tools/bare_osc_timing.py LIB [VOICES] [batches] [warm-up batches]  -> one JSON line"""
import ctypes, json, os, sys, time
lib = sys.argv[1]
nvoices = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
batches = int(sys.argv[3]) if len(sys.argv) > 3 else 12
warm = int(sys.argv[4]) if len(sys.argv) > 4 else 4
os.environ["A2AMD_LIB"] = lib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import audiality2_amd
from audiality2_amd import synth


class Stats(ctypes.Structure):
    _fields_ = [("fragments", ctypes.c_uint64), ("voice_fragments", ctypes.c_uint64), ("records", ctypes.c_uint64),
                ("launches", ctypes.c_uint64), ("last_kernel_ms", ctypes.c_double), ("last_leaf_ms", ctypes.c_double),
                ("live", ctypes.c_uint32 * 4), ("timed_leaf_ms", ctypes.c_double), ("timed_all_ms", ctypes.c_double),
                ("timed_batches", ctypes.c_uint64)]


be = audiality2_amd.open_backend(max_batch=64)
sc = synth.Scene(be)
sc.root()
ngroups = max(1, nvoices // 64)
left = nvoices
for g in range(ngroups):
    m = sc.add_mono_group(pan=((g % 17) - 8) / 8.0)
    n = left if g == ngroups - 1 else 64
    sc.add_voices(n, "osc", group=m, total=256)
    left -= n

sc.walk(64)
be.render(64)
rows = []
for b in range(warm + batches):
    if b == warm:
        be.lib.a2amd_set_profiling(be.ctx, 1)
    t0 = time.perf_counter()
    be.fragment_repeat(64, 64)
    t1 = time.perf_counter()
    out = be.render(64 * 64)
    t2 = time.perf_counter()
    if b >= warm:
        rows.append((t1 - t0, t2 - t1))
st = Stats()
be.lib.a2amd_get_stats(be.ctx, ctypes.byref(st))
# (who rendered the last batch's voices and groups, where the library says)
bare = be.last_batch_bare() if hasattr(be.lib, "a2amd_last_batch_bare") else None
bus = be.last_batch_buses() if hasattr(be.lib, "a2amd_last_batch_buses") else None
rec = np.array(rows) * 1e3
print(json.dumps({"lib": os.path.basename(os.path.dirname(lib)) + "/" + os.path.basename(lib), "voices": nvoices, "groups": ngroups,
                  "batches": batches, "render_call_ms_median": float(np.median(rec[:, 1])),
                  "render_call_ms_min": float(rec[:, 1].min()), "render_call_ms_max": float(rec[:, 1].max()),
                  "kernel_ms_per_batch": st.timed_all_ms / max(1, st.timed_batches), "timed_batches": int(st.timed_batches),
                  "launched": int(bare.launched) if bare else None, "quiet_voices": int(bare.quiet_voices) if bare else None,
                  "vpw": int(bare.vpw) if bare else None, "mono_drivers": int(bare.mono_drivers) if bare else None,
                  "driver_voices": int(bus.driver_voices) if bus else None, "generic_owners": int(bus.generic_voices) if bus else None,
                  "peak": int(np.abs(out).max()), "sum": int(out.astype(np.int64).sum())}))
be.close()
