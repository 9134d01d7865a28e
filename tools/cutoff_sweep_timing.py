"""What a sweeping filter costs: 16 384 osc-filter-pan voices x 64 fragments per batch, SWEEPS of them with a cutoff
ramp that outlasts the run.  Mode calls: every fragment walked by calls (a2amd_voice_process per voice) - the only way a
library from before the sweep pass can render the scene, and the bar.  Mode repeat: one fragment walked and rendered ahead
of everything, then every batch 64 fragments through a2amd_fragment_repeat - the coefficients made on the device
(a2amd_cutsweep.hip).  Per batch: the time the recording calls take as driven from Python (ctypes overhead included - the
same for any library), the a2amd_render() call, the kernels' HIP-event time.  LIB: the liba2amd.so to measure (two builds
interleaved: one process each).

usage: tools/cutoff_sweep_timing.py LIB calls|repeat SWEEPS [batches] [warm-up batches] [VOICES]  -> one JSON line"""
import ctypes, json, os, sys, time
lib, mode, sweeps = sys.argv[1], sys.argv[2], int(sys.argv[3])
batches = int(sys.argv[4]) if len(sys.argv) > 4 else 4
warm = int(sys.argv[5]) if len(sys.argv) > 5 else 2
nvoices = int(sys.argv[6]) if len(sys.argv) > 6 else 16384
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
sc.add_voices(nvoices, "osc-filter-pan", total=256)
heads = [u for u in sc.leaves]
# the sweeps: spread over the voices, 4 octaves up or down over (far) more frames than the run renders
step = max(1, nvoices // max(sweeps, 1))
for k in range(sweeps):
    be.unit_write(heads[(k * step) % nvoices][1], 0, synth.fix(4.0 if k % 2 else -1.0), 0, (1 << 20) << 8)


def walk():
    be.fragment(64)
    be.unit_process(sc.rootv[0], 0, 64)
    for units in heads:
        be.voice_process(units, 0, 64)
    be.inline_end(sc.rootv[0])
    be.unit_process(sc.rootv[1], 0, 64)
    be.unit_process(sc.rootv[2], 0, 64)


be.lib.a2amd_fragment_repeat.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint]
rows = []
if mode == "repeat":
    walk()
    be.render(64)
for b in range(warm + batches):
    if b == warm:
        be.lib.a2amd_set_profiling(be.ctx, 1)
    t0 = time.perf_counter()
    if mode == "calls":
        for _ in range(64):
            walk()
    else:
        rc = be.lib.a2amd_fragment_repeat(be.ctx, 64, 64)
        if rc:
            raise SystemExit(f"a2amd_fragment_repeat: {rc} ({be._err(be.ctx).decode()})")
    t1 = time.perf_counter()
    out = be.render(64 * 64)
    t2 = time.perf_counter()
    if b >= warm:
        rows.append((t1 - t0, t2 - t1))
st = Stats()
be.lib.a2amd_get_stats(be.ctx, ctypes.byref(st))
info = be.last_batch_sweeps() if hasattr(be.lib, "a2amd_last_batch_sweeps") else None
rec = np.array(rows) * 1e3
print(json.dumps({"lib": os.path.basename(os.path.dirname(lib)) + "/" + os.path.basename(lib), "mode": mode, "voices": nvoices,
                  "sweeps": sweeps, "batches": batches, "record_ms_median": float(np.median(rec[:, 0])),
                  "record_ms_min": float(rec[:, 0].min()), "record_ms_max": float(rec[:, 0].max()),
                  "render_call_ms_median": float(np.median(rec[:, 1])), "render_call_ms_min": float(rec[:, 1].min()),
                  "render_call_ms_max": float(rec[:, 1].max()),
                  "kernel_ms_per_batch": st.timed_all_ms / max(1, st.timed_batches), "timed_batches": int(st.timed_batches),
                  "filters": int(info.filters) if info else None, "ramp_windows": int(info.ramp_windows) if info else None,
                  "standin_voices": int(info.standin_voices) if info else None,
                  "peak": int(np.abs(out).max()), "sum": int(out.astype(np.int64).sum())}))
be.close()
