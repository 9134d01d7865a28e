"""What a noise voice costs: 16 384 noise-pan voices x 64 fragments per batch, every fragment walked by calls
(a2amd_voice_process per voice: a seed record and a host loop over its draws per window), or one fragment walked and
63 through a2amd_fragment_repeat_noise (the seeds made on the device).  Per batch: the time the recording calls take
as driven from Python (ctypes overhead included - the same for any library), the a2amd_render() call, and the kernels'
HIP-event time.  LIB: the liba2amd.so to measure (two builds interleaved: one process each).
Mode repeat_only: one fragment walked and rendered ahead of everything, then every batch 64 fragments through
a2amd_fragment_repeat_noise and nothing else - no noise voice has a record of its own, which is where k_leaf_noisepan
renders them (a library from before it: the stand-in record and the window kernels).
CHAIN: noise-pan (default) or noisefilt-pan - synth's wtosc (noise); filter12; panmix voice, k_leaf_noisefiltpan's (from
A2AMD_NZF_MIN of them on); VOICES: how many (default 16 384).

usage: tools/noise_repeat_timing.py LIB calls|repeat|repeat_only [batches] [warm-up batches] [CHAIN] [VOICES]  -> one JSON line"""
import ctypes, json, os, sys, time
lib, mode = sys.argv[1], sys.argv[2]
batches = int(sys.argv[3]) if len(sys.argv) > 3 else 8
warm = int(sys.argv[4]) if len(sys.argv) > 4 else 3
chain = sys.argv[5] if len(sys.argv) > 5 else "noise-pan"
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
be.noise.value = 0x2545F491
sc = synth.Scene(be)
sc.root()
sc.add_voices(nvoices, chain, total=256)
heads = [u for u in sc.leaves]


def walk():
    be.fragment(64)
    be.unit_process(sc.rootv[0], 0, 64)
    for units in heads:
        be.voice_process(units, 0, 64)
    be.inline_end(sc.rootv[0])
    be.unit_process(sc.rootv[1], 0, 64)
    be.unit_process(sc.rootv[2], 0, 64)


rows = []
if mode == "repeat_only":
    walk()
    be.render(64)
for b in range(warm + batches):
    if b == warm:
        be.lib.a2amd_set_profiling(be.ctx, 1)
    t0 = time.perf_counter()
    if mode == "calls":
        for _ in range(64):
            walk()
    elif mode == "repeat_only":
        be.fragment_repeat_noise(64, 64)
    else:
        walk()
        t0 = time.perf_counter()      # (the one walked fragment is not what is measured)
        be.fragment_repeat_noise(64, 63)
    t1 = time.perf_counter()
    out = be.render(64 * 64)
    t2 = time.perf_counter()
    if b >= warm:
        rows.append((t1 - t0, t2 - t1))
st = Stats()
be.lib.a2amd_get_stats(be.ctx, ctypes.byref(st))
# (who rendered the last batch's noise voices, where the library says)
quiet = be.last_batch_noise() if hasattr(be.lib, "a2amd_last_batch_noise") else None
if chain == "noisefilt-pan":
    quiet = be.last_batch_noise_filter() if hasattr(be.lib, "a2amd_last_batch_noise_filter") else None
rec = np.array(rows) * 1e3
print(json.dumps({"lib": os.path.basename(os.path.dirname(lib)) + "/" + os.path.basename(lib), "mode": mode, "chain": chain, "voices": nvoices,
                  "batches": batches, "record_ms_median": float(np.median(rec[:, 0])), "record_ms_min": float(rec[:, 0].min()),
                  "record_ms_max": float(rec[:, 0].max()), "render_call_ms_median": float(np.median(rec[:, 1])),
                  "render_call_ms_min": float(rec[:, 1].min()), "render_call_ms_max": float(rec[:, 1].max()),
                  "kernel_ms_per_batch": st.timed_all_ms / max(1, st.timed_batches), "timed_batches": int(st.timed_batches),
                  "quiet_launched": int(quiet.quiet_launched) if quiet else None,
                  "quiet_voices": int(quiet.quiet_voices) if quiet else None,
                  "noise": int(be.noise.value), "peak": int(np.abs(out).max()),
                  "sum": int(out.astype(np.int64).sum())}))
be.close()
