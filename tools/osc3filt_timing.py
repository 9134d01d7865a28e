"""What a three-oscillator subtractive lead costs: sustained `wtosc; wtosc+; wtosc+; filter12; panmix+ >` voices
(Scene.add_voices("osc3-filter-pan")) rendered by k_leaf_osc3filtpan (the default) or, with A2AMD_NO_FAST=1024 in the
environment, by the general kernel as before the class existed - the second setting must report class_voices 0.  One
fragment is walked by calls and rendered ahead of everything; then every batch goes through a2amd_fragment_repeat and
nothing else: no voice has a record.  Per batch: the a2amd_render() call as driven from Python, and the kernels' HIP-event
time with profiling on (a2amd_set_profiling: no graphs then).

Cells:
  r64, r1024, r16384   that many voices under the root, 64 fragments a batch: a player's 4 096-frame buffer
  g16384               16 384 voices under 256 delay groups of 64, 256 fragments a batch
  c6, c64, c1024, c16384   that many voices in one stereo group, 64 fragments a batch of which the first is cut in two -
                       (0, 31) (31, 33), walked by calls, the group once per window; the other 63 repeated: every lead's
                       run is windows only in every batch.  k_leaf_osc3filtpan_win renders them (include/a2amd_osc3win.h); with
                       A2AMD_NO_FAST=2048 the general kernel, as before that launch existed - window_voices must then be 0

usage: [A2AMD_NO_FAST=1024] tools/osc3filt_timing.py CELL [batches] [warm-up batches]   -> one JSON line
       tools/osc3filt_timing.py all OUT.jsonl [repeats]    every r and g cell, class on and off interleaved `repeats` (3)
                                                           times, one process each; the lines to OUT.jsonl, a table to stdout
       tools/osc3filt_timing.py cut OUT.jsonl [repeats]    the c cells likewise, the windows launch on and off (2048)"""
import ctypes, json, os, subprocess, sys, time

CELLS = ("r64", "r1024", "r16384", "g16384")
CUT_CELLS = ("c6", "c64", "c1024", "c16384")
OFF = "1024"
CUT_OFF = "2048"


def run_all(path, repeats, CELLS=CELLS, OFF=OFF):
    rows = []
    with open(path, "w") as out:
        for _rep in range(repeats):
            for cell in CELLS:
                for off in (False, True):
                    env = dict(os.environ)
                    env.pop("A2AMD_NO_FAST", None)
                    if off:
                        env["A2AMD_NO_FAST"] = OFF
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), cell], env=env, capture_output=True, text=True,
                                       timeout=240)
                    if r.returncode != 0:       # (nothing more is started on the device behind a failure)
                        sys.stderr.write(r.stdout + r.stderr)
                        sys.exit(f"{cell} (off={off}) ended with status {r.returncode}")
                    line = r.stdout.strip().splitlines()[-1]
                    out.write(line + "\n")
                    out.flush()
                    rows.append(json.loads(line))
    print("| cell | voices | fragments | class on: kernels ms per batch (runs) | off: ms per batch (runs) | off spread | on - off median |")
    print("|---|---|---|---|---|---|---|")
    for cell in CELLS:
        on = sorted(r["kernel_ms_per_batch"] for r in rows if r["cell"] == cell and r["no_fast"] == "0")
        off = sorted(r["kernel_ms_per_batch"] for r in rows if r["cell"] == cell and r["no_fast"] == OFF)
        one = next(r for r in rows if r["cell"] == cell)
        fmt = lambda xs: " / ".join(f"{x:.3f}" for x in xs)
        print(f"| {cell} | {one['voices']} | {one['fragments']} | {fmt(on)} | {fmt(off)} | {off[-1] - off[0]:.3f} | "
              f"{on[len(on) // 2] - off[len(off) // 2]:+.3f} |")


if len(sys.argv) > 1 and sys.argv[1] in ("all", "cut"):
    cut = sys.argv[1] == "cut"
    run_all(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 3, CUT_CELLS if cut else CELLS, CUT_OFF if cut else OFF)
    sys.exit(0)

cell = sys.argv[1] if len(sys.argv) > 1 else "r1024"
batches = int(sys.argv[2]) if len(sys.argv) > 2 else 12
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 4
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import audiality2_amd
from audiality2_amd import synth


class Stats(ctypes.Structure):
    _fields_ = [("fragments", ctypes.c_uint64), ("voice_fragments", ctypes.c_uint64), ("records", ctypes.c_uint64),
                ("launches", ctypes.c_uint64), ("last_kernel_ms", ctypes.c_double), ("last_leaf_ms", ctypes.c_double),
                ("live", ctypes.c_uint32 * 4), ("timed_leaf_ms", ctypes.c_double), ("timed_all_ms", ctypes.c_double),
                ("timed_batches", ctypes.c_uint64)]


nvoices = int(cell[1:])
bfrags = 256 if cell[0] == "g" else 64
be = audiality2_amd.open_backend(max_batch=bfrags)
sc = synth.Scene(be)
sc.root()
cutg = None
if cell[0] == "g":
    for g in range(256):
        sc.add_voices(nvoices // 256, "osc3-filter-pan", group=sc.add_group(preset="fmtest4"), total=nvoices)
elif cell[0] == "c":
    cutg = sc.add_bus_group()
    sc.add_voices(nvoices, "osc3-filter-pan", group=cutg, total=nvoices)
else:
    sc.add_voices(nvoices, "osc3-filter-pan", total=nvoices)


def walk_cut(g, windows=((0, 31), (31, 33))):
    """one 64-frame fragment in which the group g, and every lead in it, is walked once per window (Scene.walk otherwise)"""
    be.fragment(64)
    be.unit_process(sc.rootv[0], 0, 64)
    for a, m in windows:
        be.unit_process(g["units"][0], a, m)
        for units in g["leaves"]:
            for u in units:
                be.unit_process(u, a, m)
        be.inline_end(g["units"][0])
        for u in g["units"][1:]:
            be.unit_process(u, a, m)
    be.inline_end(sc.rootv[0])
    be.unit_process(sc.rootv[1], 0, 64)
    be.unit_process(sc.rootv[2], 0, 64)


sc.walk(64)
be.render(64)
rows, infos, winfos = [], [], []
for b in range(warm + batches):
    if b == warm:
        be.lib.a2amd_set_profiling(be.ctx, 1)
    if cutg:
        walk_cut(cutg)
        be.fragment_repeat(64, bfrags - 1)
    else:
        be.fragment_repeat(64, bfrags)
    t1 = time.perf_counter()
    out = be.render(64 * bfrags)
    t2 = time.perf_counter()
    if b >= warm:
        rows.append(t2 - t1)
        infos.append(be.last_batch_osc3filt())
        winfos.append(be.last_batch_osc3filt_windows())
st = Stats()
be.lib.a2amd_get_stats(be.ctx, ctypes.byref(st))
rec = np.array(rows) * 1e3
per = st.timed_all_ms / max(1, st.timed_batches)
print(json.dumps({"cell": cell, "no_fast": os.environ.get("A2AMD_NO_FAST", "0"), "voices": nvoices, "fragments": bfrags,
                  "batches": batches, "render_call_ms_median": float(np.median(rec)), "render_call_ms_min": float(rec.min()),
                  "render_call_ms_max": float(rec.max()), "kernel_ms_per_batch": per, "leaf_ms_per_batch": st.timed_leaf_ms / max(1, st.timed_batches),
                  "timed_batches": int(st.timed_batches),
                  "voice_samples_per_s": nvoices * bfrags * 64 / (per * 1e-3) if per > 0 else None,
                  "launched": sorted({int(i.launched) for i in infos}), "class_voices": sorted({int(i.class_voices) for i in infos}),
                  "quiet_voices": sorted({int(i.quiet_voices) for i in infos}), "record_voices": sorted({int(i.record_voices) for i in infos}),
                  "vpg": sorted({int(i.vpg) for i in infos}), "workgroups": sorted({int(i.workgroups) for i in infos}),
                  "window_voices": sorted({int(w.window_voices) for w in winfos}), "windows": sorted({int(w.windows) for w in winfos}),
                  "window_vpg": sorted({int(w.vpg) for w in winfos}), "window_workgroups": sorted({int(w.workgroups) for w in winfos}),
                  "peak": int(np.abs(out).max()), "sum": int(out.astype(np.int64).sum())}))
be.close()
