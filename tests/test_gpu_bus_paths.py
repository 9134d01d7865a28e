"""The two bus kernels of a2amd_fast.hip off their settled path, against the oracle, with the proof that they were
reached (a2amd_last_batch_buses, include/a2amd_bus.h).

k_bus_driver (inline; panmix 2->2; xinsert >: the root and the group drivers) renders a driver whose volume or pan
glides on one workgroup that steps both rampers through the batch first; k_bus_fbdchain renders chains of one to four
fbdelay units in rounds of as many fragments as the shortest tap allows.  Every GPU test renders one script on the
oracle and on the GPU, compares the audio batch by batch and asserts, batch by batch, who rendered the bus owners.  The
expected counts are tables written down from the script - which write lands in front of which batch, how long its ramp
is - by the frame arithmetic spelled out at each table; none is a recording of what the library said.

The tests without the gpu mark check on the oracle alone that each script does what it is built for: with a restatement
of the rampers (a2amd_dsp.h: ramp_set / ramp_prepare / ramp_run, i.e. a2_SetRamper / a2_PrepareRamper / a2_RunRamper)
where a ramp ends and when the pan clamp is on, and that the tables follow from the host's documented bound."""
import ctypes as C

import numpy as np
import pytest

from audiality2_amd import synth
from conftest import make_gpu, make_oracle

fix = synth.fix
PAN, VOL = 1, 0                                  # panmix registers
COUNTS = ("driver_voices", "driver_ramping", "driver_windows_dropped", "fbd_voices", "generic_voices")
BUFSIZE = 131072                                 # the delay line (fbdelay.c:27)


def first_diff(a, b):
    if a.shape != b.shape:
        return ("shape", a.shape, b.shape)
    d = np.nonzero(a != b)
    if not len(d[0]):
        return None
    i = int(np.argmin(d[1]))
    return int(d[0][i]), int(d[1][i]), int(a[d[0][i], d[1][i]]), int(b[d[0][i], d[1][i]])


def counts(bi, names=COUNTS):
    return tuple(int(getattr(bi, n)) for n in names)


def render_async(gpu, frames):
    """render(UPLOAD | SUBTREES | ROOT | READBACK | ASYNC) and a2amd_collect at once: the path on which the root may
    store the batch straight into the host's readback buffer"""
    gpu.lib.a2amd_collect.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_int32)), C.c_uint]
    assert gpu._render(gpu.ctx, 4 | 1 | 2 | 8 | 32, None, 0) == frames, gpu._err(gpu.ctx)
    out = np.zeros((2, frames), dtype=np.int32)
    p = (C.POINTER(C.c_int32) * 2)()
    for c in range(2):
        p[c] = out[c].ctypes.data_as(C.POINTER(C.c_int32))
    assert gpu.lib.a2amd_collect(gpu.ctx, p, frames) == frames, gpu._err(gpu.ctx)
    return out


def frag_plan(batches, bfrags, short=None):
    """the frames of every fragment, batch by batch: 64, and 37 in the fragment `short` = (batch, index)"""
    plan = [[64] * bfrags for _ in range(batches)]
    if short:
        plan[short[0]][short[1]] = 37
    return plan


def batch_starts(plan):
    return [sum(sum(b) for b in plan[:k]) for k in range(len(plan))]


def run_script(be, sc, plan, before=None, walk=None, render=None, info=None):
    """Walks and renders `plan`; before[b](): the writes made in front of batch b.  info: a list that gets
    a2amd_last_batch_buses() of every batch.  Returns the batches' audio."""
    chunks = []
    for b, frags in enumerate(plan):
        if before and b in before:
            before[b]()
        for f, n in enumerate(frags):
            if walk:
                walk(b, f, n)
            else:
                sc.walk(n)
        chunks.append(render(sum(frags)) if render else be.render(sum(frags)))
        if info is not None:
            info.append(be.last_batch_buses())
    return chunks


def bus_scene(be, root_leaves=True):
    """Root -> bus group A (depth 1) -> bus group C and delay group D (depth 2); bus group B (depth 1); three leaves
    straight under the root, or none.  6 osc-pan voices in every group.  Every bus owner is a driver or a delay chain
    and the leaves under the root add into the root's own bus, not into the master bus: a batch in which no bus owner
    carries a record is a self-cleaning one (a2amd_host.h: owners_all_driver, consume_ok) - the bus kernels zero what
    they read, and the root stores the master bus into the host's buffer where the render reads it back itself."""
    sc = synth.Scene(be, nwaves=4)
    sc.root()
    A = sc.add_bus_group()
    Cg = sc.add_bus_group(parent=A)
    D = sc.add_group(parent=A)
    B = sc.add_bus_group()
    for g in (A, Cg, D, B):
        sc.add_voices(6, chain="osc-pan", group=g, total=32)
    if root_leaves:
        sc.add_voices(3, chain="osc-pan", total=32)
    return sc, dict(root=sc.rootv, A=A["units"], B=B["units"], C=Cg["units"], D=D["units"], Cgroup=Cg)


# ---------------------------------------------------------------------------
# the rampers, restated (a2amd_dsp.h:22-58)
# ---------------------------------------------------------------------------
def _w(x):
    """int32 wrap-around"""
    return ((int(x) + 2 ** 31) % 2 ** 32) - 2 ** 31


def _cdiv(a, b):
    """C's integer division: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


class Ramper:
    def __init__(self, v):
        self.value = self.target = _w(v << 8)
        self.delta = self.timer = 0

    def set(self, target, start, dur):
        self.target = _w(target << 8)
        self.timer = _w(dur + start)
        if self.timer < 256:
            self.value = self.target
        else:
            self.value = _w(self.value + (_w(self.delta * start) >> 8))

    def prepare(self, frames):
        """returns the frames of this window after which the ramp is over, None where it is not over in this window"""
        if not self.timer:
            self.value, self.delta = self.target, 0
            return None
        left = self.timer >> 8
        if frames <= left:
            self.delta = _w(_cdiv(_w(self.target - self.value) * 256, self.timer))
            self.timer = _w(self.timer - (frames << 8))
            return None
        self.delta = _cdiv(_w(self.target - self.value), frames)
        self.timer = 0
        return left

    def run(self, frames):
        self.value = _w(self.value + _w(self.delta * frames))


def driver_model(plan, writes):
    """The panmix of one driver through `plan`, windows = fragments.  writes: (batch, reg, value, start, dur), made in
    front of the batch, or (batch, reg, value, start, dur, f): made behind the driver's window of the batch's fragment f.
    Per fragment (batch, index, running, clamp, ends): running - a ramper's timer or delta is not
    zero when the fragment begins (k_bus_driver's test for its one-workgroup path, taken at the batch's start); clamp -
    the flag panmix_process22 decides in front of a2_PrepareRamper (panmix.c:192-249); ends - the frames into the
    fragment at which the VOLUME ramp's timer runs out."""
    vol, pan = Ramper(65536), Ramper(0)
    out = []
    for b, frags in enumerate(plan):
        for wb, reg, value, start, dur, *at in writes:
            if wb == b and not at:
                (pan if reg == PAN else vol).set(value, start & 255, dur)
        for f, n in enumerate(frags):
            running = bool(vol.timer | vol.delta | pan.timer | pan.delta) or vol.value != vol.target or pan.value != pan.target
            clamp = abs(pan.target) > 0xffffff or abs(pan.value) > 0xffffff
            ends = vol.prepare(n)
            pan.prepare(n)
            out.append((b, f, running, clamp, ends))
            vol.run(n)
            pan.run(n)
            for wb, reg, value, start, dur, *at in writes:
                if wb == b and at == [f]:
                    (pan if reg == PAN else vol).set(value, start & 255, dur)
    return out


def bound_ramping(plan, writes, b):
    """include/a2amd_bus.h, driver_ramping: any write to a bus owner's panmix made at frame T - the frames of all
    fragments before the one it is made in or in front of - keeps the voice within the host's bound until frame
    T + ((start + dur) >> 8) + 256; a batch counts it when it begins before that."""
    t = batch_starts(plan)
    return any(wb < b and t[b] < t[wb] + sum(plan[wb][:at[0]] if at else ()) + (((start & 255) + dur) >> 8) + 256
               for wb, _r, _v, start, dur, *at in writes)


# ---------------------------------------------------------------------------
# a. driver ramps across batches
# ---------------------------------------------------------------------------
# lead-in 0 (births), 1 (settled); writes in front of 2; C's way back in front of 4, A's in front of 5
A_BATCHES, A_WRITE, A_BACK, A_AGAIN = 10, 2, 4, 5


def a_plan(bfrags):
    return frag_plan(A_BATCHES, bfrags, short=(3, 5))


def a_writes(bfrags):
    """driver -> its writes (batch, reg, value, start, dur), the low byte of dur a fraction of a frame"""
    plan = a_plan(bfrags)
    two = sum(plan[A_WRITE]) + sum(plan[A_WRITE + 1])
    return {
        # ends 21 frames into the twelfth fragment behind the write
        "root": [(A_WRITE, VOL, fix(0.3), 33, ((11 * 64 + 21) << 8) + 77)],
        # beyond +-1: clamped all the way.  Then back to 0.9 over 1536 frames: the value comes inside +-1 after four
        # fifths of them, 1229 frames behind the write - in a batch behind the write's own at 8 and at 16 fragments, where
        # k_bus_driver has to decide the clamp fragment by fragment: on in its first fragments, off in its last
        "A": [(A_WRITE, PAN, fix(1.4), 0, (20 * 64) << 8), (A_AGAIN, PAN, fix(0.9), 0, (24 * 64) << 8)],
        # ... and back inside from beyond: clamped until the value is inside
        "C": [(A_WRITE, PAN, fix(-1.3), 200, ((5 * 64 + 1) << 8) + 255), (A_BACK, PAN, fix(0.5), 0, (14 * 64) << 8)],
        # its batch and the next one, whole: over on the batch boundary, the delta stale in the batch behind it
        "B": [(A_WRITE, VOL, fix(0.35), 0, two << 8)],
    }


# (driver_voices, driver_ramping, driver_windows_dropped, fbd_voices, generic_voices) of batches 1 .. 9.  Bus owners:
# root, A, B, C (drivers) and D (two delays).  With t the frame at which batch 2 begins, a batch is 512 frames at 8
# fragments, 1024 at 16, and batch 3 is 27 short.  The host's bound (a2amd_bus.h) is the ramp's length + 256:
#                   root 725 + 256 = 981    A 1280 + 256 = 1536    C 322 + 256 = 578
#                   from their batches on: C's way back (4) 896 + 256 = 1152, A's (5) 1536 + 256 = 1792
#   8 fragments:    B 512 + 485 + 256 = 1253;  batches 3 .. 9 begin at t + 512, 997, 1509, 2021, 2533, 3045, 3557
#        batch 2: the four written drivers carry records.  3: all four within their bounds.  4: C written again; A and B.
#        5: A written again; C (512 < 1152).  6: A (512 < 1792) and C (1024 < 1152).  7, 8: A (1024, 1536).  9: nobody.
#   16 fragments:   B 1024 + 997 + 256 = 2277;  batches 3 .. 9 begin at t + 1024, 2021, 3045, 4069, 5093, 6117, 7141
#        3: A (1024 < 1536) and B.  4: C written; B (2021 < 2277).  5: A written; C (1024 < 1152).  6: A (1024 < 1792).
#        7 .. 9: nobody.
A_COUNTS = {
    8: [(4, 0, 0, 1, 0), (0, 0, 0, 1, 4), (4, 4, 0, 1, 0), (3, 2, 0, 1, 1), (3, 1, 0, 1, 1), (4, 2, 0, 1, 0), (4, 1, 0, 1, 0), (4, 1, 0, 1, 0),
        (4, 0, 0, 1, 0)],
    16: [(4, 0, 0, 1, 0), (0, 0, 0, 1, 4), (4, 2, 0, 1, 0), (3, 1, 0, 1, 1), (3, 1, 0, 1, 1), (4, 1, 0, 1, 0), (4, 0, 0, 1, 0), (4, 0, 0, 1, 0),
         (4, 0, 0, 1, 0)],
}


def a_script(be, bfrags, ramps=True, root_leaves=True, render=None, info=None):
    sc, u = bus_scene(be, root_leaves)
    before = {}
    if ramps:
        for name, ws in a_writes(bfrags).items():
            for b, reg, value, start, dur in ws:
                before.setdefault(b, []).append((u[name][1], reg, value, start, dur))
    return run_script(be, sc, a_plan(bfrags), render=render, info=info,
                      before={b: (lambda ws=ws: [be.unit_write(*w) for w in ws]) for b, ws in before.items()})


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


@pytest.mark.parametrize("bfrags", [8, 16])
def test_ramp_script_does_what_it_is_built_for(oracle_memo, bfrags):
    plan, writes = a_plan(bfrags), a_writes(bfrags)
    model = {name: driver_model(plan, ws) for name, ws in writes.items()}
    # A: clamped in every fragment from the write on, until it is written again.  C's way back: clamped at first, then not,
    # the ramp still going
    assert all(clamp for b, f, running, clamp, ends in model["A"] if A_WRITE <= b < A_AGAIN)
    # A's way back comes inside in the middle of a batch without a record: k_bus_driver's one workgroup sees the flag
    # change from one fragment to the next.  At 8 fragments the ramp goes on to the batch's end; at 16 it is over with
    # the batch's eighth fragment and the rampers are at rest from the tenth on - the end state that workgroup stores
    cross = A_AGAIN + (2 if bfrags == 8 else 1)
    assert [(running, clamp) for b, f, running, clamp, ends in model["A"] if b == cross] == \
        [(True, True)] * 4 + [(True, False)] * (4 if bfrags == 8 else 5) + [(False, False)] * (0 if bfrags == 8 else 7)
    back = [(running, clamp) for b, f, running, clamp, ends in model["C"] if b >= A_BACK]
    assert (True, True) in back and (True, False) in back
    # C is at rest at -1.3 when its way back is written
    assert not any(running for b, f, running, clamp, ends in model["C"] if b == A_BACK - 1)
    # the root's ramp is over strictly inside a fragment ...
    ends = [(b, f, e) for b, f, running, clamp, e in model["root"] if e is not None]
    assert len(ends) == 1 and 0 < ends[0][2] < plan[ends[0][0]][ends[0][1]]
    # ... at 8 fragments of a batch in which no bus owner carries a record: k_bus_driver's (at 16 of the write's own)
    assert ends[0][:2] == ((A_WRITE + 1, 3) if bfrags == 8 else (A_WRITE, 11))
    # B's is over with the last frame of batch 3, and batch 4 begins on the stale delta
    assert [(b, f) for b, f, running, clamp, e in model["B"] if running][-1] == (A_WRITE + 2, 0)
    # at 8 fragments every driver begins a batch without a record of its own unsettled: the one-workgroup path.  At 16
    # the root's ramp and C's two are over within the batches of their writes: A and B
    for name in (writes if bfrags == 8 else "AB"):
        rec = {w[0] for w in writes[name]}
        assert any(running and f == 0 and b not in rec for b, f, running, clamp, ends in model[name]), name
    # the table is the host's bound applied to the script, and whoever begins a batch unsettled is within it
    for b in range(1, A_BATCHES):
        listed = [n for n in writes if b not in {w[0] for w in writes[n]}]
        row = A_COUNTS[bfrags][b - 1]
        assert row == (len(listed), sum(bound_ramping(plan, writes[n], b) for n in listed), 0, 1, 4 - len(listed)), b
        for n in listed:
            unsettled = next(running for bb, f, running, clamp, ends in model[n] if (bb, f) == (b, 0))
            assert not unsettled or bound_ramping(plan, writes[n], b), (b, n)
    # heard: every batch from the write on differs from the same scene left alone
    want = oracle_memo(("a", bfrags, True), lambda be: a_script(be, bfrags))
    flat = oracle_memo(("a-flat", bfrags), lambda be: a_script(be, bfrags, ramps=False))
    for b in range(A_BATCHES):
        assert want[b].any()
        assert (first_diff(want[b], flat[b]) is not None) == (b >= A_WRITE), b


@pytest.mark.gpu
@pytest.mark.parametrize("bfrags,root_leaves", [(8, True), (16, True), (8, False)])
def test_driver_ramps_across_batches_match_oracle(oracle_memo, bfrags, root_leaves):
    """k_bus_driver with gridDim.y = 2 (8 fragments) and 16 (16 fragments) for the drivers at rest, and its launch of one
    workgroup a voice for those in flight: the root's volume, A's pan (clamped all the way, then back inside in the middle
    of a batch), C's pan out beyond -1 and back inside, B's volume to the very end of a batch.  At 16 fragments only A's
    and B's ramps reach beyond the batches of their writes.  The batches without a record on a bus owner are
    self-cleaning ones: the ramping root stores the host's buffer.  Without leaves under the root, through the
    asynchronous readback."""
    want = oracle_memo(("a", bfrags, root_leaves), lambda be: a_script(be, bfrags, root_leaves=root_leaves))
    gpu = make_gpu(max_batch=bfrags)
    info = []
    got = a_script(gpu, bfrags, root_leaves=root_leaves, info=info,
                   render=None if root_leaves else (lambda frames: render_async(gpu, frames)))
    gpu.close()
    for b in range(A_BATCHES):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {info[b]}"
    for b in range(1, A_BATCHES):
        assert counts(info[b]) == A_COUNTS[bfrags][b - 1], f"batch {b}: {info[b]}"
        # a record on a bus owner: a memset and an adding root, a copy behind the batch
        quiet = A_COUNTS[bfrags][b - 1][4] == 0
        assert (info[b].consume, info[b].master_direct) == ((3, 1) if quiet else (0, 0)), f"batch {b}"


# ... and with more workgroups than the device holds at once.  A driver at rest has 16 workgroups at 64 fragments, and
# from 2 048 workgroups of 256 threads on the last ones start when the first have finished.  A ramp that is over in the
# middle of a batch leaves the rampers settled: a workgroup that looked at them only then, and took the voice for one at
# rest, would render its fragments a second time.  The drivers in flight have a launch of their own, one workgroup each.
M_GROUPS, M_FRAGS, M_BATCHES = 160, 64, 4
M_RAMP = (1, VOL, fix(0.45), 0, (84 * 64) << 8)
# written in front of batch 1; within the bound while a batch begins before t + 5376 + 256: batch 2 (t + 4096; batch 3 at
# t + 8192).  The root and 160 groups.
M_COUNTS = [(1, 0, 0, 0, 160), (161, 160, 0, 0, 0), (161, 0, 0, 0, 0)]


def m_script(be, info=None):
    sc = synth.Scene(be, nwaves=4)
    sc.root()
    groups = [sc.add_bus_group() for _ in range(M_GROUPS)]
    for g in groups:
        sc.add_voices(1, chain="osc-pan", group=g, total=M_GROUPS)
    before = {M_RAMP[0]: lambda: [be.unit_write(g["units"][1], M_RAMP[1], M_RAMP[2] + 64 * k, M_RAMP[3], M_RAMP[4])
                                  for k, g in enumerate(groups)]}
    return run_script(be, sc, frag_plan(M_BATCHES, M_FRAGS), before=before, info=info)


def test_many_drivers_script_does_what_it_is_built_for():
    plan = frag_plan(M_BATCHES, M_FRAGS)
    assert [bound_ramping(plan, [M_RAMP], b) for b in range(1, M_BATCHES)] == [row[1] > 0 for row in M_COUNTS]
    # over with fragment 19 of batch 2, settled from fragment 21 on: most of the batch behind the ramp's end
    model = driver_model(plan, [M_RAMP])
    assert [(b, f) for b, f, running, clamp, ends in model if running][-1] == (2, 20)
    assert (M_GROUPS + 1) * 16 > 2048


@pytest.mark.gpu
def test_many_drivers_whose_ramps_end_inside_a_batch_match_oracle(oracle_memo):
    """A guard for the shape, not a reproduction: the kernel from before the drivers in flight had their own launch
    passed this test too when it was tried - whether a workgroup starts late enough is the device's business.  That the
    two launches cannot render a fragment twice follows from the kernel's text, not from this test."""
    want = oracle_memo("m", m_script)
    gpu = make_gpu(max_batch=M_FRAGS)
    info = []
    got = m_script(gpu, info=info)
    gpu.close()
    for b in range(M_BATCHES):
        assert want[b].any()
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {info[b]}"
    for b in range(1, M_BATCHES):
        assert counts(info[b]) == M_COUNTS[b - 1], f"batch {b}: {info[b]}"


# ... and the writes that are no glides by their dur, made at the very end of a batch.  a2_SetRamper starts a ramp from
# start + dur >= 256 on: start 200, dur 100 is a ramp of one frame, which the next window stretches to its own length
# and leaves with a delta until the window after it.  Below that the write still leaves the timer set until the next
# window.  Either way the driver begins the next batch unsettled, without a record: it must be on the list of
# k_bus_driver's second launch, or nobody renders it - then and ever after.
L_BATCHES, L_FRAGS = 5, 8
L_WRITES = {"C": [(2, PAN, fix(-0.8), 200, 100, 6)],        # behind C's window of fragment 6: fragment 7 runs the ramp
            "B": [(2, VOL, fix(0.4), 33, 0, 7)]}            # behind B's last window of the batch: the timer stays set
# batches 1 .. 4: batch 2 carries the two records; batch 3 begins 128 and 64 frames behind the fragments of the writes,
# within 1 + 256 and 0 + 256; batch 4, 512 frames later, does not
L_COUNTS = [(4, 0, 0, 1, 0), (2, 0, 0, 1, 2), (4, 2, 0, 1, 0), (4, 0, 0, 1, 0)]


def l_script(be, writes=True, info=None):
    sc, u = bus_scene(be)
    g = {"C": u["Cgroup"], "B": sc.groups[1]}

    def walk(b, f, n):
        sc.walk(n)
        for name, ws in L_WRITES.items():
            for wb, reg, value, start, dur, at in ws:
                if writes and (wb, at) == (b, f):
                    be.unit_write(g[name]["units"][1], reg, value, start, dur)
    return run_script(be, sc, frag_plan(L_BATCHES, L_FRAGS), walk=walk, info=info)


def test_late_writes_script_does_what_it_is_built_for(oracle_memo):
    plan = frag_plan(L_BATCHES, L_FRAGS)
    for name, ws in L_WRITES.items():
        assert all(dur < 256 for _b, _r, _v, _s, dur, _f in ws)
        model = driver_model(plan, ws)
        # unsettled when batch 3 begins, and only then; and whoever begins a batch unsettled is within the host's bound
        assert [b for b, f, running, clamp, ends in model if f == 0 and running] == [3], name
        for b in range(1, L_BATCHES):
            assert bound_ramping(plan, ws, b) == (b == 3), (name, b)
    assert L_COUNTS == [(4, 0, 0, 1, 0), (2, 0, 0, 1, 2)] + [(4, 2 * bound_ramping(plan, L_WRITES["C"], b), 0, 1, 0) for b in (3, 4)]
    want = oracle_memo("l", l_script)
    # heard: from the batch behind the writes on (in their own batch C's lasts one fragment, B's is behind the last window)
    flat = oracle_memo("l-flat", lambda be: l_script(be, writes=False))
    for b in range(L_BATCHES):
        assert want[b].any()
        assert (first_diff(want[b], flat[b]) is not None) == (b >= 2), b


@pytest.mark.gpu
def test_writes_at_the_end_of_a_batch_that_leave_a_driver_unsettled_match_oracle(oracle_memo):
    want = oracle_memo("l", l_script)
    gpu = make_gpu(max_batch=L_FRAGS)
    info = []
    got = l_script(gpu, info=info)
    gpu.close()
    for b in range(L_BATCHES):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {info[b]}"
    for b in range(1, L_BATCHES):
        assert counts(info[b]) == L_COUNTS[b - 1], f"batch {b}: {info[b]}"


# ---------------------------------------------------------------------------
# b. cut windows on a driver
# ---------------------------------------------------------------------------
B_BATCHES, B_FRAGS, B_WRITE = 7, 8, 2
B_RAMP = (B_WRITE, PAN, fix(-0.6), 0, (19 * 64 + 30) << 8)
# C's pan is written in front of batch 2 (its record: the general kernel) and the host counts it ramping while a batch
# begins before t + 1246 + 256: batches 3 and 4 (t + 512, t + 1024; batch 5 at t + 1536).  The ramp is over 30 frames
# into batch 4's fourth fragment, a cut one: in the window [20, 47), which then brings the ramp to its end by frame 47
# where the whole fragment would take until frame 64.  There C's cut windows are records the general
# kernel must execute (every window prepares the rampers anew); in batches 1, 5 and 6 C is at rest, the windows change
# nothing and are dropped - C stays k_bus_driver's.  Nobody else has a ramp or a record.
B_COUNTS = [(4, 0, 1, 1, 0), (3, 0, 0, 1, 1), (3, 0, 0, 1, 1), (3, 0, 0, 1, 1), (4, 0, 1, 1, 0), (4, 0, 1, 1, 0)]


def b_script(be, cuts=True, ramp=True, info=None):
    """bus_scene with C walked in the windows [0, 20), [20, 47), [47, 64) in every third fragment"""
    sc, u = bus_scene(be)
    rootv, A, Cg, D, B = sc.rootv, sc.groups[0], u["Cgroup"], sc.groups[0]["subs"][1], sc.groups[1]

    def group(g, a=0, n=64):
        be.unit_process(g["units"][0], a, n)
        for units in g["leaves"]:
            for x in units:
                be.unit_process(x, a, n)
        be.inline_end(g["units"][0])
        for x in g["units"][1:]:
            be.unit_process(x, a, n)

    def walk(b, f, n):
        be.fragment(n)
        be.unit_process(rootv[0], 0, n)
        be.unit_process(A["units"][0], 0, n)
        edges = [0, 20, 47, 64] if cuts and f % 3 == 0 else [0, 64]
        for lo, hi in zip(edges[:-1], edges[1:]):
            group(Cg, lo, hi - lo)
        group(D)
        for units in A["leaves"]:
            for x in units:
                be.unit_process(x, 0, n)
        be.inline_end(A["units"][0])
        for x in A["units"][1:]:
            be.unit_process(x, 0, n)
        group(B)
        for units in sc.leaves:
            for x in units:
                be.unit_process(x, 0, n)
        be.inline_end(rootv[0])
        be.unit_process(rootv[1], 0, n)
        be.unit_process(rootv[2], 0, n)

    before = {B_WRITE: lambda: be.unit_write(u["C"][1], *B_RAMP[1:])} if ramp else None
    return run_script(be, sc, frag_plan(B_BATCHES, B_FRAGS), before=before, walk=walk, info=info)


def test_cut_windows_script_does_what_it_is_built_for(oracle_memo):
    """At rest the cut windows change nothing - which is why the host may drop them; while the pan ramps they do."""
    plan = frag_plan(B_BATCHES, B_FRAGS)
    for b in range(1, B_BATCHES):
        ramping = bound_ramping(plan, [B_RAMP], b)
        assert B_COUNTS[b - 1] == ((3, 0, 0, 1, 1) if b == B_WRITE or ramping else (4, 0, 1, 1, 0)), b
    # (the model's windows are whole fragments)
    model = driver_model(plan, [(B_WRITE, VOL) + B_RAMP[2:]])
    assert [(b, f, e) for b, f, running, clamp, e in model if e is not None] == [(B_WRITE + 2, 3, 30)]
    cut = oracle_memo("b", b_script)
    whole = oracle_memo("b-whole", lambda be: b_script(be, cuts=False))
    rest = oracle_memo("b-rest", lambda be: b_script(be, ramp=False))
    rest_whole = oracle_memo("b-rest-whole", lambda be: b_script(be, cuts=False, ramp=False))
    for b in range(B_BATCHES):
        assert first_diff(rest[b], rest_whole[b]) is None, b
        if b not in (B_WRITE, B_WRITE + 1):     # (there the windows move a delta by an LSB at the most)
            assert (first_diff(cut[b], whole[b]) is not None) == (b == B_WRITE + 2), b
        assert (first_diff(cut[b], rest[b]) is not None) == (b >= B_WRITE), b


@pytest.mark.gpu
def test_cut_windows_on_a_driver_at_rest_and_ramping_match_oracle(oracle_memo):
    """a2amd_sched.cpp, upload(): a driver at rest whose records are windows only stays with k_bus_driver, its records
    dropped; one whose pan ramps must keep them and go to the general kernel."""
    want = oracle_memo("b", b_script)
    gpu = make_gpu(max_batch=B_FRAGS)
    info = []
    got = b_script(gpu, info=info)
    gpu.close()
    for b in range(B_BATCHES):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {info[b]}"
    for b in range(1, B_BATCHES):
        assert counts(info[b]) == B_COUNTS[b - 1], f"batch {b}: {info[b]}"


# ---------------------------------------------------------------------------
# c. delay-chain shapes
# ---------------------------------------------------------------------------
C_BATCHES, C_FRAGS = 8, 10
C_RAMP = (2, PAN, fix(-0.7), 0, (30 * 64) << 8)
# taps in ms (a fragment is 4/3 ms); the rounds k_bus_fbdchain cuts the batch of 10 fragments into are of
# min(shortest tap, 131072 - longest tap) / 64 whole fragments: 3, 4, 1 and 7 - none divides 10
C_TAPS = {
    "G1": [(4.2, 5.0, 6.3)],
    "G3": [(5.5, 7.0, 9.0), (6.0, 8.0, 11.0), (5.4, 12.0, 20.0)],
    "G3a": [(2.1, 3.0, 4.0), (2.5, 2.2, 5.0), (3.3, 2.9, 2.05)],
    "G4": [(9.5, 10.0, 12.5), (14.0, 9.9, 11.0), (10.1, 13.0, 16.0), (12.0, 18.0, 9.7)],
    "G5": [(3.0, 4.0, 5.0), (3.5, 4.5, 5.5), (4.0, 5.0, 6.0), (4.5, 5.5, 6.5), (5.0, 6.0, 7.0)],
}
C_ROUNDS = {"G1": 3, "G3": 4, "G3a": 1, "G4": 7}
C_GAINS = (0.4, 0.3, 0.35)
# Bus owners: root, N, R (drivers); G1, G3, G3a, G4 (one, three, three and four delays: the delay kernel); G5 (five
# delays: the host refuses the class).  R's pan is written in front of batch 2 and is within the host's bound while a
# batch begins before t + 1920 + 256: batches 3, 4, 5 (t + 640, 1253, 1893; batch 6 at t + 2533).  A tap of G3 is
# written below one fragment in front of batch 4 (a record, then the general kernel by class) and back above in front of
# batch 6 (a record; from batch 7 on the delay kernel again).
C_COUNTS = [(3, 0, 0, 4, 1), (2, 0, 0, 4, 2), (3, 1, 0, 4, 1), (3, 1, 0, 3, 2), (3, 1, 0, 3, 2), (3, 0, 0, 3, 2), (3, 0, 0, 4, 1)]


def c_script(be, mid_add=True, info=None):
    """Root -> G1 (one delay) -> bus group N; G3; G3a (three delays, the middle one adding); G5; bus group R -> G4.
    Four osc-pan voices in each of the seven groups.  A driver inside a delay chain's bus and a delay chain inside a
    ramping driver's: each depth's kernels must have run before the depth above reads its bus."""
    sc = synth.Scene(be, nwaves=4)
    sc.root()
    g = {}
    g["G1"] = sc.add_group(fb=C_TAPS["G1"], gains=C_GAINS, delays=1)
    g["N"] = sc.add_bus_group(parent=g["G1"])
    g["G3"] = sc.add_group(fb=C_TAPS["G3"], gains=C_GAINS, delays=3)
    g["G3a"] = sc.add_group(fb=C_TAPS["G3a"], gains=C_GAINS, delays=3, mid_add=mid_add)
    g["G5"] = sc.add_group(fb=C_TAPS["G5"], gains=C_GAINS, delays=5)
    g["R"] = sc.add_bus_group()
    g["G4"] = sc.add_group(fb=C_TAPS["G4"], gains=C_GAINS, delays=4, parent=g["R"])
    for name in ("G1", "N", "G3", "G3a", "G5", "R", "G4"):
        sc.add_voices(4, chain="osc-pan", group=g[name], total=32)
    before = {
        C_RAMP[0]: lambda: be.unit_write(g["R"]["units"][1], *C_RAMP[1:]),
        4: lambda: be.unit_write(g["G3"]["units"][2], 1, fix(0.9)),         # 43 frames
        6: lambda: be.unit_write(g["G3"]["units"][2], 1, fix(8.0)),
    }
    return run_script(be, sc, frag_plan(C_BATCHES, C_FRAGS, short=(3, 4)), before=before, info=info)


def test_delay_shapes_script_does_what_it_is_built_for(oracle_memo):
    for name, rf in C_ROUNDS.items():
        frames = [int(fix(ms) * 48000 / 65536000) for taps in C_TAPS[name] for ms in taps]
        assert all(64 <= t <= BUFSIZE - 64 for t in frames)
        assert min(min(frames), BUFSIZE - max(frames)) // 64 == rf
        assert rf == 1 or C_FRAGS % rf != 0
    assert int(fix(0.9) * 48000 / 65536000) == 43 and int(fix(8.0) * 48000 / 65536000) == 384
    plan = frag_plan(C_BATCHES, C_FRAGS, short=(3, 4))
    assert [bound_ramping(plan, [C_RAMP], b) for b in range(1, C_BATCHES)] == [row[1] == 1 for row in C_COUNTS]
    # the adding middle delay is heard
    want = oracle_memo("c", c_script)
    plain = oracle_memo("c-plain", lambda be: c_script(be, mid_add=False))
    assert all(w.any() for w in want)
    assert first_diff(np.concatenate(want, axis=1), np.concatenate(plain, axis=1)) is not None


@pytest.mark.gpu
def test_delay_chains_of_one_to_five_units_match_oracle(oracle_memo):
    """k_bus_fbdchain with nd = 1, 3 and 4 (FBC_MAXD), a middle delay in adding mode, rounds of 1, 3, 4 and 7 fragments
    in a batch of 10 with a fragment of 37 frames; five delays are the general kernel's; a tap rewritten below a fragment
    and back moves a chain to the general kernel and back."""
    want = oracle_memo("c", c_script)
    gpu = make_gpu(max_batch=C_FRAGS)
    info = []
    got = c_script(gpu, info=info)
    gpu.close()
    for b in range(C_BATCHES):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {info[b]}"
    for b in range(1, C_BATCHES):
        assert counts(info[b]) == C_COUNTS[b - 1], f"batch {b}: {info[b]}"
        assert info[b].consume == 0         # (G5: a bus the general kernel reads)


# ---------------------------------------------------------------------------
# d. tap edges
# ---------------------------------------------------------------------------
# raw register value -> frames at 48 kHz (value * samplerate / 65536000, truncated) -> the delay kernel?
D_EDGES = [(87382, 64, True), (87381, 63, False), (178869590, BUFSIZE - 64, True), (178870955, BUFSIZE - 63, False)]
# One group per accepted value with the value in all three positions - the first delay's fb and r tap, the second delay's
# l tap: the kernel reads every one of them at the edge - and one group per refused value and position: any one tap out
# of range must cost the chain its class, whichever tap it is.
D_GROUPS = [(v, fr, fast, pos) for v, fr, fast in D_EDGES for pos in ((("fb", "l", "r"),) if fast else (("fb",), ("l",), ("r",)))]
D_POS = {"fb": (0, 0), "l": (1, 1), "r": (0, 2)}        # position -> (delay of the chain, register)
D_FRAGS, D_BATCH = 2200, 256
D_OTHER = (fix(4.0), fix(6.5), fix(9.0))        # 192, 312 and 432 frames


def d_script(be, long_gain=True, info=None):
    """A group of two delays per entry of D_GROUPS, four osc-pan voices each; the taps that do not hold the edge value
    are a few fragments long.  2 200 fragments: 140 800 frames, so every delay line has wrapped and the taps of 131 008
    frames read what was written.  long_gain=False: the gains of the taps that hold the two long values are zero."""
    sc = synth.Scene(be, nwaves=4)
    sc.root()
    for value, frames, _fast, pos in D_GROUPS:
        g = sc.add_group()
        gain = fix(0.3) if long_gain or frames < 1000 else 0
        regs = [[D_OTHER[0], D_OTHER[1], D_OTHER[2]], [D_OTHER[1], D_OTHER[2], D_OTHER[0]]]
        for name in pos:
            regs[D_POS[name][0]][D_POS[name][1]] = None
        for d, row in zip(g["units"][1:], regs):
            for reg, v in enumerate(row):
                be.unit_write(d, reg, value if v is None else v)
                if v is None:
                    be.unit_write(d, 4 + reg, gain)
        sc.add_voices(4, chain="osc-pan", group=g, total=32)
    chunks = []
    for lo in range(0, D_FRAGS, D_BATCH):
        n = min(D_BATCH, D_FRAGS - lo)
        for _ in range(n):
            sc.walk(64)
        chunks.append(be.render(n * 64))
        if info is not None:
            info.append(be.last_batch_buses())
    return chunks


def test_tap_edges_script_does_what_it_is_built_for(oracle_memo):
    for value, frames, fast in D_EDGES:
        assert value * 48000 // 65536000 == frames
        assert fast == (64 <= frames <= BUFSIZE - 64)
        if fast:        # one fragment per round
            taps = [frames] + [v * 48000 // 65536000 for v in D_OTHER]
            assert min(min(taps), BUFSIZE - max(taps)) // 64 == 1
    assert D_FRAGS * 64 > BUFSIZE + 100 * 64
    # the long taps are heard in the last 100 fragments
    want = np.concatenate(oracle_memo("d", d_script), axis=1)
    mute = np.concatenate(oracle_memo("d-mute", lambda be: d_script(be, long_gain=False)), axis=1)
    assert first_diff(want[:, :BUFSIZE - 64], mute[:, :BUFSIZE - 64]) is None
    assert first_diff(want[:, -6400:], mute[:, -6400:]) is not None


@pytest.mark.gpu
def test_delay_taps_at_the_edges_of_the_delay_kernel_match_oracle(oracle_memo):
    """fbd_tap_ok: taps of exactly one fragment and of exactly the delay line less one fragment are the delay kernel's,
    in rounds of one fragment; one frame less / more in any one of the fb, l and r taps is the general kernel's."""
    want = oracle_memo("d", d_script)
    gpu = make_gpu(max_batch=D_BATCH)
    info = []
    got = d_script(gpu, info=info)
    gpu.close()
    for b in range(len(want)):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {info[b]}"
    # the root; the two accepted values; three groups for each of the two refused ones
    assert len(D_GROUPS) == 8
    for b in range(1, len(want)):
        assert counts(info[b]) == (1, 0, 0, 2, 6), f"batch {b}: {info[b]}"


# ---------------------------------------------------------------------------
# e. self-cleaning buses after an unsettled batch
# ---------------------------------------------------------------------------
E_BATCHES, E_FRAGS = 7, 8
E_RAMP = (2, VOL, fix(0.4), 0, (20 * 64) << 8)
# B's volume is written in front of batch 2 and within its bound while a batch begins before t + 1280 + 256: batches 3, 4
# (t + 512, t + 1024; batch 5 at t + 1536).  A's pan is written at once in front of batch 5.  Batches 1 .. 6:
E_COUNTS = [(4, 0, 0, 1, 0), (3, 0, 0, 1, 1), (4, 1, 0, 1, 0), (4, 1, 0, 1, 0), (3, 0, 0, 1, 1), (4, 0, 0, 1, 0)]
E_CONSUME = [3, 0, 3, 3, 0, 3]


def e_script(be, render=None, info=None):
    sc, u = bus_scene(be, root_leaves=False)
    before = {E_RAMP[0]: lambda: be.unit_write(u["B"][1], *E_RAMP[1:]),
              5: lambda: be.unit_write(u["A"][1], PAN, fix(0.25), 33, 0)}
    return run_script(be, sc, frag_plan(E_BATCHES, E_FRAGS), before=before, render=render, info=info)


def test_self_cleaning_script_does_what_it_is_built_for(oracle_memo):
    plan = frag_plan(E_BATCHES, E_FRAGS)
    assert [bound_ramping(plan, [E_RAMP], b) for b in range(1, E_BATCHES)] == [row[1] == 1 for row in E_COUNTS]
    # B begins the write's own batch and batches 3 and 4 unsettled: those two are the one-workgroup path's
    model = driver_model(plan, [E_RAMP])
    assert [b for b, f, running, clamp, ends in model if f == 0 and running] == [2, 3, 4]
    assert [c == 3 for c in E_CONSUME] == [row[4] == 0 for row in E_COUNTS]
    assert all(w.any() for w in oracle_memo("e", e_script))


@pytest.mark.gpu
def test_buses_are_left_clean_by_ramping_and_record_batches(oracle_memo):
    """Nothing but group drivers and a delay chain under the root: the bus kernels zero what they read and the root
    stores the master bus - also on k_bus_driver's one-workgroup path - unless a bus owner carries a record: then a
    memset clears the buses and the next self-cleaning batch must find them clean.  A bus left unzeroed is a fragment
    heard twice."""
    want = oracle_memo("e", e_script)
    gpu = make_gpu(max_batch=E_FRAGS)
    info = []
    got = e_script(gpu, info=info, render=lambda frames: render_async(gpu, frames))
    gpu.close()
    for b in range(E_BATCHES):
        assert first_diff(got[b], want[b]) is None, f"batch {b}: {info[b]}"
    for b in range(1, E_BATCHES):
        assert counts(info[b]) == E_COUNTS[b - 1], f"batch {b}: {info[b]}"
        assert info[b].consume == E_CONSUME[b - 1], f"batch {b}"
        assert info[b].master_direct == (E_CONSUME[b - 1] == 3), f"batch {b}"
