"""k_leaf_osc2tame / k_leaf_osc2pan under live graphs: the captured-graph and replay paths of the pair
(a2amd_sched.cpp upload(), a2amd_render.cpp run_phases() / a2amd_replay() / a2amd_osc2quiet_hold()).

tests/test_gpu_osc2tame_kernel.py changes the number of fragments from batch to batch, so none of its batches runs from
a graph.  Here the batches repeat: W is sixteen fragments of 64 frames, C9 and C3 are W with a 37-frame fragment at
index 9 / 3.  Every batch is compared with the oracle bit for bit, and per batch the tests assert
  - the change of a2amd_get_stats().launches: 0 is a batch that ran from a graph, above 0 one that was launched
    directly or captured,
  - a2amd_last_batch_osc2quiet(): launched and wavefronts (for a replayed batch: the capture's, see the header), and the
    change of taken_total - the wavefronts k_leaf_osc2tame took in that batch,
  - the change of a2amd_osc2_tame_voices().
The scenes, staging masks and the oracle cache are test_gpu_osc2tame_kernel.py's (40 voices, the pair forced with
A2AMD_DEBUG bit 20), except in case 6: 1 024 / 1 023 voices, no switch set, the shape pick_fast_shape() gives.

Which batch is launched, captured or replayed is worked out by _host_rule() below, the host's rule restated from the
sources - never from a run: a batch with records, or behind one, is uploaded in full (quiet_streak 0, graphs dropped);
an identical record-free batch adds to the streak; one cut differently keeps the graphs while the fragment count and
osc2_pair_wanted() stay the same; from quiet_streak >= 1 and 8 fragments on a batch runs from the graph of its
destination, capturing it first where there is none.  A synchronous render() reads back through one pinned buffer of the
library's own, so there is one graph; a2amd_osc2quiet_hold() drops the graphs and leaves the streak.  So behind a birth
batch B: W (uploaded), W (captured), W (replayed), ...  The cases spell the sequences out as well.

The tests without the gpu mark are the premises, on the oracle alone.

Negative checks, done once by hand (profiles/osc2_tame_graphs.md): upload() without the osc2_pair_wanted() term,
a2amd_osc2quiet_hold() without drop_graphs(), k_leaf_osc2tame's end phase a fragment early, k_leaf_osc2pan ignoring
taken[] - each fails cases below."""
import numpy as np
import pytest

from audiality2_amd import synth
from conftest import make_gpu, make_oracle
from test_gpu_launch_plan import launches
from test_gpu_osc2_lds_taps import MAXB, PHASES, _pitch
from test_gpu_osc2_tame import LENGTH
from test_gpu_osc2_voice_major import _assert_batches_equal
from test_gpu_osc2tame_kernel import _REF, GOOD, NV, WHO, _batches, _bits, _builder

W = [64] * 16
C9 = [37 if f == 9 else 64 for f in range(16)]
C3 = [37 if f == 3 else 64 for f in range(16)]
FORCED = [(4, 16), (32, 1)]         # 10 and 2 wavefronts of 40 voices: the state staged, the state written in place
TAME_MIN = 1024                     # A2D_OSC2TAME_MIN
ON = _bits(20)


class S:
    """One batch of a sequence.  rec: it carries records (a birth, a death); hold: a2amd_osc2quiet_hold() in front of it;
    pre(sc): run in front of its first fragment on either backend; n: the voices of the class when it is launched;
    left: wavefronts left to k_leaf_osc2pan where the pair runs (None: all of them - the batch the scene is born in);
    tame: voices given the tame bit, by either kernel (n unless given; not asserted of the first batch)"""

    def __init__(self, frags, rec=False, hold=None, pre=None, n=NV, left=0, tame=None):
        self.frags, self.rec, self.hold, self.pre, self.n, self.left = list(frags), rec, hold, pre, n, left
        self.tame = n if tame is None else tame


def _seq(*frags, **kw):
    """the batch the voices are born in - every one carries records, no wavefront is eligible - and the batches behind"""
    return [S(frags[0], rec=True, left=None, **kw)] + [S(f, **kw) for f in frags[1:]]


def _host_rule(steps, forced, off=False):
    """[(launched directly or captured, the pair launched)] per batch, by the rule of upload(), run_phases() and
    osc2_pair_wanted() as the module's text restates it"""
    out, streak, graph, prev, prev_rec, quiet, hold = [], 0, False, None, True, False, False
    for s in steps:
        if s.hold is not None:
            graph = graph and bool(s.hold) == hold
            hold = bool(s.hold)

        def wanted(frags):
            return (s.n >= TAME_MIN or forced) and not off and not hold and all(f == 64 for f in frags)
        if s.rec or prev_rec or not quiet:          # the full upload
            streak, graph, quiet = 0, False, not s.rec
        elif s.frags == prev or (len(s.frags) == len(prev) and wanted(s.frags) == wanted(prev)):
            streak += 1
        else:
            streak, graph = 0, False
        if streak >= 1 and len(s.frags) >= 8:
            direct, graph = not graph, True
        else:
            direct = True
        out.append((direct, wanted(s.frags)))
        prev, prev_rec = s.frags, s.rec
    return out


def _env(monkeypatch, shape, debug, **more):
    for name, v in (("A2AMD_VPW", shape and shape[0]), ("A2AMD_YSPLIT", shape and shape[1]), ("A2AMD_DEBUG", debug)):
        if v:
            monkeypatch.setenv(name, str(v))
        else:
            monkeypatch.delenv(name, raising=False)
    monkeypatch.delenv("A2AMD_NO_MOVING", raising=False)
    for k, v in more.items():
        monkeypatch.setenv(k, v)


def _walk(be, build, steps):
    """every fragment walked, a synchronous render per batch; on the product library the reports of every batch"""
    sc, outs, rows = build(be), [], []
    for s in steps:
        if s.hold is not None and be.prefix == "a2amd_":
            be.osc2quiet_hold(s.hold)
        if s.pre:
            s.pre(sc)
        for n in s.frags:
            sc.walk(n)
        before = launches(be) if be.prefix == "a2amd_" else 0
        outs.append(be.render(sum(s.frags)).copy())
        if be.prefix == "a2amd_":
            rows.append((launches(be) - before, be.last_batch_osc2quiet(), be.last_batch_osc2(), be.osc2_tame_voices()))
    be.close()
    return np.concatenate(outs, axis=1), rows


def _ref(oracle_lib, key, build, steps):
    key = ("graphs", key)
    if key not in _REF:
        _REF[key] = _walk(make_oracle(oracle_lib), build, steps)[0]
        _REF[key].setflags(write=False)
    return _REF[key]


def _check(rows, steps, want, shape=None):
    """want: [(directly, pair)] per batch.  Every batch is looked at; the list of what is wrong, batch by batch"""
    seen_taken = seen_tame = 0
    bad = []
    for b, ((dl, q, o, t), s, (direct, pair)) in enumerate(zip(rows, steps, want)):
        print(b, s.frags.index(37) if 37 in s.frags else "-", dl, q, o, t)
        # (ysplit as the launcher clamped it to the batch's chunks: more than one slice stages the state)
        if not (o.launched == 1 and o.voices == s.n and (shape is None or (o.vpw, o.ysplit > 1) == (shape[0], shape[1] > 1))):
            bad.append(f"batch {b}: k_leaf_osc2pan's launch is {o}, for {s.n} voices at {shape}")
        waves = -(-o.voices // max(o.vpw, 1))
        if (dl > 0) != direct:
            bad.append(f"batch {b}: {dl} launches, but it is to be " +
                       ("launched directly or captured" if direct else "replayed from a graph"))
        if (q.launched, q.wavefronts) != ((1, waves) if pair else (0, 0)):
            bad.append(f"batch {b}: {q}, but the pair is {'' if pair else 'not '}to be launched ({waves} wavefronts)")
        taken = 0 if not pair or s.left is None else waves - s.left
        if q.taken_total - seen_taken != taken:
            bad.append(f"batch {b}: {q.taken_total - seen_taken} wavefronts taken, not {taken}")
        if b and t - seen_tame != s.tame:
            bad.append(f"batch {b}: {t - seen_tame} voices given the tame bit, not {s.tame}")
        seen_taken, seen_tame = q.taken_total, t
    return bad


def _verdict(bad, got, want, plan):
    """the reports' mismatches and the audio's, together: a failure names every batch that is wrong, and says whether
    the audio stayed the oracle's"""
    try:
        _assert_batches_equal(got, want, plan)
    except pytest.fail.Exception as e:
        bad = bad + [str(e)]
    assert not bad, "\n".join(bad)


def _case(oracle_lib, monkeypatch, key, build, steps, shape, debug, spelled=None, **more):
    forced = bool(debug) and bool(int(debug) & (1 << 20))
    off = bool(debug) and bool(int(debug) & (1 << 19))
    want = _host_rule(steps, forced, off)
    if spelled is not None:       # the sequence as the case states it: "D" directly, "C" captured, "R" replayed; + with the pair
        assert [("R" not in w, "+" in w) for w in spelled.split()] == want, (spelled, want)
    _env(monkeypatch, shape, debug, **more)
    assert all(len(s.frags) <= MAXB for s in steps)
    got, rows = _walk(make_gpu(max_batch=MAXB), build, steps)
    _verdict(_check(rows, steps, want, shape), got, _ref(oracle_lib, key, build, steps), [s.frags for s in steps])
    return rows


# ---- 1. steady replay ----------------------------------------------------------------------------------------------------
STEADY = "D+ D+ C+ R+ R+ R+"


@pytest.mark.gpu
@pytest.mark.parametrize("bit17", [False, True])
@pytest.mark.parametrize("vpw,ysplit", FORCED + [(32, 16), (4, 1)])
def test_steady_replay(oracle_lib, monkeypatch, vpw, ysplit, bit17):
    """The birth batch and five identical W: uploaded, captured, and three times replayed.  From the second batch on
    every wavefront is taken and every voice tame, replayed or not; the replayed batches report the launch they were
    captured with.  With bit 17 no level is staged in LDS."""
    rows = _case(oracle_lib, monkeypatch, ("steady", 16), _builder(), _seq(*[W] * 6), (vpw, ysplit),
                 _bits(20, 17) if bit17 else ON, STEADY)
    assert [dl for dl, *_ in rows[3:]] == [0, 0, 0]
    assert all((q.launched, q.wavefronts) == (1, -(-NV // vpw)) for _, q, _, _ in rows[3:])


@pytest.mark.gpu
@pytest.mark.parametrize("vpw,ysplit", FORCED)
@pytest.mark.parametrize("nfrags", [8, 17])
def test_steady_replay_other_lengths(oracle_lib, monkeypatch, nfrags, vpw, ysplit):
    """8 fragments, the fewest a graph takes, and 17: a partial super-chunk behind a whole one"""
    _case(oracle_lib, monkeypatch, ("steady", nfrags), _builder(), _seq(*[[64] * nfrags] * 6), (vpw, ysplit), ON, STEADY)


# ---- 2., 3. the rule's answer flips under a live graph -------------------------------------------------------------------------
FLIP = [W, W, W, W, C9, C9, C9, C3, W, W, W, W]


@pytest.mark.gpu
@pytest.mark.parametrize("vpw,ysplit", FORCED)
def test_rule_flips_under_a_live_graph(oracle_lib, monkeypatch, vpw, ysplit):
    """W until replayed; the first C9 drops the graphs and is k_leaf_osc2pan's alone, launched directly, the later ones
    are captured and replayed without the pair; C3 - the same fragment count, the same answer - runs from C9's graph on
    its own fragment table; the first W behind it drops the graphs again and launches the pair, the later ones are
    captured and replayed with it."""
    _case(oracle_lib, monkeypatch, "flip", _builder(), _seq(*FLIP), (vpw, ysplit), ON,
          "D+ D+ C+ R+  D C R  R  D+ C+ R+ R+")


@pytest.mark.gpu
@pytest.mark.parametrize("vpw,ysplit", FORCED)
@pytest.mark.parametrize("debug", [None, _bits(19, 20)])
def test_graphs_kept_where_the_rule_says_no_throughout(oracle_lib, monkeypatch, debug, vpw, ysplit):
    """"... and only then": 40 voices without bit 20, and bit 19 - the pair is never launched, and the graph captured
    over W serves C9, C3 and W again, as before the pair existed"""
    _case(oracle_lib, monkeypatch, "flip", _builder(), _seq(*FLIP), (vpw, ysplit), debug, "D D C R  R R R  R  R R R R")


# ---- 4. hold under a live graph ----------------------------------------------------------------------------------------------
def _held(first):
    steps = _seq(*[W] * 9)
    if first == "pair":
        for b, h in ((4, 1), (6, 1), (7, 0)):
            steps[b].hold = h
        return steps, "D+ D+ C+ R+  C R  R  C+ R+"
    for b, h in ((0, 1), (4, 1), (5, 0), (7, 1)):
        steps[b].hold = h
    return steps, "D D C R  R  C+ R+  C R"


@pytest.mark.gpu
@pytest.mark.parametrize("vpw,ysplit", FORCED)
@pytest.mark.parametrize("first", ["pair", "held"])
def test_hold_under_a_live_graph(oracle_lib, monkeypatch, first, vpw, ysplit):
    """W until replayed with the pair; hold(1): the graph is dropped, the next W goes out anew with k_leaf_osc2pan alone
    (the streak stands, so it is captured as it goes) and the ones behind it are replayed so; hold(1) again changes
    nothing; hold(0): the next W goes out anew with the pair, and is replayed with it.  And in the other order, held
    from the start."""
    steps, spelled = _held(first)
    _case(oracle_lib, monkeypatch, ("steady", 16, 9), _builder(), steps, (vpw, ysplit), ON, spelled)


# ---- 5. a2amd_replay() ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("vpw,ysplit", FORCED)
@pytest.mark.parametrize("held", [False, True])
def test_replay_entry_point(oracle_lib, monkeypatch, held, vpw, ysplit):
    """The birth batch, W, W kept, a2amd_replay(9) - one graph of eight steps and one of one - the kept batch once more,
    heard, and a walked W: batches 0, 1, 2, 12 and 13 of the oracle's fourteen.  Each of the nine unheard steps takes
    every wavefront; with the hold set in front of the kept render none does, and the audio is the same."""
    _env(monkeypatch, (vpw, ysplit), ON)
    want = _ref(oracle_lib, ("steady", 16, 14), _builder(), _seq(*[W] * 14))
    want = _batches(want, [W] * 14)
    be = make_gpu(max_batch=MAXB)
    sc, waves, marks = _builder()(be), -(-NV // vpw), []

    def walked():
        for n in W:
            sc.walk(n)
        return sum(W)

    def mark():
        marks.append((be.last_batch_osc2quiet(), be.osc2_tame_voices()))
        print(marks[-1])
    heard = {0: be.render(walked()).copy()}
    mark()
    heard[1] = be.render(walked()).copy()
    mark()
    if held:
        be.osc2quiet_hold(1)
    walked()
    heard[2] = be.render_kept(sum(W)).copy()
    mark()
    be.replay(9)
    mark()
    heard[12] = be.render(sum(W)).copy()
    mark()
    heard[13] = be.render(walked()).copy()
    mark()
    be.close()
    for b, x in heard.items():
        assert np.array_equal(x, want[b]), f"batch {b} differs from the oracle's"
    taken = [q.taken_total for q, _ in marks]
    tame = [t for _, t in marks]
    each = 0 if held else waves
    assert [b - a for a, b in zip(taken, taken[1:])] == [waves, each, 9 * each, each, each], (taken, waves)
    assert [b - a for a, b in zip(tame, tame[1:])] == [NV, NV, 9 * NV, NV, NV], tame
    assert [(q.launched, q.wavefronts) for q, _ in marks] == [(1, waves)] * 2 + [(0, 0) if held else (1, waves)] * 4, marks


# ---- 6. the rule's own threshold, the shape production takes -----------------------------------------------------------------
SHORT_FLIP = [W, W, W, W, C9, C9, C9, C3, W, W, W]


def _many(n):
    return _seq(*SHORT_FLIP, n=n)


@pytest.mark.gpu
def test_threshold_met(oracle_lib, monkeypatch):
    """1 024 voices, no switch: the pair is launched by the rule itself, over voices / vpw wavefronts of the shape
    pick_fast_shape() gives, takes them all from the second batch on, replays from a graph and flips as in case 2"""
    _case(oracle_lib, monkeypatch, ("many", TAME_MIN), _builder(n=TAME_MIN), _many(TAME_MIN), None, None,
          "D+ D+ C+ R+  D C R  R  D+ C+ R+")


@pytest.mark.gpu
def test_threshold_missed_by_one(oracle_lib, monkeypatch):
    """1 023 voices: never launched, and the graph is kept across W, C9, C3 and W"""
    n = TAME_MIN - 1
    _case(oracle_lib, monkeypatch, ("many", n), _builder(n=n), _many(n), None, None, "D D C R  R R R  R  R R R")


def _born(sc):
    k = len(sc.units)
    assert k == TAME_MIN - 1
    sc.units.append(sc.voice(GOOD[k % len(GOOD)][0], (PHASES[k % 8], PHASES[(k + 3) % 8]), k, None, total=TAME_MIN))


def _dies(sc):
    for u in sc.leaves.pop(1):
        sc.be.unit_deinit(u)


def _crossing():
    n = TAME_MIN - 1
    return _seq(W, W, W, W, n=n) + [S(W, rec=True, pre=_born, n=n + 1, left=1, tame=n)] + [S(W, n=n + 1) for _ in range(3)] + \
        [S(W, rec=True, pre=_dies, n=n + 1, left=1, tame=n)] + [S(W, n=n) for _ in range(3)]


@pytest.mark.gpu
def test_threshold_crossed_in_one_context(oracle_lib, monkeypatch):
    """1 023 voices until replayed (no pair); a birth makes them 1 024: the birth batch launches the pair, which takes
    every wavefront but the newborn's, the steps behind it take all and reach a graph again.  A voice dies: it is
    listed to the end of that batch, its wavefront not taken; the step behind it has 1 023 voices and launches
    k_leaf_osc2pan alone."""
    _case(oracle_lib, monkeypatch, "crossing", _builder(n=TAME_MIN - 1), _crossing(), None, None,
          "D D C R  D+  D+ C+ R+  D+  D C R")


# ---- 7. a glide that ends --------------------------------------------------------------------------------------------------------
RAMP = 2900         # frames: the ramp ends inside the third batch (frames 2 048 .. 3 071), 172 frames before its end
BATCH = sum(W)


def _glide(what):
    def after(sc):
        osc, _, pan = sc.units[WHO]
        if what == "amplitude":
            sc.be.unit_write(osc, 2, 1200, 0, RAMP << 8)
        elif what == "pitch":
            name, level, where = GOOD[WHO % len(GOOD)][0][0]
            sc.be.unit_write(osc, 1, _pitch(sc.tab, sc.base, LENGTH[name], level, where) - 3000, 0, RAMP << 8)
        else:
            sc.be.unit_write(pan, 1, synth.fix(0.9), 0, RAMP << 8)
    return _builder(after=after)


def _glide_batches(no_moving):
    """(the first batch in which the voice's wavefront is the pair's, the batch that cleans the host's list of moving
    voices).  The write is made in front of the first fragment: the ramp lasts (start + dur) >> 8 = RAMP frames and
    settles in the window after the one it ends in; the host holds the voice to walk time + 64 + RAMP + 192
    (moving_until) - it carries the stand-in record until the first batch that begins at or after that, unless
    A2AMD_NO_MOVING leaves it to the kernels, which take it from the first batch at whose start the rampers are at rest.
    The list is cleaned by the full upload of the first batch that begins at or after moving_until either way: the batch
    behind that is the first on the quiet path, the second its graph's capture, the third its replay."""
    arrived = (RAMP // 64 + 2) * 64
    until = 0 + 64 + RAMP + 192
    cleaned = -(-until // BATCH)
    return (-(-arrived // BATCH) if no_moving else cleaned), cleaned


@pytest.mark.gpu
@pytest.mark.parametrize("vpw,ysplit", FORCED)
@pytest.mark.parametrize("no_moving", [False, True])
@pytest.mark.parametrize("what", ["amplitude", "pitch", "pan"])
def test_glide_that_ends(oracle_lib, monkeypatch, what, no_moving, vpw, ysplit):
    """Voice WHO glides for 2 900 frames: its wavefront is k_leaf_osc2pan's while it is unsettled (or carries the
    stand-in record), the pair's from the batch the two rules give, and is then seen taken inside a replayed graph."""
    first, cleaned = _glide_batches(no_moving)
    assert (first, cleaned) == ((3, 4) if no_moving else (4, 4)) and RAMP < 3 * BATCH
    steps = _seq(*[W] * (cleaned + 4))
    for b, s in enumerate(steps):
        if b < first:
            s.left, s.tame = (None if b == 0 else 1), NV - 1
    want = [(b < cleaned + 2, True) for b in range(len(steps))]
    _env(monkeypatch, (vpw, ysplit), ON, **({"A2AMD_NO_MOVING": "1"} if no_moving else {}))
    build = _glide(what)
    got, rows = _walk(make_gpu(max_batch=MAXB), build, steps)
    _verdict(_check(rows, steps, want, (vpw, ysplit)), got, _ref(oracle_lib, ("glide", what), build, steps),
             [s.frags for s in steps])
    waves = -(-NV // vpw)
    assert [(dl, q.taken_total - p.taken_total) for (dl, q, _, _), (_, p, _, _) in zip(rows[-2:], rows[-3:])] == [(0, waves)] * 2


# ---- the premises: the oracle alone ------------------------------------------------------------------------------------------
def _sounds(x, plan):
    for b, y in enumerate(_batches(x, plan)):
        assert np.abs(y[0]).max() > 1000 and np.abs(y[1]).max() > 1000, b


@pytest.mark.parametrize("nfrags", [8, 16, 17])
def test_premise_steady_scene_sounds_in_every_batch(oracle_lib, nfrags):
    steps = _seq(*[[64] * nfrags] * 6)
    _sounds(_ref(oracle_lib, ("steady", nfrags), _builder(), steps), [s.frags for s in steps])


@pytest.mark.parametrize("n", [TAME_MIN, TAME_MIN - 1])
def test_premise_large_scenes_sound_in_every_batch(oracle_lib, n):
    _sounds(_ref(oracle_lib, ("many", n), _builder(n=n), _many(n)), SHORT_FLIP)


def test_premise_crossing_scene_sounds_in_every_batch(oracle_lib):
    steps = _crossing()
    _sounds(_ref(oracle_lib, "crossing", _builder(n=TAME_MIN - 1), steps), [s.frags for s in steps])


def test_premise_cut_batches_differ_behind_the_cut(oracle_lib):
    """case 2: every batch sounds, and the C9 batch in front of C3 and the C3 batch differ in the frames behind C3's
    cut - were C3 rendered on C9's fragment table, it would be heard"""
    x = _ref(oracle_lib, "flip", _builder(), _seq(*FLIP))
    _sounds(x, FLIP)
    b = _batches(x, FLIP)
    assert FLIP[6] == C9 and FLIP[7] == C3
    cut = 3 * 64 + 37
    assert np.array_equal(b[6].shape, b[7].shape) and not np.array_equal(b[6][:, cut:], b[7][:, cut:])
    assert (b[6][:, cut:] != b[7][:, cut:]).any(axis=0).mean() > 0.5


@pytest.mark.parametrize("what", ["amplitude", "pitch", "pan"])
def test_premise_glide_is_heard_to_its_end_and_after(oracle_lib, what):
    """case 7: the glide changes the mix against the scene at rest from the batch it starts in, while it lasts and in
    the batches after its end - the hand-over batch among them, whichever of the two rules gives it"""
    steps = _seq(*[W] * 8)
    plan = [s.frags for s in steps]
    base = _batches(_ref(oracle_lib, ("steady", 16, 8), _builder(), steps), plan)
    with_it = _ref(oracle_lib, ("glide", what), _glide(what), steps)
    _sounds(with_it, plan)
    for b, (x, y) in enumerate(zip(base, _batches(with_it, plan))):
        assert (x != y).any(axis=0).mean() > 0.5, (what, b)
    assert {_glide_batches(True)[0], _glide_batches(False)[0]} == {3, 4}
