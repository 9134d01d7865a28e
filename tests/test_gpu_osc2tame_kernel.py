"""k_leaf_osc2tame in front of k_leaf_osc2pan (a2amd_osc2tame.hip; include/a2amd_osc2tame_kernel.h).

Whole wavefronts of settled, tame `wtosc; wtosc; panmix` voices on power-of-two levels are rendered by a kernel of
their own in batches of whole fragments; every other wavefront, and every batch with a cut fragment, stays with
k_leaf_osc2pan.  Every case renders at least three consecutive batches through the C ABI and compares every batch with the
oracle bit for bit - the phases a batch parks are what the next batch's audio starts from - and asserts per batch, from
a2amd_last_batch_osc2quiet() and a2amd_osc2_tame_voices(), whether the pair was launched, how many wavefronts the new
kernel took and how many voices had the tame bit.  The scenes are small (40 voices), so every case that wants the pair
sets A2AMD_DEBUG bit 20; the waves, pitches and start phases are those of tests/test_gpu_osc2_lds_taps.py and
tests/test_gpu_osc2_tame.py, so all four staging masks occur among the eligible voices.

The first batch of every case is the one in which the voices are born: they carry records, no wavefront is eligible, and
the new kernel - launched all the same - takes none.

The tests without the gpu mark are the premises, on the oracle alone: every scene sounds in every batch, and the voice
that makes a wavefront ineligible is audible from the batch in which it does.

Negative checks, done once by hand (profiles/osc2_tame_kernel.md): the new kernel taking a wavefront that has an untame
voice, the end phase taken one fragment early, and taken[] never read by k_leaf_osc2pan - each fails cases below."""
import numpy as np
import pytest

from audiality2_amd import synth
from conftest import make_gpu, make_oracle
from test_gpu_osc2_lds_taps import MAXB, PHASES, _assert_masks, _pitch
from test_gpu_osc2_tame import LENGTH, _Scene
from test_gpu_osc2_voice_major import _assert_batches_equal

_REF = {}
NV = 40


def _bits(*n):
    return str(sum(1 << k for k in n))


def _ref(oracle_lib, key, build, plan, between=None):
    if key not in _REF:
        _REF[key] = _run(make_oracle(oracle_lib), build, plan, between)[0]
        _REF[key].setflags(write=False)
    return _REF[key]


# ---- scenes --------------------------------------------------------------------------------------------------------
NAMES = ["A32", "A64", "B64", "A96", "A128", "A256", "W+"]
GOOD = [    # (oscillators, staging mask): tame, power-of-two levels
    ((("A128", 1, "lo"), ("B64", 0, "hi")), 3),
    ((("A128", 0, "hi"), ("A256", 1, "lo")), 1),
    ((("A256", 0, "hi"), ("B64", 0, 0.45)), 2),
    ((("A256", 0, "hi"), ("A256", 0, 0.3)), 0),
    ((("A32", 0, "hi"), ("A64", 1, "lo")), 3),
]
WRAPS = ((("W+", 0, 1.1), ("A64", 0, 0.9)), 3)      # a level with a wrapping product: not tame
ODD = ((("A96", 0, "hi"), ("A128", 1, "hi")), 2)    # a level of 96 entries: tame, no power of two
WHO = 21    # the voice that is made ineligible, by its place in the scene


def _builder(special=None, buses=3, after=None, n=NV):
    def build(be):
        sc = _Scene(be, NAMES)
        sc.root()
        if buses == 3:
            bs = [sc.add_group(preset="fmtest4"), sc.add_bus_group(), None]
        else:       # two delay groups, a mono group, the root
            bs = [sc.add_group(preset="fmtest4"), sc.add_group(), sc.add_mono_group(pan=0.25), None]
        sc.units, sc.want_masks = [], []
        for k in range(n):
            spec, mask = special if (special and k == WHO) else GOOD[k % len(GOOD)]
            sc.units.append(sc.voice(spec, (PHASES[k % 8], PHASES[(k + 3) % 8]), k, bs[k % len(bs)], total=n))
            sc.want_masks.append(mask)
        if be.prefix == "a2amd_":
            _assert_masks(be, sc, sc.want_masks)
            assert [be.osc2_tame_rule(*t) for t in sc.tame] == [0 if (special is WRAPS and k == WHO) else 1 for k in range(n)]
        if after:
            after(sc)
        return sc
    return build


def _glide_pitch(sc):
    name, level, where = GOOD[WHO % len(GOOD)][0][0]
    sc.be.unit_write(sc.units[WHO][0], 1, _pitch(sc.tab, sc.base, LENGTH[name], level, where) - 3000, 0, 30000 << 8)


def _glide_pan(sc):
    sc.be.unit_write(sc.units[WHO][2], 1, synth.fix(0.9), 0, 30000 << 8)


def _write_in_batch_2(sc, b, f):
    if (b, f) == (2, 1):
        sc.be.unit_write(sc.units[WHO][2], 1, synth.fix(-0.6))      # a pan jump: a record in this batch, at rest after it


# ---- the walk and what is asserted of it ---------------------------------------------------------------------------------
def _run(be, build, plan, between=None, hold=None):
    sc, outs, infos = build(be), [], []
    for b, frags in enumerate(plan):
        if hold is not None and be.prefix == "a2amd_":
            be.osc2quiet_hold(hold[b])
        for f, n in enumerate(frags):
            if between:
                between(sc, b, f)
            sc.walk(n)
        outs.append(be.render(sum(frags)).copy())
        if be.prefix == "a2amd_":
            infos.append((be.last_batch_osc2quiet(), be.last_batch_osc2(), be.osc2_tame_voices()))
    be.close()
    return np.concatenate(outs, axis=1), infos


def _case(oracle_lib, monkeypatch, key, build, plan, vpw, ysplit, debug, launched, taken, tame, between=None, hold=None,
          **more):
    """launched[b]: was the pair launched in batch b; taken[b]: "all", "all-1" or 0 wavefronts taken by the new kernel;
    tame[b]: voices given the tame bit, by either kernel (not asserted of the first batch, as in test_gpu_osc2_tame.py)"""
    monkeypatch.setenv("A2AMD_VPW", str(vpw))
    monkeypatch.setenv("A2AMD_YSPLIT", str(ysplit))
    if debug:
        monkeypatch.setenv("A2AMD_DEBUG", debug)
    else:
        monkeypatch.delenv("A2AMD_DEBUG", raising=False)
    for k, v in more.items():
        monkeypatch.setenv(k, v)
    assert len(plan) >= 3 and all(len(f) <= MAXB for f in plan)
    got, infos = _run(make_gpu(max_batch=MAXB), build, plan, between, hold)
    seen_taken = seen_tame = 0
    for b, (q, o, t) in enumerate(infos):
        print(b, q, o, t)
        waves = -(-o.voices // vpw)
        assert (o.launched, o.vpw) == (1, vpw) and 8 <= o.voices <= 96, (b, o)
        assert (q.launched, q.wavefronts) == ((1, waves) if launched[b] else (0, 0)), (b, q, o)
        want = {"all": waves, "all-1": waves - 1, 0: 0}[taken[b]]
        assert q.taken_total - seen_taken == want, (b, q, seen_taken, want)
        assert b == 0 or t - seen_tame == tame[b], (b, t, seen_tame, tame[b])
        seen_taken, seen_tame = q.taken_total, t
    _assert_batches_equal(got, _ref(oracle_lib, key, build, plan, between), plan)
    return got


# batches of 1, 3, 4, 5, 16, 17 and 33 fragments behind the first: partial chunks, partial super-chunks, a slice longer
# than a super-chunk; a last batch behind each so that what the one before parked is heard
PLANS = {"a": [[64] * 4, [64] * 5, [64] * 17, [64] * 33, [64] * 4],
         "b": [[64] * 5, [64] * 1, [64] * 3, [64] * 4, [64] * 16, [64] * 5]}
SHAPES = [(4, 1), (4, 16), (32, 1), (32, 16)]
ON = _bits(20)


def _all(plan, first=0):
    return [first] + ["all"] * (len(plan) - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("bit17", [False, True])
@pytest.mark.parametrize("vpw,ysplit", SHAPES)
@pytest.mark.parametrize("plan", sorted(PLANS))
def test_every_wavefront_eligible(oracle_lib, monkeypatch, plan, vpw, ysplit, bit17):
    """40 voices with the staging masks 0, 1, 2 and 3 on three buses: every wavefront is taken in every batch behind the
    first; with bit 17 no level is staged and every tap is a gather."""
    p = PLANS[plan]
    _case(oracle_lib, monkeypatch, ("good", plan), _builder(), p, vpw, ysplit, _bits(20, 17) if bit17 else ON,
          [1] * len(p), _all(p), [NV] * len(p))


CAUSES = {
    # name: (scene, between, voices with the tame bit per batch of plan "a", wavefronts taken per batch, environment)
    "wraps": (_builder(WRAPS), None, [NV - 1] * 5, [0] + ["all-1"] * 4, {}),
    "odd-size": (_builder(ODD), None, [NV] * 5, [0] + ["all-1"] * 4, {}),
    "pitch-glide": (_builder(after=_glide_pitch), None, [NV - 1] * 5, [0] + ["all-1"] * 4, {"A2AMD_NO_MOVING": "1"}),
    "pan-glide": (_builder(after=_glide_pan), None, [NV - 1] * 5, [0] + ["all-1"] * 4, {"A2AMD_NO_MOVING": "1"}),
    "pan-glide-record": (_builder(after=_glide_pan), None, [NV - 1] * 5, [0] + ["all-1"] * 4, {}),
    "written": (_builder(), _write_in_batch_2, [NV, NV, NV - 1, NV, NV], [0, "all", "all-1", "all", "all"], {}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("vpw,ysplit", [(4, 16), (32, 1), (32, 16)])
@pytest.mark.parametrize("cause", sorted(CAUSES))
def test_one_ineligible_voice(oracle_lib, monkeypatch, cause, vpw, ysplit):
    """One voice of one wavefront is not the new kernel's - a level that wraps, a level of 96 entries, a gliding pitch, a
    gliding pan (kept quiet by A2AMD_NO_MOVING, and with the stand-in record a gliding voice gets otherwise), a control
    write inside the third batch: that wavefront is rendered by k_leaf_osc2pan, the others stay taken; the written voice's
    wavefront is taken again in the batch after."""
    build, between, tame, taken, more = CAUSES[cause]
    p = PLANS["a"]
    _case(oracle_lib, monkeypatch, ("cause", cause), build, p, vpw, ysplit, ON, [1] * len(p), taken, tame, between, **more)


@pytest.mark.gpu
@pytest.mark.parametrize("vpw,ysplit", [(4, 16), (32, 1)])
def test_buses_within_a_wavefront(oracle_lib, monkeypatch, vpw, ysplit):
    """Voices of one wavefront on two delay groups and the root: the tile is flushed where the bus changes.  Every fourth
    voice mixes into a mono group: a one-channel bus is not this launch class's (those ten are the general kernel's), and
    the class's list is the other thirty."""
    p = PLANS["a"]
    _case(oracle_lib, monkeypatch, "buses", _builder(buses=4), p, vpw, ysplit, ON, [1] * len(p), _all(p),
          [NV - NV // 4] * len(p))


CUT = [37 if f == 9 else 64 for f in range(17)]


@pytest.mark.gpu
@pytest.mark.parametrize("vpw,ysplit", [(4, 16), (32, 1)])
def test_cut_window_then_whole_batch(oracle_lib, monkeypatch, vpw, ysplit):
    """A batch with a 37-frame fragment is k_leaf_osc2pan's alone, the whole batch behind it the pair's, twice over: the
    state goes from one kernel to the other and back"""
    p = [[64] * 5, CUT, [64] * 17, CUT[::-1], [64] * 16, [64] * 4]
    _case(oracle_lib, monkeypatch, "cut", _builder(), p, vpw, ysplit, ON, [1, 0, 1, 0, 1, 1], [0, 0, "all", 0, "all", "all"],
          [NV] * len(p))


@pytest.mark.gpu
@pytest.mark.parametrize("vpw,ysplit", [(4, 16), (32, 1)])
@pytest.mark.parametrize("first", ["pair", "general"])
def test_hold_toggled_between_batches(oracle_lib, monkeypatch, first, vpw, ysplit):
    """What bit 19 does, switched per batch inside one context (a2amd_osc2quiet_hold): k_leaf_osc2pan alone and the pair in
    turn, in both orders"""
    p = [[64] * 5, [64] * 17, [64] * 5, [64] * 33, [64] * 3, [64] * 4]
    hold = [b % 2 == (1 if first == "general" else 0) for b in range(len(p))]
    _case(oracle_lib, monkeypatch, "hold", _builder(), p, vpw, ysplit, ON, [0 if h else 1 for h in hold],
          [0 if h or b == 0 else "all" for b, h in enumerate(hold)], [NV] * len(p), hold=hold)


@pytest.mark.gpu
@pytest.mark.parametrize("debug,tame", [(None, NV), (_bits(19, 20), NV), (str(16 + (1 << 20)), NV), (_bits(18, 20), 0)])
def test_not_launched(oracle_lib, monkeypatch, debug, tame):
    """Below A2D_OSC2TAME_MIN voices without bit 20, under bit 19, and where the walk it holds is switched off (the
    switch called bit 16, whose value is 16, and bit 18): k_leaf_osc2pan alone, as before"""
    p = PLANS["a"]
    _case(oracle_lib, monkeypatch, ("good", "a"), _builder(), p, 32, 16, debug, [0] * len(p), [0] * len(p), [tame] * len(p))


# ---- the premises: the oracle alone ----------------------------------------------------------------------------------------
def _batches(x, plan):
    starts = [0] + list(np.cumsum([sum(f) for f in plan]))
    return [x[:, a:b].astype(np.int64) for a, b in zip(starts, starts[1:])]


@pytest.mark.parametrize("buses", [3, 4])
def test_premise_every_scene_sounds_in_every_batch(oracle_lib, buses):
    p = PLANS["a"]
    ref = _ref(oracle_lib, ("good", "a") if buses == 3 else "buses", _builder(buses=buses), p)
    for b, x in enumerate(_batches(ref, p)):
        assert np.abs(x[0]).max() > 1000 and np.abs(x[1]).max() > 1000, b


@pytest.mark.parametrize("cause", sorted(CAUSES))
def test_premise_the_ineligible_voice_is_heard(oracle_lib, cause):
    """Each cause changes the mix against the scene of eligible voices from the batch in which it acts (a glide or another
    wave: the first; the write: the third) and not before"""
    build, between, _, _, _ = CAUSES[cause]
    p = PLANS["a"]
    base = _batches(_ref(oracle_lib, ("good", "a"), _builder(), p), p)
    with_it = _batches(_ref(oracle_lib, ("cause", cause), build, p, between), p)
    since = 2 if cause == "written" else 0
    for b, (x, y) in enumerate(zip(base, with_it)):
        assert np.array_equal(x, y) == (b < since), (cause, b)
