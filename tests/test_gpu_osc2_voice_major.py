"""k_leaf_osc2pan's two walks of its settled voices (a2amd_fast.hip; include/a2amd_osc2.h).

A wavefront renders its voices over one time slice of the batch in super-chunks of at most 16 fragments.  A super-chunk
of whole 64-frame fragments is walked voice by voice - a voice's constants fetched once, its phases carried from chunk
to chunk, the bus sums of the 16 fragments in LDS; one that holds a shorter fragment, and every one under A2AMD_DEBUG
bit 16, is walked chunk by chunk with the sums in registers.  Both must render what the reference renders: every case
renders at least three consecutive batches through the C ABI, compares every batch's master bus with the oracle bit for
bit - a phase that was carried, wrapped or parked wrongly shows in the same or in the next batch - and asserts from
a2amd_last_batch_osc2() which walk every super-chunk took, against the rule restated here.

The unit state itself has no reader in the C ABI: "equal state" is what the following batches' audio says.

Negative checks, done once by hand against this file (see the commit that added it): an end phase taken from the last
computed row of a partial last chunk instead of from the last real fragment, and a flush_tile() that does not clear
the tile."""
import numpy as np
import pytest

from audiality2_amd import synth
from conftest import make_gpu, make_oracle

pytestmark = pytest.mark.gpu

FCH, SCH = 4, 16    # fragments per chunk and per super-chunk (csrc/a2amd_device.h: A2D_OSC2_FCH, A2D_OSC2_SCH)
MAXB = 40
_REF = {}           # the oracle's render of a scene and plan, made once and shared by the shape cases (read only)


def _ref(key, make):
    if key not in _REF:
        _REF[key] = make()
        _REF[key].setflags(write=False)
    return _REF[key]


def _env(monkeypatch, vpw, ysplit, off=False, **more):
    monkeypatch.setenv("A2AMD_VPW", str(vpw))
    monkeypatch.setenv("A2AMD_YSPLIT", str(ysplit))
    if off:
        monkeypatch.setenv("A2AMD_DEBUG", "16")
    else:
        monkeypatch.delenv("A2AMD_DEBUG", raising=False)
    for k, v in more.items():
        monkeypatch.setenv(k, v)


def _scene(be, private=None, counts=(20, 20, 80)):
    """osc2-pan voices on three buses - a delay group, a bus group, the root: with 64 voices per wavefront the first
    wavefront holds voices of all three, with 32 of two; 120 voices are no multiple of 32, 64 or 5 x 4"""
    sc = synth.Scene(be)
    sc.root()
    if private:
        sc.private_waves(5, length=private, period=256)
    total = sum(counts)
    sc.add_voices(counts[0], chain="osc2-pan", group=sc.add_group(preset="fmtest4"), total=total, private=bool(private))
    sc.add_voices(counts[1], chain="osc2-pan", group=sc.add_bus_group(), total=total, private=bool(private))
    sc.add_voices(counts[2], chain="osc2-pan", total=total, private=bool(private))
    return sc


def _all_leaves(sc):
    return [u for g in sc.groups for u in g["leaves"]] + list(sc.leaves)


def _walked(be, build, plan, between=None, info=None):
    """plan: per batch the list of its fragments' lengths; every fragment walked, a render per batch.
    between(sc, batch, fragment) runs in front of every fragment's walk; info collects a2amd_last_batch_osc2()."""
    sc = build(be)
    outs = []
    for b, frags in enumerate(plan):
        for f, n in enumerate(frags):
            if between:
                between(sc, b, f)
            sc.walk(n)
        outs.append(be.render(sum(frags)).copy())
        if info is not None:
            info.append(be.last_batch_osc2())
    be.close()
    return np.concatenate(outs, axis=1)


def _assert_batches_equal(got, want, plan, what="the oracle"):
    starts = [0] + list(np.cumsum([sum(frags) for frags in plan]))
    assert got.shape == want.shape
    for b in range(len(plan)):
        a, w = got[:, starts[b]:starts[b + 1]], want[:, starts[b]:starts[b + 1]]
        if not np.array_equal(a, w):
            ch, fr = [int(x[0]) for x in np.nonzero(a != w)]
            pytest.fail(f"batch {b} differs from {what}: first at channel {ch}, frame {fr} of the batch "
                        f"(got {int(a[ch, fr])}, want {int(w[ch, fr])}); "
                        f"{int((a != w).any(axis=0).sum())} of its {a.shape[1]} frames differ")


def _walks(frags, ysplit):
    """the rule of a2d_osc2_slice / a2d_osc2_whole, restated: per super-chunk of the batch, in time order, True where
    all its fragments are whole"""
    nchunks = (len(frags) + FCH - 1) // FCH
    per = (nchunks + ysplit - 1) // ysplit
    out = []
    for c_lo in range(0, nchunks, per):
        c_hi = min(nchunks, c_lo + per)
        for s_lo in range(c_lo, c_hi, SCH // FCH):
            s_hi = min(c_hi, s_lo + SCH // FCH)
            out.append(all(n == 64 for n in frags[s_lo * FCH:s_hi * FCH]))
    return out


def _assert_walks(infos, plan, vpw, ysplit, voices, off=False):
    assert len(infos) == len(plan) >= 3
    for b, (bi, frags) in enumerate(zip(infos, plan)):
        print(b, bi)
        y = min(ysplit, (len(frags) + FCH - 1) // FCH)      # (pick_fast_shape: no more slices than chunks)
        assert (bi.launched, bi.voices, bi.vpw, bi.ysplit, bi.voice_major) == (1, voices, vpw, y, 0 if off else 1), (b, bi)
        whole = [w and not off for w in _walks(frags, y)]
        assert bi.superchunks_voice_major == sum(whole), (b, bi, whole)
        assert bi.superchunks_chunk_major == len(whole) - sum(whole), (b, bi, whole)
        assert bi.chunk_major_mask == sum(1 << i for i, w in enumerate(whole) if not w), (b, bi, whole)


def _case(oracle_lib, monkeypatch, key, build, plan, vpw, ysplit, voices=120, between=None, off=False, **more):
    _env(monkeypatch, vpw, ysplit, off, **more)
    infos = []
    got = _walked(make_gpu(max_batch=MAXB), build, plan, between, infos)
    want = _ref(key, lambda: _walked(make_oracle(oracle_lib), build, plan, between))
    _assert_batches_equal(got, want, plan)
    _assert_walks(infos, plan, vpw, ysplit, voices, off)
    return got


@pytest.mark.parametrize("vpw", [1, 5, 32, 64])
@pytest.mark.parametrize("ysplit", [1, 16])
@pytest.mark.parametrize("nfrags", [1, 3, 4, 5, 15, 16, 17, 33, 40])
def test_batch_lengths(oracle_lib, monkeypatch, nfrags, ysplit, vpw):
    """Whole fragments only, so every super-chunk is walked voice-major: a partial last chunk (1, 3, 5, 15, 17, 33), a
    partial last super-chunk (everything but 16), a slice longer than one super-chunk (17, 33, 40 in one slice), slices
    of one chunk (16 slices asked for), lanes without a voice (120 voices)."""
    plan = [[64] * nfrags] * 3
    _case(oracle_lib, monkeypatch, ("len", nfrags), _scene, plan, vpw, ysplit)


SHORT = {"start": [0], "middle": [20], "end": [39], "two": [15, 16], "all": list(range(40))}


@pytest.mark.parametrize("vpw", [5, 32])
@pytest.mark.parametrize("ysplit", [1, 2, 16])
@pytest.mark.parametrize("where", sorted(SHORT))
def test_short_fragments(oracle_lib, monkeypatch, where, ysplit, vpw):
    """Batches of 40 fragments with 37-frame ones at the start, in the middle, at the end, on both sides of a
    super-chunk's edge, and nothing else: the super-chunk that holds one is walked chunk-major, its neighbours - whose
    phases start behind the short fragment's frames - voice-major (one slice: super-chunks of 16, 16 and 8 fragments;
    two: 16 + 4 each; ten slices of one chunk)."""
    frags = [37 if f in SHORT[where] else 64 for f in range(40)]
    plan = [frags, frags[::-1], frags]
    _case(oracle_lib, monkeypatch, ("short", where), _scene, plan, vpw, ysplit)
    # (what the case is for: both walks in one batch, unless every fragment is short)
    walks = _walks(frags, min(ysplit, 10))
    assert (True in walks) == (where != "all") and False in walks


def _mixed_build(be):
    """Of every five voices in a row two stay settled, one fades and one sweeps its pan (ramps of 1500 frames end inside
    the second batch of 17 fragments, those of 2500 inside the third: walked fragment by fragment and staged whole
    while they last, settled after), and one is written to in the third batch.  The first voice of the launch list
    (lane 0 of the first wavefront) is among the written ones: its bus offset reads -1 in that batch."""
    sc = _scene(be)
    for k, units in enumerate(_all_leaves(sc)):
        frames = 1500 if k % 2 else 2500
        if k % 5 == 2:
            be.unit_write(units[k % 2], 2, synth.fix(0.0007 * (1 + k % 3)), 0, frames << 8)     # fade
        if k % 5 == 3:
            be.unit_write(units[-1], 1, synth.fix(((k % 9) - 4) / 5.0), 0, frames << 8)         # pan sweep
    return sc


def _mixed_writes(sc, b, f):
    if (b, f) != (2, 5):
        return
    for k, units in enumerate(_all_leaves(sc)):
        if k % 10 in (0, 4):
            sc.be.unit_write(units[-1], 1, synth.fix(((k % 7) - 3) / 4.0))                      # pan jumps
        if k % 10 == 9:
            sc.be.unit_write(units[0], 2, synth.fix(0.0009), 0, 2000 << 8)                      # amplitude glides


@pytest.mark.parametrize("vpw", [5, 32, 64])
@pytest.mark.parametrize("ysplit", [1, 16])
def test_settled_gliding_and_written_voices_in_one_wavefront(oracle_lib, monkeypatch, ysplit, vpw):
    """Six batches of 17 fragments (a partial last chunk: the end phase is parked from a chunk of one fragment) with
    voices of every kind in every wavefront.  Only the settled ones take the voice-major walk; the staging markers and
    the committed phases are what the next batch starts from.  A2AMD_NO_MOVING: gliding voices stay this kernel's."""
    plan = [[64] * 17] * 6
    _case(oracle_lib, monkeypatch, "mixed", _mixed_build, plan, vpw, ysplit, between=_mixed_writes, A2AMD_NO_MOVING="1")


@pytest.mark.parametrize("vpw", [5, 64])
@pytest.mark.parametrize("ysplit", [1, 16])
@pytest.mark.parametrize("length", [3001, 769])
def test_waves_of_odd_sizes(oracle_lib, monkeypatch, length, ysplit, vpw):
    """Private waves whose mip levels have no power-of-two size (3001, 1501, 751 ...; 769, 385, 193 ...): the carried
    phase goes through wrap_phase's chain.  A voice advances by up to two samples a frame, 2 048 in a super-chunk of 16
    fragments: on the waves of 769 samples every voice's phase passes the level's end inside every super-chunk, more
    than once, on those of 3001 in most; the first batch starts the voices at phases up to the period's end."""
    def build(be):
        sc = _scene(be, private=length)
        for k, units in enumerate(_all_leaves(sc)):
            if k % 3 == 0:
                be.unit_write(units[k % 2], 3, 65535 - k % 7)       # (wtosc_Phase: the last steps of the period)
        return sc
    plan = [[64] * 33, [64] * 17, [64] * 40]
    _case(oracle_lib, monkeypatch, ("odd", length), build, plan, vpw, ysplit)


OFF_CASES = {
    "lengths": (_scene, [[64] * 17, [64] * 40, [64] * 3, [64] * 16], None, {}),
    "short": (_scene, [[37 if f in (0, 20) else 64 for f in range(40)]] * 3, None, {}),
    "mixed": (_mixed_build, [[64] * 17] * 6, _mixed_writes, {"A2AMD_NO_MOVING": "1"}),
}


@pytest.mark.parametrize("vpw,ysplit", [(5, 1), (32, 16), (64, 2)])
@pytest.mark.parametrize("what", sorted(OFF_CASES))
def test_switch_off_against_switch_on(oracle_lib, monkeypatch, what, vpw, ysplit):
    """A2AMD_DEBUG bit 16: the report says that no super-chunk was walked voice-major, and every batch - so the state
    every batch left for the next - is what the voice-major walk renders, and the oracle."""
    build, plan, between, more = OFF_CASES[what]
    on = _case(oracle_lib, monkeypatch, ("off", what), build, plan, vpw, ysplit, between=between, **more)
    off = _case(oracle_lib, monkeypatch, ("off", what), build, plan, vpw, ysplit, between=between, off=True, **more)
    _assert_batches_equal(off, on, plan, "the voice-major walk")
