"""k_leaf_osc2pan's fused multiply-add steps on tame mip levels (a2amd_fast.hip; include/a2amd_osc2tame.h).

A settled voice both of whose oscillators play levels in which no product of the reference's Hermite interpolation
wraps (a2amd_wave_level_tame, checked at a2amd_wave_upload) reads 16 byte coefficient entries on the voice-major walk
and takes one multiply-add and one shift per Horner step; every other voice - one oscillator on a level that is not
tame, the chunk-major walk, something moving, every voice under A2AMD_DEBUG bit 18 - takes the wrap-around steps.
Every case renders at least three batches of at most 40 fragments through the C ABI and compares every batch with the
oracle bit for bit; the tame bit and the staging mask every voice is meant to get are asserted from the rules
(a2amd_osc2_tame_rule, a2amd_osc2_stage_rule) on the very buffers uploaded, and the number of voices the kernel itself gave
the bit in every batch is read back from the device (a2amd_osc2_tame_voices): a library that never takes the fused body
fails every case.

The waves that are not tame carry the window at the edge of the 24 bit product, (dm, 32767, -32768, -32768) with
a = 65 794 - it wraps at fraction 255 only - or its mirror image, sixteen times a cycle of 64 samples, played at several
increments over thousands of frames, so that lanes do reach it at fraction 255.  That the reference really wraps there
is asserted on the oracle's own output: the same scene with the twin wave, a = 65 793 (dm two higher, tame by the
rule), differs from it by two units of one sample in four wherever nothing wraps, and by tens of thousands where
something does.

Negative check, done once by hand (profiles/osc2_tame.md): with the rule forced to "tame" in the kernel the cases with
a wrapping wave below fail, and nothing else does."""
import numpy as np
import pytest

from audiality2_amd import synth
from conftest import make_gpu, make_oracle
from test_gpu_osc2_lds_taps import MAXB, PHASES, _assert_masks, _cycle, _pitch
from test_gpu_osc2_voice_major import _assert_batches_equal, _assert_walks, _walked

pytestmark = pytest.mark.gpu

BIT18 = str(1 << 18)
_REF = {}


def _ref(key, make):
    if key not in _REF:
        _REF[key] = make()
        _REF[key].setflags(write=False)
    return _REF[key]


# ---- the waves -----------------------------------------------------------------------------------------------------
EDGE = {"W+": [32249, 32767, -32768, -32768], "T+": [32251, 32767, -32768, -32768],       # a = 65 794 / 65 793
        "W-": [-32250, -32768, 32767, 32767], "T-": [-32252, -32768, 32767, 32767]}       # a = -65 794 / -65 793
PLAIN = {"A32": (32, 1), "A64": (64, 2), "B64": (64, 3), "A96": (96, 4), "A128": (128, 5), "A256": (256, 7)}
LENGTH = dict({k: v[0] for k, v in PLAIN.items()}, **{k: 64 for k in EDGE}, **{k + "POST": 64 for k in EDGE})


def _pyramid(name):
    """(sizes, levels, tame per level as the scene is written for - None: whatever the rule says)"""
    if name in PLAIN:
        sizes, data = synth.wave_pyramid(_cycle(*PLAIN[name]))
        return sizes, data, [True] * len(sizes)
    if name in EDGE:            # the window sixteen times a cycle
        sizes, data = synth.wave_pyramid(np.array(EDGE[name] * 16, dtype=np.int16))
        return sizes, data, [name[0] == "T"] + [None] * (len(sizes) - 1)
    # ...POST: a quiet cycle whose post-pad, beyond the level's end, holds the window 32 times: the pads are not the
    # payload's, and only lanes past the end - at 2 samples a frame, up to 126 entries past it - reach them
    sizes, data = synth.wave_pyramid((_cycle(64, 8) // 8).astype(np.int16))
    at = synth.WAVEPRE + 64 + 1
    data[0][at:at + 128] = EDGE[name[:2]] * 32
    return sizes, data, [name[0] == "T"] + [True] * (len(sizes) - 1)


class _Scene(synth.Scene):
    """synth.Scene with voices made from this file's waves, and the staging masks' and tame rule's inputs per voice"""

    def __init__(self, be, names):
        super().__init__(be)
        self.w = {}
        for i, name in enumerate(names):
            sizes, data, want = _pyramid(name)
            wid = be.wave_upload(0x30000 + i, synth.WMIPWAVE, synth.LOOPED, LENGTH[name], sizes, data)
            per, tame = [None] * len(sizes), [None] * len(sizes)
            if be.prefix == "a2amd_":       # (the oracle has no such functions and no use for the bits)
                per = [be.wave_level_periodic(d) for d in data]
                tame = [be.wave_level_tame(d) for d in data]
                assert all(w is None or w == t for w, t in zip(want, tame)), (name, want, tame)
                assert per[0] == (not name.endswith("POST")), (name, per)
            self.w[name] = (wid, sizes, per, tame)
        self.tab = be.get_pitch_table()
        self.base = synth.basepitch_for(48000)
        self.masks, self.tame = [], []

    def voice(self, spec, phases, k, group=None, total=6):
        be, key = self.be, self._key()
        units = [be.unit_init(key, synth.K_WTOSC, 0, 0, 1, 0),
                 be.unit_init(key, synth.K_WTOSC, synth.PROCADD, 0, 1, 0),
                 be.unit_init(key, synth.K_PANMIX, synth.PROCADD, 1, 2, 1)]
        sp, tm = [], []
        for o, (name, level, where) in enumerate(spec):
            wid, sizes, per, tame = self.w[name]
            be.unit_write(units[o], 0, wid)
            be.unit_write(units[o], 1, _pitch(self.tab, self.base, LENGTH[name], level, where))
            be.unit_write(units[o], 2, max(1, (3 << 16) // total) + 17 * o + k)
            be.unit_write(units[o], 3, phases[o])
            sp += [sizes[level], per[level]]
            tm.append(tame[level])
        be.unit_write(units[2], 1, synth.fix(((k % 17) - 8) / 8.0))
        (self.leaves if group is None else group["leaves"]).append(units)
        self.nvoices += 1
        self.masks.append(tuple(sp))
        self.tame.append(tuple(tm))
        return units


def _builder(names, voices):
    """voices: (spec, bus) with bus 0 / 1 = one of two groups, None = the root"""
    def build(be):
        sc = _Scene(be, names)
        sc.root()
        buses = [sc.add_group(preset="fmtest4"), sc.add_bus_group()]
        for k, (spec, bus) in enumerate(voices):
            sc.voice(spec, (PHASES[k % 8], PHASES[(k + 3) % 8]), k, None if bus is None else buses[bus])
        return sc
    return build


def _case(oracle_lib, monkeypatch, key, names, voices, plan, vpw, ysplit, masks, tame, debug=None):
    monkeypatch.setenv("A2AMD_VPW", str(vpw))
    monkeypatch.setenv("A2AMD_YSPLIT", str(ysplit))
    if debug:
        monkeypatch.setenv("A2AMD_DEBUG", debug)
    else:
        monkeypatch.delenv("A2AMD_DEBUG", raising=False)
    assert 2 <= len(voices) <= 6 and len(plan) >= 3 and all(len(f) <= MAXB for f in plan)
    build, infos = _builder(names, voices), []

    def build_and_check(be):
        sc = build(be)
        _assert_masks(be, sc, masks)
        got = [be.osc2_tame_rule(*t) for t in sc.tame]
        assert got == tame, list(zip(sc.tame, got, tame))
        return sc
    be, counts = make_gpu(max_batch=MAXB), []
    render = be.render

    def render_and_count(frames):
        out = render(frames)
        counts.append(be.osc2_tame_voices())
        return out
    be.render = render_and_count
    got = _walked(be, build_and_check, plan, None, infos)
    # the kernel itself gave the bit to that many voices in every batch behind the first (in which the voices are born
    # and carry records: not this kernel's) - none under bit 18
    want_tame = 0 if debug else sum(tame)
    assert [b - a for a, b in zip(counts, counts[1:])] == [want_tame] * (len(plan) - 1), (counts, want_tame)
    assert counts[0] in (0, want_tame), counts
    want = _ref(key, lambda: _walked(make_oracle(oracle_lib), build, plan))
    _assert_batches_equal(got, want, plan)
    _assert_walks(infos, plan, vpw, ysplit, len(voices))
    return got


PLAN = [[64] * 5, [64] * 17, [64] * 20]

# every staging mask with both oscillators tame, sizes that are no power of two among them, on two buses and the root
MASKED = [
    ((("A128", 1, "lo"), ("B64", 0, "hi")), 0),         # 64 + 64: mask 3
    ((("A128", 0, "hi"), ("A256", 1, "lo")), 0),        # 128 + 128: mask 1
    ((("A256", 0, "hi"), ("B64", 0, 0.45)), 1),         # 256, 64: mask 2
    ((("A256", 0, "hi"), ("A256", 0, 0.3)), 1),         # mask 0
    ((("A96", 0, "hi"), ("A128", 1, "hi")), None),      # 96 entries: mask 2
    ((("A32", 0, "hi"), ("A64", 1, "lo")), None),       # 32 + 32: mask 3
]
MASKED_NAMES = ["A32", "A64", "B64", "A96", "A128", "A256"]
MASKED_MASKS = [3, 1, 2, 0, 2, 3]


@pytest.mark.parametrize("vpw,ysplit", [(32, 1), (2, 16)])
def test_every_staging_mask_tame(oracle_lib, monkeypatch, vpw, ysplit):
    """Both oscillators tame under each of the four staging masks - gathers from the 16 byte table, 16 byte copies in
    LDS, one of each - with increments on a level's last and first value and below half a sample, start phases at the
    period's end, batches of 5, 17 and 20 fragments: partial chunks and a second super-chunk."""
    _case(oracle_lib, monkeypatch, "masked", MASKED_NAMES, MASKED, PLAN, vpw, ysplit, MASKED_MASKS, [1] * 6)


@pytest.mark.parametrize("where", [0, 9, 19])
def test_short_fragment(oracle_lib, monkeypatch, where):
    """A 37-frame fragment in a batch of 20: its super-chunk is walked chunk by chunk with the wrap-around steps, the
    other takes the fused ones."""
    frags = [37 if f == where else 64 for f in range(20)]
    _case(oracle_lib, monkeypatch, ("short", where), MASKED_NAMES, MASKED, [frags, frags[::-1], frags], 32, 1,
          MASKED_MASKS, [1] * 6)


def _edge_voices(w):
    return [
        (((w, 0, 0.45), ("A64", 0, "hi")), 0),          # the first oscillator not tame: the wrapped body, both staged
        ((("A256", 0, 1.2), (w, 0, 1.5)), 0),           # the second: the wrapped body, the second staged
        ((("A64", 0, 1.3), ("B64", 0, 0.9)), 0),        # a tame voice between them, same wavefront, same bus
        (((w, 0, 1.1), (w, 0, 0.7)), 1),                # both, on the second bus
        ((("A256", 0, "hi"), ("A64", 0, 0.45)), 1),     # tame, on the second bus
        (((w, 0, "hi"), ("A256", 0, 0.3)), None),
    ]


EDGE_MASKS = [3, 2, 3, 3, 2, 1]


@pytest.mark.parametrize("sign", ["+", "-"])
def test_wrapping_window_takes_the_wrapped_body(oracle_lib, monkeypatch, sign):
    """a = 65 794 (-65 794): a voice with one oscillator or both on that level is not tame, beside tame voices in the
    same wavefront on two buses; and the twin wave, a = 65 793 (-65 793), is tame in every voice"""
    names = ["A64", "B64", "A256", "W" + sign]
    _case(oracle_lib, monkeypatch, "W" + sign, names, _edge_voices("W" + sign), PLAN, 32, 1, EDGE_MASKS, [0, 0, 1, 0, 1, 0])
    names[-1] = "T" + sign
    _case(oracle_lib, monkeypatch, "T" + sign, names, _edge_voices("T" + sign), PLAN, 32, 1, EDGE_MASKS, [1] * 6)
    # (the reference wraps in W and not in T: dm differs by 2, the outputs by tens of thousands)
    assert np.abs(_REF["W" + sign].astype(np.int64) - _REF["T" + sign]).max() > 2000


def _post_voices(w):
    return [
        (((w, 0, "hi"), ("A64", 0, "hi")), 0),          # 2 samples a frame from the period's end: lane 63 is 126 entries past it
        ((("A256", 0, 1.2), (w, 0, 1.9)), 0),
        ((("A64", 0, 1.3), ("B64", 0, 0.9)), 1),
        (((w, 0, 1.7), (w, 0, "hi")), None),
    ]


POST_MASKS = [2, 0, 3, 0]


def test_wrapping_window_in_the_post_pad(oracle_lib, monkeypatch):
    """The only wrapping windows lie in the post-pad, beyond the level's end (the pads are not the payload's, so the
    level is not staged either): reached by the lanes past the end, and the voice is not tame"""
    names = ["A64", "B64", "A256", "W+POST"]
    _case(oracle_lib, monkeypatch, "WPOST", names, _post_voices("W+POST"), PLAN, 32, 1, POST_MASKS, [0, 0, 1, 0])
    names[-1] = "T+POST"
    _case(oracle_lib, monkeypatch, "TPOST", names, _post_voices("T+POST"), PLAN, 32, 1, POST_MASKS, [1] * 4)
    assert np.abs(_REF["WPOST"].astype(np.int64) - _REF["TPOST"]).max() > 2000


@pytest.mark.parametrize("vpw,ysplit", [(32, 1), (2, 16)])
def test_switch_off_against_switch_on(oracle_lib, monkeypatch, vpw, ysplit):
    """A2AMD_DEBUG bit 18: no voice takes the fused steps; every batch equals the fused render and the oracle."""
    on = _case(oracle_lib, monkeypatch, "masked", MASKED_NAMES, MASKED, PLAN, vpw, ysplit, MASKED_MASKS, [1] * 6)
    off = _case(oracle_lib, monkeypatch, "masked", MASKED_NAMES, MASKED, PLAN, vpw, ysplit, MASKED_MASKS, [1] * 6, debug=BIT18)
    _assert_batches_equal(off, on, PLAN, "the fused render")
