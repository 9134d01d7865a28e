"""k_leaf_osc2pan's voice-major walk with small mip levels read from LDS (a2amd_fast.hip; include/a2amd_osc2lds.h).

A settled voice's oscillator whose level has periodic pads, a power-of-two size and at most 128 entries has that level's
payload entries copied into the wavefront's LDS and its taps read there, indexed modulo the size; the second oscillator
too if both levels fit in the 128 entries together (a2amd_osc2_stage_rule).  Everything else - other levels, the
chunk-major walk, voices with something moving, every voice under A2AMD_DEBUG bit 17 - gathers from the global table.
Every case renders at least three batches through the C ABI and compares every batch with the oracle bit for bit; the
mask every voice is meant to get is asserted from the rule and the sizes uploaded here, the walk from
a2amd_last_batch_osc2().  The waves are this file's own single cycles of 32, 64, 96, 128 and 256 samples; the pitches
are found on the backend's own pitch table so that an increment sits exactly on the last value of a level (2 samples a
frame), on the first of the next (just above 1), or well inside.

Negative check, done once by hand (profiles/osc2_lds_taps.md): with the periodic bit forced on in the kernel the
non-periodic cases below fail, and nothing else does."""
import numpy as np
import pytest

from audiality2_amd import synth
from conftest import make_gpu, make_oracle
from test_gpu_osc2_voice_major import _assert_batches_equal, _assert_walks, _walked

pytestmark = pytest.mark.gpu

MAXB = 40
MAXPHINC, MIPS = 512, 10
BIT17 = str(1 << 17)
_REF = {}


def _ref(key, make):
    if key not in _REF:
        _REF[key] = make()
        _REF[key].setflags(write=False)
    return _REF[key]


# ---- the waves -----------------------------------------------------------------------------------------------------
def _cycle(length, seed):
    """a band-rich single cycle: three sines and a little noise, so that no two entries of a level are alike"""
    rng = np.random.default_rng(seed)
    n = np.arange(length)
    w = (np.sin(2 * np.pi * n / length) * 14000 + np.sin(2 * np.pi * 3 * n / length + seed) * 9000
         + np.sin(2 * np.pi * 7 * n / length) * 4000 + rng.integers(-2500, 2501, size=length))
    return np.clip(w, -32767, 32767).astype(np.int16)


WAVES = {"A32": (32, 1), "A64": (64, 2), "B64": (64, 3), "A96": (96, 4), "A128": (128, 5), "B128": (128, 6), "A256": (256, 7),
         "NPOST": (64, 8), "NPRE": (64, 9), "PPOST": (64, 8), "PPRE": (64, 9)}    # (P...: N...'s cycle with its pads left periodic)


def _pyramid(name):
    length, seed = WAVES[name]
    sizes, data = synth.wave_pyramid(_cycle(length, seed))
    if name == "NPOST":         # one post-pad sample of level 0 is not the payload's: sample size + 1
        data[0][synth.WAVEPRE + length + 1] ^= 0x2aaa
    if name == "NPRE":          # ... the pre-pad
        data[0][0] ^= 0x2aaa
    return sizes, data


def _upload(be, names):
    """{name: (wave id, sizes, periodic per level)}.  The product library says itself, by the check a2amd_wave_upload()
    runs (a2amd_wave_level_periodic), which of the very buffers uploaded have periodic pads: every level but level 0
    of the N... waves.  The oracle has no such function and no use for the flags."""
    out = {}
    for i, name in enumerate(names):
        sizes, data = _pyramid(name)
        wid = be.wave_upload(0x20000 + i, synth.WMIPWAVE, synth.LOOPED, WAVES[name][0], sizes, data)
        per = [None] * len(sizes)
        if be.prefix == "a2amd_":
            per = [be.wave_level_periodic(d) for d in data]
            assert per == [not (name.startswith("N") and lv == 0) for lv in range(len(sizes))], (name, per)
        out[name] = (wid, sizes, per)
    return out


# ---- pitches ---------------------------------------------------------------------------------------------------------
def _p2i(tab, pitch):
    """a2_P2I, pitch.c:57-67"""
    n, octave = pitch & 0xffff, pitch >> 16
    dph = ((int(tab[2 * (n >> 10) + 1]) * (n & 0x3ff)) & 0xffffffff) >> 2
    dph = (dph + int(tab[2 * (n >> 10)])) & 0xffffffff
    return dph >> ((7 - octave) & 31)


def _mip(dphase, period):
    """wtosc.c:250-258: (level, samples a frame there)"""
    d, mm = (((dphase + 255) & 0xffffffff) >> 8) * period, 0
    while d > (MAXPHINC << 8) and mm < MIPS - 1:
        d >>= 1
        mm += 1
    return mm, ((dphase * period) >> mm) / float(1 << 24)


def _pitch(tab, base, period, level, where):
    """The value to write to a wtosc's pitch register so that a wave of `period` plays at `level`: where = "hi", the
    last pitch of the level (2 samples a frame); "lo", the first (just above 1; level >= 1); a number, that many samples
    a frame."""
    def lvl(p):
        return _mip(_p2i(tab, p + base), period)[0]
    lo, hi = -6 << 16, 6 << 16
    if where == "hi":           # the largest p with lvl(p) <= level
        assert lvl(lo) <= level < lvl(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if lvl(mid) <= level else (lo, mid)
        p = lo
    elif where == "lo":         # the smallest p with lvl(p) >= level
        assert level >= 1 and lvl(lo) < level <= lvl(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if lvl(mid) >= level else (mid, hi)
        p = hi
    else:
        p = int(round(np.log2(where * (1 << level) * 48000.0 / (period * 261.626)) * 65536.0))
    mm, inc = _mip(_p2i(tab, p + base), period)
    assert mm == level, (period, level, where, mm, inc)
    if where == "hi":
        assert 1.999 < inc <= 2.0, inc
    elif where == "lo":
        assert 1.0 < inc < 1.001, inc
    return p


# ---- scenes ------------------------------------------------------------------------------------------------------------
# a voice: ((wave, level, where), (wave, level, where)); an oscillator's level size is the wave's length >> level
PAIRS = [
    ((64, 64), 3, (("A128", 1, "lo"), ("B64", 0, "hi"))),
    ((128, 128), 1, (("A128", 0, "hi"), ("A256", 1, "lo"))),
    ((128, 64), 1, (("B128", 0, 1.5), ("A64", 0, "hi"))),
    ((256, 64), 2, (("A256", 0, "hi"), ("B64", 0, 0.45))),
    ((64, 256), 1, (("A64", 0, 0.45), ("A256", 0, 1.25))),
    ((32, 32), 3, (("A32", 0, "hi"), ("A64", 1, "lo"))),
    ((96, 64), 2, (("A96", 0, "hi"), ("A128", 1, "hi"))),
    ((256, 256), 0, (("A256", 0, "hi"), ("A256", 0, 0.3))),
]
# start phases (wtosc_Phase: 16 bit fractions of the period): the period's last steps put the first fragment's lane 63,
# at 2 samples a frame, at the highest index a fragment reaches - past the level's end by 126 entries and tap B's one
# more, four times around a level of 32
PHASES = [65535, 0, 65280, 32768, 65535 - 300, 12345, 65534, 1]


class _Scene(synth.Scene):
    """synth.Scene with voices made from this file's waves, and the masks the rule gives them"""

    def __init__(self, be, names):
        super().__init__(be)
        self.w = _upload(be, names)
        self.tab = be.get_pitch_table()
        self.base = synth.basepitch_for(48000)
        self.masks = []

    def voice(self, spec, phases, k, group=None, total=64):
        be, key = self.be, self._key()
        units = [be.unit_init(key, synth.K_WTOSC, 0, 0, 1, 0),
                 be.unit_init(key, synth.K_WTOSC, synth.PROCADD, 0, 1, 0),
                 be.unit_init(key, synth.K_PANMIX, synth.PROCADD, 1, 2, 1)]
        sp = []
        for o, (name, level, where) in enumerate(spec):
            wid, sizes, per = self.w[name]
            be.unit_write(units[o], 0, wid)
            be.unit_write(units[o], 1, _pitch(self.tab, self.base, WAVES[name][0], level, where))
            be.unit_write(units[o], 2, max(1, (3 << 16) // total) + 17 * o + k)
            be.unit_write(units[o], 3, phases[o])
            sp += [sizes[level], per[level]]
        be.unit_write(units[2], 1, synth.fix(((k % 17) - 8) / 8.0))
        (self.leaves if group is None else group["leaves"]).append(units)
        self.nvoices += 1
        self.masks.append(tuple(sp))
        return units


def _pairs_build(be):
    """Every size pair eight times with the start phases above (the second oscillator's one step round), then six more
    voices: 70, two wavefronts of 32 and a tail; three buses"""
    names = sorted({n for _, _, spec in PAIRS for n, _, _ in spec})
    sc = _Scene(be, names)
    sc.root()
    buses = [sc.add_group(preset="fmtest4"), sc.add_bus_group(), None]
    k = 0
    for j in range(len(PHASES)):
        for sizes, _, spec in PAIRS:
            sc.voice(spec, (PHASES[j], PHASES[(j + 1) % len(PHASES)]), k, buses[k % 3], total=70)
            assert sc.masks[-1][0::2] == sizes      # (the levels have the sizes the pair is named for)
            k += 1
    for j in range(6):
        sc.voice(PAIRS[(3 * j) % len(PAIRS)][2], (PHASES[j], PHASES[j]), k, buses[k % 3], total=70)
        k += 1
    return sc


def _assert_masks(be, sc, want):
    """the rule on what was uploaded gives every voice the mask the scene was written for"""
    got = [be.osc2_stage_rule(*m) for m in sc.masks]
    assert got == want, list(zip(sc.masks, got, want))


def _case(oracle_lib, monkeypatch, key, build, plan, vpw, ysplit, voices, masks, between=None, debug=None, **more):
    monkeypatch.setenv("A2AMD_VPW", str(vpw))
    monkeypatch.setenv("A2AMD_YSPLIT", str(ysplit))
    if debug:
        monkeypatch.setenv("A2AMD_DEBUG", debug)
    else:
        monkeypatch.delenv("A2AMD_DEBUG", raising=False)
    for k, v in more.items():
        monkeypatch.setenv(k, v)
    infos, scenes = [], []

    def build_and_keep(be):
        scenes.append(build(be))
        _assert_masks(be, scenes[-1], masks)
        return scenes[-1]
    got = _walked(make_gpu(max_batch=MAXB), build_and_keep, plan, between, infos)
    want = _ref(key, lambda: _walked(make_oracle(oracle_lib), build, plan, between))
    _assert_batches_equal(got, want, plan)
    _assert_walks(infos, plan, vpw, ysplit, voices)
    return got


PLAN = [[64] * 1, [64] * 4, [64] * 5, [64] * 16, [64] * 17, [64] * 20]
PAIR_MASKS = [m for _ in PHASES for _, m, _ in PAIRS] + [PAIRS[(3 * j) % len(PAIRS)][1] for j in range(6)]


@pytest.mark.parametrize("vpw,ysplit", [(32, 1), (5, 16), (32, 16)])
def test_size_pairs(oracle_lib, monkeypatch, vpw, ysplit):
    """Every pair of level sizes at and around the limit - both staged, the first only (the budget's edge: 128 + 128,
    128 + 64), the second only (a first level too large, or of 96 entries), none - with increments on a level's last
    value, on its first and below half a sample, from start phases at the period's end; batches of 1, 4, 5, 16, 17 and
    20 fragments, so partial chunks and a second super-chunk."""
    _case(oracle_lib, monkeypatch, "pairs", _pairs_build, PLAN, vpw, ysplit, 70, PAIR_MASKS)


# one wavefront, in this order on each of three buses: table A, table B of the same size, unstaged, table A again, two
# different tables at once - and between them a voice that fades and one that is written to in the third batch, and
# behind them one whose pitch glides across a level's edge
ORDER = [
    (1, (("A64", 0, "hi"), ("A256", 0, 1.1))),
    (1, (("B64", 0, 1.7), ("A256", 0, "hi"))),
    (None, (("A64", 0, 1.3), ("B64", 0, 0.9))),         # fades: not settled while it does; staged (both) after
    (0, (("A256", 0, 0.8), ("A256", 0, "hi"))),
    (1, (("A64", 0, 0.45), ("A256", 0, 0.7))),
    (None, (("B64", 0, "hi"), ("A64", 0, "hi"))),       # its pan is written in the third batch
    (3, (("A64", 0, "hi"), ("B64", 0, "hi"))),
    (1, (("A128", 0, "hi"), ("A64", 0, 1.0))),          # its first pitch glides up: level 0 (128) -> level 1 (64), mask 1 -> 3
]
ORDER_MASKS = [3 if m is None else m for m, _ in ORDER] * 3


def _order_build(be):
    sc = _Scene(be, ["A64", "B64", "A128", "A256"])
    sc.root()
    k = 0
    for bus in (sc.add_group(preset="fmtest4"), sc.add_bus_group(), None):
        for j, (m, spec) in enumerate(ORDER):
            units = sc.voice(spec, (PHASES[(j + k) % 8], PHASES[(j + 3) % 8]), k, bus, total=24)
            if j == 2:
                be.unit_write(units[0], 2, synth.fix(0.0007), 0, 700 << 8)      # (ends inside the fourth batch)
            if j == 7:      # (2 -> 3 samples a frame at level 0, that is 1.5 at level 1; ends inside the third batch)
                be.unit_write(units[0], 1, _pitch(sc.tab, sc.base, 128, 1, 1.5), 0, 500 << 8)
            k += 1
    return sc


def _order_writes(sc, b, f):
    if (b, f) == (2, 2):
        for k, units in enumerate([u for g in sc.groups for u in g["leaves"]] + list(sc.leaves)):
            if k % len(ORDER) == 5:
                sc.be.unit_write(units[2], 1, synth.fix(((k % 7) - 3) / 4.0))


@pytest.mark.parametrize("ysplit", [1, 16])
def test_one_wavefront_restages_between_voices(oracle_lib, monkeypatch, ysplit):
    """24 voices in one wavefront: what one voice left in the wavefront's LDS must not be read by the next - another
    table of the same size, no table, the first again, two tables - with gliding and record-carrying voices in between
    and a tile flush at every change of bus.  A2AMD_NO_MOVING: the gliding voices stay this kernel's."""
    _case(oracle_lib, monkeypatch, "order", _order_build, PLAN, 32, ysplit, 24, ORDER_MASKS, between=_order_writes,
          A2AMD_NO_MOVING="1")


def _nonperiodic_build(which):
    def build(be):
        sc = _Scene(be, ["A64", "A256", which])
        sc.root()
        bus = sc.add_bus_group()
        for k in range(12):
            spec = ((which, 0, ("hi", 1.5, 0.45)[k % 3]), ("A64", 0, "hi")) if k % 2 == 0 else \
                   (("A256", 0, 1.2), (which, 0, ("hi", 1.5, 0.45)[k % 3]))
            sc.voice(spec, (PHASES[k % 8], PHASES[(k + 5) % 8]), k, bus if k % 4 < 2 else None, total=12)
        return sc
    return build


NONPERIODIC_MASKS = [2 if k % 2 == 0 else 0 for k in range(12)]


@pytest.mark.parametrize("which", ["NPOST", "NPRE"])
def test_non_periodic_wave_is_not_staged(oracle_lib, monkeypatch, which):
    """A wave of 64 samples whose post-pad (sample 65) or pre-pad differs from the payload in one sample: the oracle reads
    the pads, so must the kernel - the level is left to the gathers, the other oscillator's level is staged beside it.
    (That the oracle's output for these waves differs from the periodic waves' was checked when the case was written,
    and is asserted below: otherwise the case could not fail.)"""
    plan = PLAN[1:4]
    _case(oracle_lib, monkeypatch, which, _nonperiodic_build(which), plan, 32, 1, 12, NONPERIODIC_MASKS)
    periodic = _ref("P" + which[1:], lambda: _walked(make_oracle(oracle_lib), _nonperiodic_build("P" + which[1:]), plan))
    assert not np.array_equal(_REF[which], periodic)


SHORT = {"start": 0, "middle": 9, "end": 19}


@pytest.mark.parametrize("where", sorted(SHORT))
def test_short_fragment(oracle_lib, monkeypatch, where):
    """A 37-frame fragment in a batch of 20: its super-chunk is walked chunk by chunk and gathers, the other stages."""
    frags = [37 if f == SHORT[where] else 64 for f in range(20)]
    plan = [frags, frags[::-1], frags]
    _case(oracle_lib, monkeypatch, ("short", where), _pairs_build, plan, 32, 1, 70, PAIR_MASKS)


@pytest.mark.parametrize("vpw,ysplit", [(32, 1), (5, 16)])
def test_switch_off_against_switch_on(oracle_lib, monkeypatch, vpw, ysplit):
    """A2AMD_DEBUG bit 17: nothing is staged; every batch equals the staged render and the oracle."""
    plan = PLAN[2:5]
    on = _case(oracle_lib, monkeypatch, "bit17", _pairs_build, plan, vpw, ysplit, 70, PAIR_MASKS)
    off = _case(oracle_lib, monkeypatch, "bit17", _pairs_build, plan, vpw, ysplit, 70, PAIR_MASKS, debug=BIT17)
    _assert_batches_equal(off, on, plan, "the staged render")
