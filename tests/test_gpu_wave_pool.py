"""The wave pool's life cycle under playing voices (csrc/a2amd_host.cpp: wave_place, a2amd_wave_drop, wave_tap_policy,
coef4_drop, grow; include/a2amd_wavepool.h).

Every wavetable kernel reads its taps through tables the host moves, rebuilds and re-labels while voices play them: the
sample pool, the 12 byte Hermite entries, the 16 byte entries of the fused steps and the per-wave descriptor with its
raw-taps, periodic and tame bits.  Every case here renders one cast of 64 settled voices - every wavetable leaf
class, on the root, a delay group, a bus group and a mono group, one voice gliding, one with control writes cut into
sub-fragment windows - through the C ABI in batches of 5 to 8 fragments (max_batch 8, one 37-frame fragment in every
case but the two of whole repeated steps), lets the host do one of these things between two batches or inside an open
one, and compares every batch with the oracle bit for bit.  That the event really happened is asserted from a2amd_wave_pool_info() against a model of the
host's layout rule kept here (_Pool: A2AMD_WAVEPRE + size + A2AMD_WAVEPOST per level, the sum rounded up to 8; first fit;
neighbours merged; the tail given back; capacity doubled; the budget on 12 bytes a sample), so a library in which a
reallocation, a dropped table, a raw flag or a reused region silently does not happen fails even where the audio
matches; the voices k_leaf_osc2pan gave the tame bit are read per batch (a2amd_osc2_tame_voices) and compared with the
rule (a2amd_osc2_tame_rule) on the levels every voice plays.

The tests without the gpu mark are the premises, on the oracle's rendering and the model alone: every phase of every
case is audible, a dropped or replaced wave changes the mix from its batch on and not before, every voice of the cast
and every voice a case adds changes the mix when it is left out, every wave is tame / not tame / periodic as the cast
is written for (a2amd_wave_level_tame, a2amd_wave_level_periodic: host functions), and the sizes put the pool on the
intended side of the budget and of the 8 388 608 samples it starts with.

Negative checks, done once by hand (profiles/wave_pool_tests.md): without the k_build_coef launch after growth the
growing cases fail; with an upload's entry range begun one sample late the reuse cases fail."""
import ctypes as C

import numpy as np
import pytest

from audiality2_amd import synth
from audiality2_amd.replay import MIPLEVELS, WAVEPOST, WAVEPRE
from conftest import make_gpu, make_oracle
from test_gpu_launch_plan import launches
from test_gpu_osc2_lds_taps import PHASES, _mip, _p2i, _pitch
from test_gpu_osc2_tame import LENGTH, _Scene, _pyramid
from test_gpu_osc2_voice_major import _assert_batches_equal, _walks

gpu = pytest.mark.gpu
MAXB = 8
POOL0 = 8388608             # samples the pool starts with (a2amd_open)
ENTRY = 12                  # bytes of a Hermite entry: what the footprint policy counts
BIGWAVE = 4300000           # two of these, plain, outgrow POOL0
ASYNC = 4 | 1 | 2 | 8 | 32  # bench.py's render flags: readback into the library's buffer, asynchronous (test_gpu_parity._async_steps)


# ---- the host's layout rule, restated ----------------------------------------------------------------------------------
def region(wtype, sizes):
    levels = MIPLEVELS if wtype == synth.WMIPWAVE else 1 if wtype == synth.WWAVE else 0
    sizes = list(sizes) + [0] * MIPLEVELS
    return (sum(WAVEPRE + sizes[lv] + WAVEPOST for lv in range(levels)) + 7) & ~7


class _Pool:
    """what wave_place(), a2amd_wave_drop(), wavepool_release(), wave_tap_policy() and grow() make of the calls"""

    def __init__(self, budget_mb):
        self.budget = budget_mb << 20
        self.used, self.cap, self.free, self.deferred = 0, POOL0, [], []
        self.waves, self.raw = {}, set()        # key: (offset, length, type, size of level 0)
        self.coef4 = self.budget >= 0
        self.reallocs = self.reused = 0
        self.open = False                       # fragments recorded and not rendered

    def place(self, key, wtype, sizes):
        total = region(wtype, sizes)
        if key in self.waves:                   # same key again: the old region serves what is recorded
            old = self.waves.pop(key)
            self.raw.discard(key)
            if old[1]:
                self.deferred.append(old[:2])
        pos = None
        for k, (off, ln) in enumerate(self.free):
            if total and ln >= total:
                pos = off
                self.free[k] = (off + total, ln - total)
                if not self.free[k][1]:
                    del self.free[k]
                self.reused += 1
                break
        if pos is None:
            if self.used + total > self.cap:
                if not (self.coef4 and (self.used + total) * ENTRY <= self.budget):
                    self.coef4 = False
                self.cap = max(self.used + total, 2 * self.cap)
                self.reallocs += 1
            pos = self.used
            self.used += total
        self.waves[key] = (pos, total, wtype, (list(sizes) + [0])[0] if total else 0)
        big = self.used * ENTRY > self.budget
        if big:
            self.coef4 = False
        self.raw = {k for k, w in self.waves.items() if big and w[2] == synth.WMIPWAVE and w[3] >= 4096}

    def release(self, off, ln):
        self.free = sorted(self.free + [(off, ln)])
        merged = []
        for o, n in self.free:
            if merged and merged[-1][0] + merged[-1][1] == o:
                merged[-1] = (merged[-1][0], merged[-1][1] + n)
            else:
                merged.append((o, n))
        if merged and merged[-1][0] + merged[-1][1] == self.used:
            self.used = merged.pop()[0]
        self.free = merged

    def drop(self, key):
        off, ln = self.waves.pop(key)[:2]
        self.raw.discard(key)
        if ln:
            self.deferred.append((off, ln))
        if not self.open:
            self.end_batch()

    def end_batch(self):
        for off, ln in self.deferred:
            self.release(off, ln)
        self.deferred, self.open = [], False

    def state(self):
        return dict(used=self.used, capacity=self.cap, free_samples=sum(n for _, n in self.free), coef4=int(self.coef4),
                    raw_waves=len(self.raw), reallocations=self.reallocs, regions_reused=self.reused)


# ---- the product library's host functions: no device ---------------------------------------------------------------------
class _Rules:
    def __init__(self, lib):
        def fn(name, restype, *argtypes):
            f = getattr(lib, name)
            f.restype, f.argtypes = restype, list(argtypes)
            return f
        self._tame = fn("a2amd_wave_level_tame", C.c_int, C.POINTER(C.c_int16), C.c_uint)
        self._periodic = fn("a2amd_wave_level_periodic", C.c_int, C.POINTER(C.c_int16), C.c_uint)
        self.tame_rule = fn("a2amd_osc2_tame_rule", C.c_uint, C.c_int, C.c_int)
        self.stage_rule = fn("a2amd_osc2_stage_rule", C.c_uint, C.c_uint, C.c_int, C.c_uint, C.c_int)

    def levels(self, data):
        out = []
        for d in data:
            d = np.ascontiguousarray(d, dtype=np.int16)
            p, n = d.ctypes.data_as(C.POINTER(C.c_int16)), len(d) - WAVEPRE - WAVEPOST
            out.append((bool(self._periodic(p, n)), bool(self._tame(p, n))))
        return out


_RULES = []


def _rules():
    if not _RULES:
        import audiality2_amd
        _RULES.append(_Rules(audiality2_amd.load_library()))
    return _RULES[0]


# ---- the waves ---------------------------------------------------------------------------------------------------------
TAME_NAMES = ["A32", "A64", "B64", "A96", "A128", "A256", "W+"]     # test_gpu_osc2_tame's, keys 0x30000 + i
_WAVES = {}


def _private(n, seed, amp=9000):
    """a looped private wave: a random walk without drift, smoothed a little, its ends joined"""
    key = (n, seed, amp)
    if key not in _WAVES:
        rng = np.random.default_rng(seed)
        w = np.cumsum(rng.integers(-300, 301, size=n + 64)).astype(np.float64)
        w -= np.linspace(w[0], w[-1], len(w))
        w = w[:n] * (amp / max(1.0, np.abs(w).max())) + rng.integers(-200, 201, size=n)
        _WAVES[key] = np.clip(w, -32767, 32767).astype(np.int16)
        _WAVES[key].setflags(write=False)
    return _WAVES[key]


def _big(i):
    """a plain wave of BIGWAVE samples with its pads, a short pattern tiled: nothing but its size matters (made once)"""
    if ("big", i) not in _WAVES:
        pat = np.random.default_rng(40 + i).integers(-9000, 9001, size=1000 + 7 * i).astype(np.int16)
        sizes, data = synth.wave_pyramid(np.resize(pat, BIGWAVE), levels=1)
        data[0].setflags(write=False)
        _WAVES[("big", i)] = (sizes, data)
    return _WAVES[("big", i)]


# ---- the cast ------------------------------------------------------------------------------------------------------------
# osc2-pan, test_gpu_osc2_tame's kinds: (oscillators, staging mask, tame)
CAST_OSC2 = [
    ((("A128", 1, "lo"), ("B64", 0, "hi")), 3, 1),      # both levels tame and staged in LDS
    ((("A32", 0, "hi"), ("A64", 1, "lo")), 3, 1),
    ((("A256", 0, "hi"), ("B64", 0, 0.45)), 2, 1),      # tame, one level staged
    ((("A128", 0, "hi"), ("A256", 1, "lo")), 1, 1),
    ((("A96", 0, "hi"), ("A128", 1, "hi")), 2, 1),
    ((("A256", 0, "hi"), ("A256", 0, 0.3)), 0, 1),      # tame and gathered
    ((("W+", 0, 0.45), ("A64", 0, "hi")), 3, 0),        # one level not tame
    ((("A256", 0, 1.2), ("W+", 0, 1.5)), 2, 0),
]
NOSC = {"osc": 1, "osc-pan": 1, "osc-filter-pan": 1, "osc2-pan": 2, "osc2-filter-pan": 2, "osc3-filter-pan": 3}
P5000, P4096, P3001 = 0x40000, 0x40001, 0x40002     # private waves of the cast (keys); a case's own from 0x41000


class _Cast(_Scene):
    """test_gpu_osc2_tame's scene - its waves, its voice() - with the other leaf classes beside it.  Every voice has a
    number k of its own; `skip` leaves that one out.  For every osc2-pan voice: the keys of its waves and whether the
    levels it plays are tame, for the count the kernel is asked for."""

    def __init__(self, be, skip=None, quiet=False):
        synth.Scene.__init__(self, be)          # the 24 built-in cycles, the noise wave
        self.skip, self.quiet, self.rules = skip, quiet, _rules()
        self.w, self.period, self.keys = {}, dict(LENGTH), {}
        self.tab, self.base = be.get_pitch_table(), synth.basepitch_for(48000)
        self.masks, self.tame, self.osc2, self.fragno, self.cut = [], [], [], 0, None
        self.nclass, self.flags = {c: 0 for c in NOSC}, {}
        for i, name in enumerate(TAME_NAMES):
            sizes, data, want = _pyramid(name)
            self.wave(name, 0x30000 + i, sizes, data, LENGTH[name])
            assert all(w is None or w == t for w, (_, t) in zip(want, self.flags[name])), name
        self.flags_wanted()
        for name, key, n, seed in (("P5000", P5000, 5000, 11), ("P4096", P4096, 4096, 12), ("P3001", P3001, 3001, 13)):
            self.wave(name, key, *synth.wave_pyramid(_private(n, seed)), 256)
        self.root()
        self.buses = [self.add_group(preset="fmtest4"), self.add_bus_group(), None]
        self.mono = self.add_mono_group(pan=0.25)
        k = 0
        for spec, mask, tame in CAST_OSC2:      # 24 voices: every kind on every bus
            for bus in range(3):
                self.voice2(spec, k, bus)
                k += 1
        builtin = self.wave_ids
        for j in range(9):                      # osc-pan: the private waves and the built-in cycles
            self.add("osc-pan", 100 + j, j % 3, [self.w[("P5000", "P4096", "P3001")[j % 3]][0]])
            self.add("osc-pan", 110 + j, (j + 1) % 3, [builtin[(5 * j) % 24]])
        for j in range(5):
            self.add("osc-filter-pan", 120 + j, j % 3, [self.w["P5000"][0] if j % 2 else builtin[3 + j]])
            self.add("osc2-filter-pan", 130 + j, (j + 1) % 3, [builtin[7 + j], self.w["P4096"][0] if j % 2 else builtin[11 + j]])
            self.add("osc3-filter-pan", 140 + j, (j + 2) % 3, [builtin[2 * j], builtin[15 + j], self.w["P3001"][0]])
            self.add("osc", 150 + j, "mono", [self.w["P5000"][0] if j % 2 else builtin[(20 + j) % 24]])
        if not quiet:
            # one voice gliding in pitch through every batch (the window kernels) ...
            units = self.add("osc-pan", 160, 2, [self.w["P5000"][0]])
            if units:
                be.unit_write(units[0], 1, synth.fix(1.25), 0, 60000 << 8)
            # ... and one with control writes cut into sub-fragment windows (the records path): walk()
            self.cut = self.add("osc-pan", 161, 1, [builtin[9]])

    def wave(self, name, key, sizes, data, period, upload=None):
        """upload (or replace) a mip-mapped wave and note what the host's own checks say of the very buffers"""
        wid = (upload or self.be.wave_upload)(key, synth.WMIPWAVE, synth.LOOPED, period, sizes, data)
        self.flags[name] = self.rules.levels(data)
        per, tame = [f[0] for f in self.flags[name]], [f[1] for f in self.flags[name]]
        self.w[name], self.period[name], self.keys[name] = (wid, sizes, per, tame), period, key
        return wid

    def flags_wanted(self):
        for name in TAME_NAMES:
            assert self.flags[name][0][0], name                     # level 0's pads are the payload's
            assert self.flags[name][0][1] == (name != "W+"), name   # ... and only the window at the product's edge wraps

    def voice2(self, spec, k, bus, device_built=()):
        """an osc2-pan voice: _Scene.voice on waves of any period.  device_built: names of waves the device made
        itself - never tame for the kernel, whatever the samples are"""
        if k == self.skip:
            return None
        saved = dict(LENGTH)
        try:                                    # (_Scene.voice looks the period up in its module's table)
            LENGTH.update({n: self.period[n] for n, _, _ in spec})
            group = {0: self.buses[0], 1: self.buses[1], 2: None}[bus]
            units = _Scene.voice(self, spec, (PHASES[k % 8], PHASES[(k + 3) % 8]), k, group, total=64)
        finally:
            LENGTH.clear()
            LENGTH.update(saved)
        tame = tuple(t and n not in device_built for t, (n, _, _) in zip(self.tame[-1], spec))
        self.osc2.append(dict(k=k, keys=[self.keys[n] for n, _, _ in spec], tame=tame, born=None))
        self.nclass["osc2-pan"] += 1
        return units

    def add(self, chain, k, bus, wids, pitch=None, phase=None):
        """a voice of any other class; oscillator o plays wids[o]; phase: where in the period it starts, of 65 536"""
        if k == self.skip:
            return None
        be, key, n = self.be, self._key(), NOSC[chain]
        if chain == "osc":
            units = [be.unit_init(key, synth.K_WTOSC, synth.PROCADD, 0, 1, 1)]
        else:
            units = [be.unit_init(key, synth.K_WTOSC, synth.PROCADD if o else 0, 0, 1, 0) for o in range(n)]
            if "filter" in chain:
                units.append(be.unit_init(key, synth.K_FILTER12, 0, 1, 1, 0))
            units.append(be.unit_init(key, synth.K_PANMIX, synth.PROCADD, 1, 2, 1))
        p = synth.fix((((k * 5) % 25) - 12) / 12.0) if pitch is None else pitch
        if "filter" in chain:
            be.unit_write(units[n], 0, p + synth.fix(2.5))
            be.unit_write(units[n], 1, synth.fix(3.0))
        for o in range(n):
            be.unit_write(units[o], 0, wids[o % len(wids)])
            be.unit_write(units[o], 1, p - synth.fix(1.0) if o == 2 else p + synth.fix(0.01) * o)
            be.unit_write(units[o], 2, (3 << 16) // 64 + 13 * o + k)
            be.unit_write(units[o], 3, (k * 2654435761 + 9973 * o) % 65536 if phase is None else phase)
        if chain != "osc":
            be.unit_write(units[-1], 1, synth.fix(((k % 17) - 8) / 8.0))
        dst = self.mono if bus == "mono" else self.buses[bus]
        (self.leaves if dst is None else dst["leaves"]).append(units)
        self.nvoices += 1
        self.nclass[chain] += 1
        return units

    def pitch(self, name, level, where):
        return _pitch(self.tab, self.base, self.period[name], level, where)

    def pitch_back_at(self, name, size, n):
        """the pitch at which a voice started on the first sample of `name`'s level 0 (`size` samples) begins its n-th
        fragment of 64 frames after that on the first sample again: 64 n increments are the size and less than one sample
        more.  (A fragment's lanes run on into the post-pad and the phase wraps between fragments, so a settled voice
        reads a level's first entry only where a fragment begins on it.)"""
        p = self.pitch(name, 0, size / (64.0 * n))
        for q in sorted(range(p - 64, p + 65), key=lambda q: abs(q - p)):
            mm, inc = _mip(_p2i(self.tab, q + self.base), self.period[name])
            if mm == 0 and 0 <= 64 * n * inc - size < 1:
                return q
        raise AssertionError((name, size, n))

    def walk(self, frames=64):
        """synth.Scene.walk, with the one voice's fragment cut in two windows and a pitch write between them"""
        be = self.be
        be.fragment(frames)
        be.unit_process(self.rootv[0], 0, frames)

        def leaf(units):
            cut = 7 + 5 * (self.fragno % 9)
            if units is self.cut and self.fragno % 2 == 0 and cut < frames:
                for u in units:
                    be.unit_process(u, 0, cut)
                be.unit_write(units[0], 1, synth.fix(((self.fragno % 13) - 6) / 12.0), 17, 300 << 8)
                for u in units:
                    be.unit_process(u, cut, frames - cut)
            else:
                for u in units:
                    be.unit_process(u, 0, frames)

        def group(g):
            be.unit_process(g["units"][0], 0, frames)
            for units in g["leaves"]:
                leaf(units)
            be.inline_end(g["units"][0])
            for u in g["units"][1:]:
                be.unit_process(u, 0, frames)
        for g in self.groups:
            group(g)
        for units in self.leaves:
            leaf(units)
        be.inline_end(self.rootv[0])
        be.unit_process(self.rootv[1], 0, frames)
        be.unit_process(self.rootv[2], 0, frames)
        self.fragno += 1


# ---- one backend's rendering of a case -------------------------------------------------------------------------------------
class _Run:
    """The script of a case against one backend, the pool's model beside it.  On the product library every event is
    checked against a2amd_wave_pool_info() and every batch against the kernels' own reports."""

    def __init__(self, be, oracle_lib, budget_mb=192, skip=None, without=(), quiet=False):
        self.be, self.gpu, self.oracle_lib, self.without = be, be.prefix == "a2amd_", oracle_lib, set(without)
        self.pool = _Pool(budget_mb)
        self.outs, self.plan, self.marks, self.inflight, self.async_plan = [], [], {}, 0, []
        self.tame_seen = be.osc2_tame_voices() if self.gpu else 0
        self.tame_due, self.launches = 0, []
        upload, drop, fragment = be.wave_upload, be.wave_drop, be.fragment

        def wave_upload(key, wtype, flags, period, sizes, data):
            self.pool.place(key, wtype, sizes)
            return upload(key, wtype, flags, period, sizes, data)

        def wave_drop(key):
            self.pool.drop(key)
            return drop(key)

        def fragment_(frames):
            self.pool.open = True
            return fragment(frames)
        be.wave_upload, be.wave_drop, be.fragment = wave_upload, wave_drop, fragment_
        self.sc = _Cast(be, skip, quiet)
        self.check()

    # -- events --
    def check(self, mark=None):
        """the library's bookkeeping is the model's; mark: keep the model's state under that name (the premises)"""
        want = self.pool.state()
        if mark:
            self.marks[mark] = dict(want, raw=set(self.pool.raw), waves=dict(self.pool.waves), budget=self.pool.budget)
        if self.gpu:
            pi = self.be.wave_pool_info()
            got = {n: int(getattr(pi, n)) for n in want}
            assert got == want, (mark, got, want)
            return pi
        return None

    def mip(self, name, key, samples, period):
        return self.sc.wave(name, key, *synth.wave_pyramid(samples), period)

    def big(self, i):
        sizes, data = _big(i)
        return self.be.wave_upload(0x42000 + i, synth.WWAVE, synth.LOOPED, 256, sizes, data)

    def captured(self, name, key, cap, pcm, period):
        """a wave the device builds from a capture; the oracle gets the same samples the host way"""
        sizes, data = synth.wave_pyramid((pcm >> 8).astype(np.int16))

        def upload(key, wtype, flags, period, sizes, data):
            if not self.gpu:
                return self.be.wave_upload(key, wtype, flags, period, sizes, data)
            self.pool.place(key, wtype, sizes)
            return self.be.wave_upload_captured(key, wtype, flags, period, sizes, cap)
        return self.sc.wave(name, key, sizes, data, period, upload)

    def drop(self, name):
        self.be.wave_drop(self.sc.keys[name])

    # -- batches --
    def _tame_want(self):
        """voices the kernel gives the tame bit in the batch about to be rendered: settled (born before it), both waves
        there, both levels tame, the 16 byte table there"""
        b, n = len(self.plan), 0
        for v in self.sc.osc2:
            if v["born"] is None:
                v["born"] = b
            live = all(k in self.pool.waves for k in v["keys"])
            if v["born"] < b and live and self.pool.coef4 and self.sc.rules.tame_rule(*map(int, v["tame"])):
                n += 1
        return n

    def _reports(self, frags):
        be, sc, b = self.be, self.sc, len(self.plan)
        if b == 0:
            return              # (the birth batch: every voice carries records)
        o2 = be.last_batch_osc2()
        assert (o2.launched, o2.voices) == (1, sc.nclass["osc2-pan"]), (b, o2)
        whole = _walks(frags, o2.ysplit)
        assert (o2.voice_major, o2.superchunks_voice_major, o2.superchunks_chunk_major) == \
            (1, sum(whole), len(whole) - sum(whole)), (b, o2, whole)
        o3 = be.last_batch_osc3filt()
        assert (o3.launched, o3.class_voices) == (1, sc.nclass["osc3-filter-pan"]), (b, o3)
        bare = be.last_batch_bare()
        assert (bare.launched, bare.class_voices) == (1, sc.nclass["osc"]), (b, bare)

    def batch(self, frags, between=None):
        assert 5 <= len(frags) <= MAXB
        for f, n in enumerate(frags):
            if between:
                between(f)
            self.sc.walk(n)
        want = self._tame_want()        # (by the tables as they stand when the batch is rendered)
        self.outs.append(self.be.render(sum(frags)).copy())
        self.pool.end_batch()
        if self.gpu:
            self._reports(frags)
            seen = self.be.osc2_tame_voices()
            if len(self.plan):
                assert seen - self.tame_seen == want, (len(self.plan), seen - self.tame_seen, want)
            self.tame_seen = seen
        self.plan.append(list(frags))
        self.check()

    def step(self, walk):
        """bench.py's step of MAXB fragments: one walked or none, the rest repeated; the render asynchronous on the
        product library and collected when the next but one is in flight"""
        if walk:
            self.sc.walk(64)
        self.be.fragment_repeat(64, MAXB - 1 if walk else MAXB)
        self.pool.open = True
        want = self._tame_want()
        self.tame_due += want if len(self.plan) else 0
        if self.gpu:
            before = launches(self.be)
            assert self.be._render(self.be.ctx, ASYNC, None, 0) == MAXB * 64, self.be.last_error()
            self.launches.append(launches(self.be) - before)
            self.inflight += 1
            if self.inflight == 2:
                self.collect(1)
        else:
            self.outs.append(self.be.render(MAXB * 64).copy())
        self.pool.end_batch()
        self.plan.append([64] * MAXB)

    def collect(self, count=2):
        while self.gpu and self.inflight and count:
            count -= 1
            out = np.zeros((2, MAXB * 64), dtype=np.int32)
            p = (C.POINTER(C.c_int32) * 2)(*[out[c].ctypes.data_as(C.POINTER(C.c_int32)) for c in range(2)])
            self.be.lib.a2amd_collect.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_int32)), C.c_uint]
            assert self.be.lib.a2amd_collect(self.be.ctx, p, MAXB * 64) == MAXB * 64, self.be.last_error()
            self.outs.append(out)
            self.inflight -= 1

    def finish(self):
        self.collect()
        if self.gpu and self.tame_due:
            assert self.be.osc2_tame_voices() - self.tame_seen == self.tame_due
        self.check("end")
        self.be.close()
        out = np.concatenate(self.outs, axis=1)
        out.setflags(write=False)
        return out


# ---- the cases' scripts --------------------------------------------------------------------------------------------------
SHORT = [64, 64, 37, 64, 64, 64, 64]


def _grow(r, at=None):
    """two plain waves of 4.3 M samples, a voice on each: the second does not fit the 8 388 608 samples"""
    r.check("before")
    assert r.pool.reallocs == 0
    wids = [r.big(0)]
    r.check("first")
    wids.append(r.big(1))
    r.check("after")
    for i, wid in enumerate(wids):
        r.sc.add("osc-pan", 200 + i, i, [wid], pitch=synth.fix(-0.5 + i))


def s_growth(r):
    """a, b: two batches, the pool grows, three more"""
    r.batch([64] * 6)
    r.batch([64] * 8)
    _grow(r)
    r.batch([64] * 5)
    r.batch(SHORT)
    r.batch([64] * 8)


def _cross(r):
    """one mip-mapped wave of 65 536 samples, a voice on it: with 2 MB the entries outgrow the budget"""
    r.check("before")
    wid = r.mip("P65536", 0x41000, _private(65536, 21), 256)
    r.check("after")
    r.sc.add("osc-pan", 210, 0, [wid], pitch=synth.fix(0.4))
    r.sc.add("osc2-filter-pan", 211, 2, [wid, r.sc.wave_ids[4]])


def s_cross(r):
    """c: the budget crossed without growth, between two settled batches on each side"""
    r.batch([64] * 6)
    r.batch([64] * 8)
    r.batch([64] * 5)
    _cross(r)
    r.batch(SHORT)
    r.batch([64] * 8)
    r.batch([64] * 6)


def s_open(event):
    def script(r):
        """d: the same event with three fragments of the batch recorded, the new voices born in the fourth"""
        r.batch([64] * 6)
        r.batch([64] * 8)
        r.batch(SHORT, between=lambda f: event(r) if f == 3 else None)
        r.batch([64] * 8)
    return script


def _neighbours(r):
    """case e's and h's waves, uploaded last and in this order: N1, V, N2 - N1's last level ends where V begins, N2's
    level 0 begins where V ends"""
    sc = r.sc
    r.mip("N1", 0x41001, _private(3001, 31), 65536)     # (a period of 65 536: played at its last levels)
    r.mip("V", 0x41002, _private(4096, 32), 4096)
    r.mip("N2", 0x41003, _private(3001, 33), 256)
    r.check("placed")
    n1, v, n2 = (r.pool.waves[sc.keys[n]] for n in ("N1", "V", "N2"))
    assert n1[0] + n1[1] == v[0] and v[0] + v[1] == n2[0] and n2[0] + n2[1] == r.pool.used
    sc.add("osc-pan", 300, 0, [sc.w["N1"][0]], pitch=sc.pitch("N1", 9, 1.4))
    sc.voice2((("N1", 9, 1.1), ("N1", 8, 1.7)), 301, 1)
    sc.add("osc-pan", 302, 1, [sc.w["N2"][0]], pitch=sc.pitch("N2", 0, 0.7))
    sc.voice2((("N2", 0, "hi"), ("N2", 1, 1.3)), 303, 2)


def _victims(r):
    """one voice of each class on V; of osc2 and osc3 voices one oscillator only"""
    sc, v, b = r.sc, r.sc.w["V"][0], r.sc.wave_ids
    sc.add("osc-pan", 310, 2, [v], pitch=sc.pitch("V", 0, 0.8))
    sc.voice2((("V", 6, 1.5), ("B64", 0, "hi")), 311, 0)        # 64 + 64 entries: both staged in LDS, tame
    sc.voice2((("A256", 0, "hi"), ("V", 5, 1.2)), 312, 1)       # 128 entries, the second oscillator: staged, tame
    sc.voice2((("V", 1, 1.6), ("A64", 0, 0.45)), 313, 2)        # 2 048 entries: gathered
    sc.add("osc-filter-pan", 314, 0, [v], pitch=sc.pitch("V", 0, 1.1))
    sc.add("osc2-filter-pan", 315, 1, [b[6], v])
    sc.add("osc3-filter-pan", 316, 2, [b[1], v, b[13]])
    sc.add("osc", 317, "mono", [v], pitch=sc.pitch("V", 1, 1.3))


def s_drop(r):
    """e: a wave dropped under every class; its region reused, filled and overrun beside playing neighbours"""
    sc = r.sc
    _neighbours(r)
    _victims(r)
    r.batch([64] * 6)
    r.batch([64] * 8)
    if "drop" not in r.without:
        r.drop("V")
        r.check("dropped")
    r.batch(SHORT)
    r.batch([64] * 8)
    s1 = r.mip("S1", 0x41004, _private(2048, 34), 2048)         # smaller than V: from the free list
    r.check("reused")
    # (the voices on a wave in the reused region start at its first sample and at even distances and, at 0.95 samples a
    # frame, read every entry of its level 0 in the 832 frames that follow: a stale entry anywhere in it is heard)
    for j in range(3):
        sc.add("osc-pan", 324 + j, j, [s1], pitch=sc.pitch("S1", 0, 0.95), phase=j * 65536 // 3)
    sc.voice2((("S1", 0, 1.1), ("S1", 4, 1.5)), 321, 1)
    s2 = r.mip("S2", 0x41005, _private(1024, 35), 1024)         # fits what is left of the region
    r.check("filled")
    s3 = r.mip("S3", 0x41006, _private(1500, 36), 256)          # does not: the end of the pool
    r.check("overrun")
    sc.add("osc-pan", 322, 2, [s2], pitch=sc.pitch("S2", 0, 0.95), phase=0)
    # (... and S2's first entry once more by a settled voice: the tenth fragment behind its birth, in the last batch)
    sc.add("osc-pan", 328, 1, [s2], pitch=sc.pitch_back_at("S2", 1024, 10), phase=0)
    sc.add("osc-pan", 327, 0, [s2], pitch=sc.pitch("S2", 0, 0.95), phase=32768)
    sc.add("osc-filter-pan", 323, 1, [s3], pitch=sc.pitch("S3", 0, 1.2))
    r.batch([64] * 5)
    r.batch([64] * 8)


def s_rekey(r):
    """f: the same key again, other data and another length - between batches under voices of three classes, and with
    three fragments recorded.  What is recorded plays the old data in the reference and the replaced descriptor here, so
    for the second only voices born after the upload name the wave."""
    sc = r.sc
    k = r.mip("K", 0x41010, _private(1500, 41), 1500)
    r.mip("K2", 0x41011, _private(1200, 42), 1200)
    sc.add("osc-pan", 400, 0, [k], pitch=sc.pitch("K", 0, 0.9))
    sc.voice2((("K", 0, 1.3), ("A64", 0, "hi")), 401, 1)
    sc.add("osc3-filter-pan", 402, 2, [sc.wave_ids[3], k, sc.wave_ids[8]])
    r.batch([64] * 6)
    r.batch([64] * 8)
    if "replace" not in r.without:
        assert r.mip("K", 0x41010, _private(2300, 43), 2300) == k
        r.check("replaced")
    r.batch([64] * 5)
    r.batch(SHORT)

    def again(f):
        if f != 3:
            return
        k2 = r.mip("K2", 0x41011, _private(500, 44), 500)
        r.check("replaced open")
        # (from the first sample, 0.9 samples a frame: every entry of level 0; and one whose tenth fragment behind this one,
        # in the next batch, begins on the first entry again)
        sc.add("osc-pan", 410, 1, [k2], pitch=sc.pitch("K2", 0, 0.9), phase=0)
        sc.add("osc-pan", 412, 2, [k2], pitch=sc.pitch_back_at("K2", 500, 10), phase=0)
        sc.add("osc2-filter-pan", 411, 0, [k2, sc.wave_ids[5]])
    r.batch([64] * 7, between=again)
    r.batch([64] * 8)


def s_inflight(r):
    """g: a step in flight; a wave it plays dropped, one of the same size uploaded into the region, a voice on it"""
    sc = r.sc
    _neighbours(r)              # (V between two waves: its region goes to the free list, not back to the pool's tail)
    sc.add("osc-pan", 310, 2, [sc.w["V"][0]], pitch=sc.pitch("V", 0, 0.8))
    sc.voice2((("V", 6, 1.5), ("B64", 0, "hi")), 311, 0)
    r.step(True)
    r.collect()
    r.step(False)               # (not collected)
    if "drop" not in r.without:
        r.drop("V")
        r.check("dropped")
        v2 = r.mip("V2", 0x41020, _private(4096, 37), 4096)
        r.check("reused")
        for j in range(9):      # (a step of 512 frames at 0.95 samples a frame from every ninth: every entry of level 0)
            sc.add("osc-pan", 330 + j, j % 3, [v2], pitch=sc.pitch("V2", 0, 0.95), phase=j * 65536 // 9)
    r.step(True)
    r.collect()


def s_graph(r):
    """g: the birth step, four identical quiet steps, case c's crossing, four more.  The readbacks alternate between two
    buffers and a graph is captured per buffer, so of identical quiet steps the first uploads, the second and third
    capture and the fourth is the first to be replayed: one step more behind the crossing than the three that find a
    graph again, so that a replay is seen there as well."""
    r.step(True)
    for _ in range(4):
        r.step(False)
    r.collect()
    r.check("before")
    r.mip("P65536", 0x41000, _private(65536, 21), 256)
    r.check("after")
    for _ in range(4):
        r.step(False)
    r.collect()


def _sub_render(be, frames=3000):
    """what the capture is made of: a few voices, `frames` frames of channel 0"""
    sc = synth.Scene(be)
    sc.root()
    sc.add_voices(12, chain="osc-filter-pan")
    pcm, left = [], frames
    while left:
        n = min(8 * 64, left)
        for f in range(0, n, 64):
            sc.walk(min(64, n - f))
        pcm.append(be.render(n).copy())
        left -= n
    return np.concatenate(pcm, axis=1)[0]


def s_captured(r):
    """h: a wave built on the device from a capture into the region a tame wave left, played by three osc2-pan voices (and three osc-pan voices over all of its level 0)"""
    sc = r.sc
    if r.gpu:
        sub = make_gpu(max_batch=MAXB)
        sub.capture_begin()
        pcm = _sub_render(sub)
        cap = sub.capture_end()
        sub.close()
    else:
        sub, cap = make_oracle(r.oracle_lib), None
        pcm = _sub_render(sub)
        sub.close()
    r.pcm = pcm
    _neighbours(r)
    sc.voice2((("V", 6, 1.5), ("B64", 0, "hi")), 311, 0)
    sc.add("osc-pan", 310, 2, [sc.w["V"][0]], pitch=sc.pitch("V", 0, 0.8))
    r.batch([64] * 6)
    r.batch([64] * 8)
    r.drop("V")
    r.check("dropped")
    r.batch([64] * 5)
    r.captured("C", 0x41030, cap, pcm, 64)
    r.check("reused")
    if cap:
        r.be.capture_free(cap)
    # (whatever its samples are, the kernel counts a wave the device made not tame: device_built)
    sc.voice2((("C", 5, 1.4), ("A64", 0, "hi")), 340, 1, device_built=("C",))
    sc.voice2((("A256", 0, 1.2), ("C", 6, 1.1)), 341, 2, device_built=("C",))
    sc.voice2((("C", 0, "hi"), ("C", 1, 1.1)), 345, 0, device_built=("C",))     # (from C's first sample: PHASES[345 % 8] is 0)
    for j in range(3):          # (... and every entry of its level 0 in the 1 317 frames that follow)
        sc.add("osc-pan", 346 + j, j, [sc.w["C"][0]], pitch=sc.pitch("C", 0, 0.95), phase=j * 65536 // 3)
    r.batch(SHORT)
    r.batch([64] * 8)
    r.batch([64] * 6)


CASES = {
    # name: (script, A2AMD_COEF_CACHE_MB, the cast without its gliding and cut voices, voices the script adds)
    # (g-graph-dropped: a batch is quiet - no records, no exception list - only without those two voices, and with the
    # cast's five osc2-filter-pan voices on their quiet kernel, which a scene this small gets with A2AMD_O2F_MIN=1)
    "a-growth-table-kept": (s_growth, 192, False, [200, 201]),
    "b-growth-table-dropped": (s_growth, 80, False, [200, 201]),
    "c-budget-crossed": (s_cross, 2, False, [210, 211]),
    "d-crossed-in-open-batch": (s_open(_cross), 2, False, [210, 211]),
    "d-grown-in-open-batch": (s_open(_grow), 192, False, [200, 201]),
    "e-drop-and-reuse": (s_drop, 192, False, [300, 301, 302, 303] + list(range(310, 318)) + [321, 322, 323, 324, 325, 326, 327, 328]),
    "f-same-key-again": (s_rekey, 192, False, [400, 401, 402, 410, 411, 412]),
    "g-in-flight": (s_inflight, 192, False, [300, 301, 302, 303, 310, 311] + list(range(330, 339))),
    "g-graph-dropped": (s_graph, 2, True, []),
    "h-captured-into-region": (s_captured, 192, False, [300, 301, 302, 303, 310, 311, 340, 341, 345, 346, 347, 348]),
}
_REF = {}


def _oracle(oracle_lib, name, skip=None, without=()):
    """the oracle's run of a case (or of a variant of it), made once"""
    key = (name, skip, tuple(without))
    if key not in _REF:
        script, mb, quiet, _ = CASES[name]
        r = _Run(make_oracle(oracle_lib), oracle_lib, mb, skip, without, quiet)
        script(r)
        r.out = r.finish()
        _REF[key] = r
    return _REF[key]


def _batches(r):
    starts = np.cumsum([0] + [sum(f) for f in r.plan])
    return [r.out[:, a:b] for a, b in zip(starts, starts[1:])]


# ---- the premises: the oracle and the model alone ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_premise_every_phase_is_audible_and_every_added_voice_counts(oracle_lib, name):
    base = _oracle(oracle_lib, name)
    assert len(base.plan) >= 3 and sum(37 in f for f in base.plan) == (0 if name.startswith("g") else 1)
    for b, out in enumerate(_batches(base)):
        assert np.abs(out).max(axis=1).min() > 256, (name, b)
    for k in CASES[name][3]:
        assert not np.array_equal(_oracle(oracle_lib, name, skip=k).out, base.out), (name, k)


def test_premise_every_voice_of_the_cast_counts(oracle_lib):
    base = _oracle(oracle_lib, "c-budget-crossed")
    cast = list(range(24)) + [100 + j for j in range(9)] + [110 + j for j in range(9)] + \
        [c + j for c in (120, 130, 140, 150) for j in range(5)] + [160, 161]
    assert 60 <= len(cast) <= 100 and base.sc.nvoices == len(cast) + 2
    for k in cast:
        assert not np.array_equal(_oracle(oracle_lib, "c-budget-crossed", skip=k).out, base.out), k


def test_premise_waves_are_what_the_cast_is_written_for(oracle_lib):
    sc, rules = _oracle(oracle_lib, "e-drop-and-reuse").sc, _rules()
    got = [int(rules.stage_rule(*m)) for m in sc.masks[:24]]
    assert got == [m for _, m, _ in CAST_OSC2 for _ in range(3)], got
    got = [int(rules.tame_rule(*map(int, t))) for t in sc.tame[:24]]
    assert got == [t for _, _, t in CAST_OSC2 for _ in range(3)], got
    # the victims: V's levels of 64 and 128 entries staged beside B64 / alone, its level of 2 048 gathered; all tame
    by_k = {v["k"]: (m, v["tame"]) for v, m in zip(sc.osc2, sc.masks)}
    assert [int(rules.stage_rule(*by_k[k][0])) for k in (311, 312, 313)] == [3, 2, 2]
    assert all(all(by_k[k][1]) for k in (311, 312, 313, 301, 303, 321))
    for name in ("P5000", "P4096", "P3001", "N1", "V", "N2", "S1", "S2", "S3"):
        assert all(p for p, _ in sc.flags[name]), name      # (looped, pads made by the loader: periodic)
    assert sc.w["P5000"][1][0] == 5000 and sc.w["P4096"][1][0] == 4096 and sc.w["P3001"][1][0] == 3001


def test_premise_sizes_put_the_pool_where_the_cases_say(oracle_lib):
    builtin = 24 * region(synth.WMIPWAVE, [2048 >> lv for lv in range(MIPLEVELS)])
    assert builtin == 129984
    for name in ("a-growth-table-kept", "b-growth-table-dropped", "d-grown-in-open-batch"):
        m = _oracle(oracle_lib, name).marks
        kept = name != "b-growth-table-dropped"
        assert m["before"]["used"] < m["first"]["used"] <= POOL0 < m["after"]["used"]
        assert (m["first"]["reallocations"], m["after"]["reallocations"], m["after"]["capacity"]) == (0, 1, 2 * POOL0)
        assert m["first"]["coef4"] == 1 and m["first"]["used"] * ENTRY <= m["first"]["budget"]
        assert m["after"]["coef4"] == kept == (m["after"]["used"] * ENTRY <= m["after"]["budget"])
        assert m["after"]["raw"] == (set() if kept else {P5000, P4096})
    for name in ("c-budget-crossed", "d-crossed-in-open-batch", "g-graph-dropped"):
        m = _oracle(oracle_lib, name).marks
        assert m["before"]["used"] * ENTRY <= m["before"]["budget"] == 2 << 20 < m["after"]["used"] * ENTRY
        assert (m["before"]["coef4"], m["before"]["raw_waves"]) == (1, 0) and m["after"]["used"] < POOL0
        assert m["after"]["coef4"] == 0 and m["after"]["raw"] == {P5000, P4096, 0x41000} and m["after"]["reallocations"] == 0
    m = _oracle(oracle_lib, "e-drop-and-reuse").marks
    v = m["placed"]["waves"][0x41002]
    assert m["dropped"]["free_samples"] == v[1] == region(synth.WMIPWAVE, [(4096 + (1 << lv) - 1) >> lv for lv in range(MIPLEVELS)])
    assert m["reused"]["regions_reused"] == 1 and m["reused"]["waves"][0x41004][0] == v[0]
    assert m["filled"]["regions_reused"] == 2 and m["filled"]["waves"][0x41005][0] == v[0] + m["reused"]["waves"][0x41004][1]
    assert 0 < m["filled"]["free_samples"] < region(synth.WMIPWAVE, [1500])
    assert m["overrun"]["regions_reused"] == 2 and m["overrun"]["waves"][0x41006][0] == m["filled"]["used"]
    m = _oracle(oracle_lib, "f-same-key-again").marks
    assert m["replaced"]["regions_reused"] == 0 and m["replaced"]["free_samples"] == 0      # (the old region: held for the batch)
    # ... and handed on after it: K2's new data lands where K's old data was, in front of K2's old
    assert m["replaced open"]["waves"][0x41011][0] < m["replaced"]["waves"][0x41011][0] < m["replaced"]["waves"][0x41010][0]
    assert m["replaced open"]["regions_reused"] == 1 and m["end"]["free_samples"] > 0
    for name in ("g-in-flight", "h-captured-into-region"):
        m = _oracle(oracle_lib, name).marks
        assert m["dropped"]["free_samples"] > 0 and m["reused"]["regions_reused"] == 1, name
    assert _oracle(oracle_lib, "g-in-flight").marks["reused"]["free_samples"] == 0          # (the same size: all of it)


@pytest.mark.parametrize("name,what,first", [("e-drop-and-reuse", "drop", 2), ("g-in-flight", "drop", 2),
                                             ("f-same-key-again", "replace", 2)])
def test_premise_drop_and_replacement_change_the_mix_from_their_batch_on(oracle_lib, name, what, first):
    base, other = _oracle(oracle_lib, name), _oracle(oracle_lib, name, without=(what,))
    same = [np.array_equal(a, b) for a, b in zip(_batches(base), _batches(other))]
    assert same == [b < first for b in range(len(same))], same


# ---- the cases on the device ---------------------------------------------------------------------------------------------------
def _gpu_case(oracle_lib, monkeypatch, name, win=None):
    script, mb, quiet, _ = CASES[name]
    want = _oracle(oracle_lib, name)
    for var in ("A2AMD_RAW", "A2AMD_DEBUG", "A2AMD_VPW", "A2AMD_YSPLIT"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("A2AMD_COEF_CACHE_MB", str(mb))
    if win is not None:
        monkeypatch.setenv("A2AMD_WIN", win)
    if name == "g-graph-dropped":
        monkeypatch.setenv("A2AMD_O2F_MIN", "1")
    r = _Run(make_gpu(max_batch=MAXB), oracle_lib, mb, quiet=quiet)
    script(r)
    got = r.finish()
    assert r.plan == want.plan and r.marks == want.marks
    _assert_batches_equal(got, want.out, want.plan)
    return r, want


@gpu
@pytest.mark.parametrize("name", ["a-growth-table-kept", "b-growth-table-dropped", "c-budget-crossed",
                                  "d-crossed-in-open-batch", "d-grown-in-open-batch"])
def test_growth_and_budget(oracle_lib, monkeypatch, name):
    """a - d.  The pool is reallocated and its tables rebuilt, or its entries outgrow the budget - the 16 byte table
    freed, the large mip-mapped waves flagged raw - between two settled batches or with three fragments recorded: the
    event is the model's (a2amd_wave_pool_info at every mark), the tame voices take the fused steps while and only
    while the table exists, every batch is the oracle's."""
    r, _ = _gpu_case(oracle_lib, monkeypatch, name)
    m = r.marks
    if "growth" in name or "grown" in name:
        assert (m["before"]["reallocations"], m["after"]["reallocations"]) == (0, 1)
        assert m["after"]["coef4"] == (name != "b-growth-table-dropped")
    else:
        assert (m["before"]["coef4"], m["before"]["raw_waves"], m["after"]["coef4"], m["after"]["raw_waves"]) == (1, 0, 0, 3)


@gpu
@pytest.mark.parametrize("win", ["1", "0"])
@pytest.mark.parametrize("name", ["e-drop-and-reuse", "f-same-key-again"])
def test_reuse(oracle_lib, monkeypatch, name, win):
    """e, f, with the window kernels and with the records kernels.  A wave dropped under one voice of every class -
    the tame count falls by exactly those voices - its region served from the free list to a smaller wave, filled by a
    second and overrun by a third while the waves on both sides of it play; a key uploaded again under its voices."""
    r, _ = _gpu_case(oracle_lib, monkeypatch, name, win)
    assert r.marks["end"]["regions_reused"] == (2 if name.startswith("e") else 1)


@gpu
def test_in_flight(oracle_lib, monkeypatch):
    """g.  A step rendered asynchronously and not collected; a wave it plays is dropped and one of the same size
    uploaded into its region (wave_place waits for the stream), a voice started on it, the next step rendered, both
    collected."""
    r, _ = _gpu_case(oracle_lib, monkeypatch, "g-in-flight")
    assert r.marks["reused"]["regions_reused"] == 1 and r.marks["reused"]["free_samples"] == 0


@gpu
def test_graph_dropped_at_the_crossing_and_found_again(oracle_lib, monkeypatch):
    """g.  Identical quiet steps are replayed from a captured graph - no kernel launch of the library's own - the budget
    crossing drops it (the kernels take the table's address as an argument), and the steps behind it find one again."""
    r, _ = _gpu_case(oracle_lib, monkeypatch, "g-graph-dropped")
    print(r.launches)
    assert [n > 0 for n in r.launches] == [True] + [True, True, True, False] * 2, r.launches


@gpu
def test_captured_wave_in_a_reused_region(oracle_lib, monkeypatch):
    """h.  A wave the device builds from a capture lands in the region a tame wave left; its osc2-pan voices render
    like the oracle's on the same samples uploaded the host way, and are not counted tame."""
    r, want = _gpu_case(oracle_lib, monkeypatch, "h-captured-into-region")
    assert np.array_equal(r.pcm, want.pcm)      # (what was captured is what the oracle's wave was made of)
    assert r.marks["reused"]["regions_reused"] == 1
