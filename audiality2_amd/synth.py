"""Synthetic workloads for the tests and bench.py.

Host-side helpers that play the role of the Audiality 2 engine for a fixed,
scripted voice tree: they prepare wave data the way the engine's wave loader
does (src/waves.c:59-130: mip levels + pad samples) and issue the unit
callbacks (Initialize / write / Process) in the order the engine's voice walk
would (src/core.c:1847-1896) against any backend that speaks the call protocol
of include/a2amd.h.  Workload shapes follow BASELINE.json / SURVEY.md 8(d).
"""
import numpy as np

from .replay import WAVEPOST, WAVEPRE, MIPLEVELS

K_WTOSC, K_PANMIX, K_FILTER12, K_FBDELAY, K_INLINE, K_XINSERT = range(6)
# the FM oscillators (a2amd_unitkind): name -> (kind, operators)
FM_KINDS = {"fm1": (6, 1), "fm2": (7, 2), "fm3": (8, 3), "fm4": (9, 4),
            "fm3p": (10, 3), "fm4p": (11, 4), "fm2r": (12, 2), "fm4r": (13, 4)}
PROCADD = 1
WOFF, WNOISE, WWAVE, WMIPWAVE = range(4)
LOOPED = 0x100
NORMALIZE, XFADE, REVMIX = 0x10000, 0x40000, 0x80000    # A2_waveflags, include/a2_waves.h:113-115
WAVEPERIOD = 2048


def basepitch_for(samplerate):
    """A2_config.basepitch, src/audiality2.c:398: log2(261.626/rate) in 16:16."""
    f = np.float32(261.626) / np.float32(samplerate)
    p = np.float32(np.log2(np.float64(f)))
    return int(np.float32(p * np.float32(65536.0) + np.float32(0.5)))


def fix(x):
    """float -> 16:16 like the engine's API conversion (truncation)."""
    return int(x * 65536.0)


def wave_pyramid(samples, looped=True, levels=MIPLEVELS):
    """Mip pyramid with pads as the engine's wave loader builds it
    (a2_wave_alloc / a2_fix_pad / a2_render_mipmaps, src/waves.c:59-130).
    Returns (sizes, [int16 array per level incl. pads])."""
    src = np.asarray(samples, dtype=np.int16)
    length = len(src)
    sizes, data = [], []
    prev = None
    for lv in range(levels):
        size = (length + (1 << lv) - 1) >> lv
        buf = np.zeros(WAVEPRE + size + WAVEPOST, dtype=np.int16)
        if lv == 0:
            buf[WAVEPRE:WAVEPRE + size] = src
        else:
            p = prev.astype(np.int32)
            k = np.arange(size)
            # d[s] = (2*sd[2s] + sd[2s-1] + sd[2s+1]) >> 2, sd = previous payload
            buf[WAVEPRE:WAVEPRE + size] = ((p[WAVEPRE + 2 * k] << 1) + p[WAVEPRE + 2 * k - 1]
                                           + p[WAVEPRE + 2 * k + 1]) >> 2
        if looped and size:
            buf[0] = buf[size]
            idx = np.arange(WAVEPOST) % size
            buf[WAVEPRE + size:] = buf[WAVEPRE + idx]
        sizes.append(size)
        data.append(buf)
        prev = buf
    return sizes, data


def wave_postprocess(pcm, chunk, flags):
    """Level 0 (int16, no pads) of a wave that was written as A2_I24 samples `pcm`, `chunk` frames per write, the
    way the engine makes it when the stream closes (src/waves.c:155-346, 405-451): with NORMALIZE the smallest of
    the writes' gains 32767 * 256 / peak, 1000 at most, and the float conversion unless that gain is exactly 1;
    with XFADE the triangular window, the overlap-add and the copy of the first half.  Every operation in the
    reference's types (np.float32 / np.float64), one by one."""
    x = np.asarray(pcm, dtype=np.int32)
    n = len(x)
    f32, f64 = np.float32, np.float64
    if flags & REVMIX:
        raise ValueError("revmix: the reference's result reads an unwritten pad sample")
    if flags & XFADE and n < 2:
        raise ValueError("xfade needs two samples")
    gain = f32(1.0)
    if flags & NORMALIZE:
        if not chunk:
            raise ValueError("normalize needs the size of the writes")
        gain = f32(1000.0)
        with np.errstate(over="ignore"):
            mag = np.maximum(x, -x)                       # (the negation wraps: INT32_MIN stays negative)
        for lo in range(0, n, chunk):
            peak = max(0, int(mag[lo:lo + chunk].max()))
            bg = f32(8388352.0) / f32(peak) if peak else f32(1.0)
            if bg < gain:
                gain = bg
    if gain == f32(1.0):
        d = (x >> 8).astype(np.int16)
    else:
        g2 = gain / f32(256.0)
        p = x.astype(np.float32) * g2                     # (float32 array * float32 scalar: a float32 multiply)
        t = np.trunc(p.astype(np.float64))
        fits = (t > -2147483649.0) & (t < 2147483648.0)   # (cvttss2si: 0x80000000 for what does not fit)
        d = np.where(fits, t, -2147483648.0).astype(np.int64).astype(np.int32).astype(np.int16)
    if flags & XFADE:
        sh = n // 2
        dg = f64(f32(1.0) / f32(sh))
        i = np.arange(n, dtype=np.int64)
        g = np.where(i < sh, i, 2 * sh - i).astype(np.float64) * dg     # (= the reference's running sum, exactly)
        d = np.trunc(d.astype(np.float64) * g).astype(np.int64).astype(np.int16)
        with np.errstate(over="ignore"):
            d[:sh] = d[:sh] + d[sh:2 * sh]                # (int16 addition wraps)
        d[sh:2 * sh] = d[:sh]
        if n & 1:
            d[n - 1] = d[0]                               # (the copy loop runs upwards: d[2 sh] = new d[sh] = d[0])
    return d


def test_waves(count=24):
    """`count` band-rich looped single-cycle waves, period 2048 (the size and
    kind of the engine's built-in geometric waves; our own shapes)."""
    n = np.arange(WAVEPERIOD)
    out = []
    for i in range(count):
        kind = i % 4
        if kind == 0:      # pulse with duty depending on i
            duty = (i // 4 + 1) * WAVEPERIOD // 16
            w = np.where(n < duty, 32767, -32767)
        elif kind == 1:    # saw
            w = n * 65534 // WAVEPERIOD - 32767
        elif kind == 2:    # triangle
            t = np.where(n < WAVEPERIOD // 2, n, WAVEPERIOD - 1 - n)
            w = t * 65534 * 2 // WAVEPERIOD - 32767
        else:              # sine with i-dependent harmonic
            h = i // 4 + 1
            w = (np.sin(n * 2.0 * np.pi * h / WAVEPERIOD) * 32767.0).astype(np.int64)
        out.append(np.asarray(w, dtype=np.int16))
    return out


class Scene:
    """A scripted voice tree driven through the unit callbacks."""

    def __init__(self, backend, nwaves=24):
        self.be = backend
        self.next_key = 1
        self.wave_ids = []
        for i, w in enumerate(test_waves(nwaves)):
            sizes, data = wave_pyramid(w)
            self.wave_ids.append(backend.wave_upload(0x100 + i, WMIPWAVE, LOOPED, WAVEPERIOD,
                                                     sizes + [0] * (MIPLEVELS - len(sizes)), data))
        self.noise_id = backend.wave_upload(0x50, WNOISE, LOOPED, 256, [0] * MIPLEVELS, [])
        self.rootv = None
        self.groups = []          # each: dict(units=[inline, d1, d2], leaves=[...])
        self.leaves = []          # leaves directly under the root
        self.nvoices = 0

    def _key(self):
        k = self.next_key
        self.next_key += 1
        return k

    def private_waves(self, count, length=65536, period=256, seed=7):
        """`count` looped, mip-mapped sample waves of `length` samples each that no two voices need share -
        SURVEY 8(d)'s "private sample wave" case: the waves of a sampler, not the 24 built-in cycles that sit
        in L2.  Deterministic content (a seeded random walk, band-limited a little), uploaded like
        a2_UploadWave's result (src/waves.c:155-237: all mip levels, pads).  Voices made by add_voices(...,
        private=True) play wave (voice number mod count)."""
        rng = np.random.default_rng(seed)
        base = rng.integers(-3000, 3001, size=length + 4096, dtype=np.int32)
        base = np.cumsum(base)
        base -= (np.arange(len(base)) * (base[-1] // len(base)))     # (no drift)
        base = (base * (28000.0 / max(1, np.abs(base).max()))).astype(np.int16)
        self.private_ids = []
        for i in range(count):
            # every wave a different stretch / polarity / level of the walk: distinct data, cheap to make
            off = (i * 977) % 4096
            w = base[off:off + length].astype(np.int32)
            if i & 1:
                w = -w
            w = (w * (0.5 + 0.5 * ((i * 37) % 64) / 63.0)).astype(np.int16)
            w[-64:] = (w[-64:].astype(np.int32) * np.arange(63, -1, -1) // 64 + w[:64].astype(np.int32) * np.arange(64) // 64).astype(np.int16)
            sizes, data = wave_pyramid(w)
            self.private_ids.append(self.be.wave_upload(0x10000 + i, WMIPWAVE, LOOPED, period,
                                                        sizes + [0] * (MIPLEVELS - len(sizes)), data))
        return self.private_ids

    # -- tree construction (what a2_PopulateVoice + the voice's first VM run do) --
    def root(self, channels=2):
        """a2_rootdriver (audiality2.c:271-280): inline 0 *; panmix * *; xinsert * >"""
        be, k = self.be, self._key()
        self.rootv = [be.unit_init(k, K_INLINE, 0, 0, channels, 0),
                      be.unit_init(k, K_PANMIX, 0, channels, channels, 0),
                      be.unit_init(k, K_XINSERT, PROCADD, channels, channels, 1)]
        return self.rootv

    # the two delays of benchmark/fmtest4.a2s:83-95 (tempo 120 4: a tick is 125 ms):
    # (fbdelay, ldelay, rdelay) in ms and (fbgain, lgain, rgain)
    FMTEST4 = (((631.25, 756.25, 1003.75), (0.03, 0.05, 0.05)),
               ((868.75, 1126.25, 1378.75), (0.03, 0.05, 0.05)))

    def add_group(self, fb=(63.1, 75.6, 100.4), gains=(0.3, 0.25, 0.25), preset=None, delays=2, mid_add=False,
                  parent=None, tail=None):
        """inline 0 *; fbdelay * *; fbdelay * >   (benchmark/fmtest4.a2s shape);
        preset="fmtest4": that song's own delay times and gains (BASELINE configs[3]).
        delays: fbdelay units in the chain, positions 0 .. delays - 1 - the last one wired and adding, the others in
        place.  mid_add: which of the others add to what they read instead of replacing it - True: the ones between the
        first and the last, positions 1 .. delays - 2; or the positions themselves, of 0 .. delays - 2.
        fb / gains: one triple for every delay, or a list with a triple per delay (the preset has two).
        parent: the bus or delay group that holds this one, instead of the root.
        tail="panmix": the master section of the reference's songs, inline 0 2; fbdelay 2 2 x delays; panmix+ 2 > 2 -
        no delay wired (mid_add: any of positions 0 .. delays - 1), the panmix wired and adding; `units` ends in it."""
        if tail not in (None, "panmix"):
            raise ValueError(f"tail {tail!r}")
        if delays < 1:
            raise ValueError("a delay group has at least one delay")
        if preset == "fmtest4" and delays != len(self.FMTEST4):
            raise ValueError(f"preset fmtest4 is a chain of {len(self.FMTEST4)} delays")
        for what in (fb, gains):
            if isinstance(what, list) and len(what) != delays:
                raise ValueError(f"{len(what)} triples for {delays} delays")
        inplace = delays if tail else delays - 1        # the delays that are not wired
        if mid_add not in (True, False, None) and not set(mid_add) <= set(range(inplace)):
            raise ValueError(f"mid_add positions are 0 .. {inplace - 1}")
        be, k = self.be, self._key()
        if mid_add is True:
            mid_add = range(1, delays - 1)
        adding = set(mid_add or ())
        u = [be.unit_init(k, K_INLINE, 0, 0, 2, 0)]
        u += [be.unit_init(k, K_FBDELAY, PROCADD if i in adding else 0, 2, 2, 0) for i in range(inplace)]
        u.append(be.unit_init(k, K_PANMIX if tail else K_FBDELAY, PROCADD, 2, 2, 1))
        for i, d in enumerate(u[1:1 + delays]):
            if preset == "fmtest4":
                dfb, dg = self.FMTEST4[i]
            else:
                dfb = fb[i] if isinstance(fb, list) else fb
                dg = gains[i] if isinstance(gains, list) else gains
            for reg, ms in enumerate(dfb):
                be.unit_write(d, reg, fix(ms))
            be.unit_write(d, 4, fix(dg[0]))
            be.unit_write(d, 5, fix(dg[1]))
            be.unit_write(d, 6, fix(dg[2]))
        g = dict(units=u, leaves=[])
        (self.groups if parent is None else parent.setdefault("subs", [])).append(g)
        return g

    def add_bus_group(self, parent=None):
        """A group voice as a2_NewGroup makes it (src/interface.c:888: the program
        a2_groupdriver, audiality2.c:292-302): inline 0 *; panmix * *; xinsert * > -
        under the root voice, under another such group or under a delay group (add_group)."""
        be, k = self.be, self._key()
        u = [be.unit_init(k, K_INLINE, 0, 0, 2, 0),
             be.unit_init(k, K_PANMIX, 0, 2, 2, 0),
             be.unit_init(k, K_XINSERT, PROCADD, 2, 2, 1)]
        g = dict(units=u, leaves=[], subs=[])
        (self.groups if parent is None else parent.setdefault("subs", [])).append(g)
        return g

    def add_mono_group(self, parent=None, pan=None, xinsert=False):
        """A mono group as `struct { inline; panmix }` compiles: inline 0 1; panmix+ 1 > 2, one channel panned into its
        parent's stereo bus - add_bus_group with a mono bus of its own.  pan: written to the panmix when given.
        xinsert: the three-unit shape, inline 0 1; panmix 1 2; xinsert+ 2 >."""
        be, k = self.be, self._key()
        if xinsert:
            u = [be.unit_init(k, K_INLINE, 0, 0, 1, 0),
                 be.unit_init(k, K_PANMIX, 0, 1, 2, 0),
                 be.unit_init(k, K_XINSERT, PROCADD, 2, 2, 1)]
        else:
            u = [be.unit_init(k, K_INLINE, 0, 0, 1, 0),
                 be.unit_init(k, K_PANMIX, PROCADD, 1, 2, 1)]
        if pan is not None:
            be.unit_write(u[1], 1, fix(pan))
        g = dict(units=u, leaves=[], subs=[])
        (self.groups if parent is None else parent.setdefault("subs", [])).append(g)
        return g

    def add_voices(self, n, chain="osc-pan", group=None, total=None, private=False):
        """n sustained voices with the per-voice parameters of SURVEY.md 8(d):
        wave 7k mod 24, pitch ((k mod 61)-30)/12 oct, pan ((k mod 17)-8)/8 ..."""
        be = self.be
        total = total or n
        amp = max(1, (4 << 16) // max(total, 1))
        dst = self.leaves if group is None else group["leaves"]
        for _ in range(n):
            k = self.nvoices
            self.nvoices += 1
            key = self._key()
            p = fix(((k % 61) - 30) / 12.0)
            units = []
            if chain == "osc":
                # `struct { wtosc }`: the oscillator alone, wired and adding - channel 0 of the parent's bus, no pan
                units = [be.unit_init(key, K_WTOSC, PROCADD, 0, 1, 1)]
                oscs, pan = [units[0]], None
            elif chain == "osc-pan":
                units = [be.unit_init(key, K_WTOSC, 0, 0, 1, 0),
                         be.unit_init(key, K_PANMIX, PROCADD, 1, 2, 1)]
                oscs, pan = [units[0]], units[1]
            elif chain == "osc-filter-pan":
                units = [be.unit_init(key, K_WTOSC, 0, 0, 1, 0),
                         be.unit_init(key, K_FILTER12, 0, 1, 1, 0),
                         be.unit_init(key, K_PANMIX, PROCADD, 1, 2, 1)]
                oscs, pan = [units[0]], units[2]
                be.unit_write(units[1], 0, p + fix(2.0))      # cutoff
                be.unit_write(units[1], 1, fix(5.0))          # q
            elif chain == "osc2-filter-pan":
                units = [be.unit_init(key, K_WTOSC, 0, 0, 1, 0),
                         be.unit_init(key, K_WTOSC, PROCADD, 0, 1, 0),
                         be.unit_init(key, K_FILTER12, 0, 1, 1, 0),
                         be.unit_init(key, K_PANMIX, PROCADD, 1, 2, 1)]
                oscs, pan = units[:2], units[3]
                be.unit_write(units[2], 0, p + fix(2.5))      # cutoff
                be.unit_write(units[2], 1, fix(3.0))          # q
            elif chain == "osc3-filter-pan":
                # `struct { wtosc; wtosc o2; wtosc o3; filter12; panmix }`: the three-oscillator subtractive lead
                units = [be.unit_init(key, K_WTOSC, 0, 0, 1, 0),
                         be.unit_init(key, K_WTOSC, PROCADD, 0, 1, 0),
                         be.unit_init(key, K_WTOSC, PROCADD, 0, 1, 0),
                         be.unit_init(key, K_FILTER12, 0, 1, 1, 0),
                         be.unit_init(key, K_PANMIX, PROCADD, 1, 2, 1)]
                oscs, pan = units[:3], units[4]
                be.unit_write(units[3], 0, p + fix(2.5))      # cutoff
                be.unit_write(units[3], 1, fix(3.0))          # q
            elif chain == "osc2-pan":
                units = [be.unit_init(key, K_WTOSC, 0, 0, 1, 0),
                         be.unit_init(key, K_WTOSC, PROCADD, 0, 1, 0),
                         be.unit_init(key, K_PANMIX, PROCADD, 1, 2, 1)]
                oscs, pan = units[:2], units[2]
            elif chain.endswith("-pan") and (chain[:-4] in FM_KINDS or chain == "fmmix-pan"):
                # fmN; panmix.  "fmmix" cycles through the eight units.
                name = sorted(FM_KINDS)[k % 8] if chain == "fmmix-pan" else chain[:-4]
                kind, nops = FM_KINDS[name]
                units = [be.unit_init(key, kind, 0, 0, 1, 0, wakefrac=(k * 37) & 255),
                         be.unit_init(key, K_PANMIX, PROCADD, 1, 2, 1)]
                oscs, pan = [], units[1]
                fm = units[0]
                ring = name.endswith("r")
                be.unit_write(fm, 1, p)                                   # p
                # a (ramping in every fourth voice), fb
                be.unit_write(fm, 2, fix(1.0) if ring else amp)
                if k % 4 == 0:
                    be.unit_write(fm, 2, (fix(1.0) if ring else amp) // 2, 0, 3000 << 8)
                be.unit_write(fm, 3, fix((k % 5) / 8.0))
                ratios = (1.0 + (k % 3) * 0.5, 2.01, (k % 7) * 0.5 + 0.5)
                depths = (0.5 + (k % 4) * 0.25, 0.7, 0.4)
                fbs = ((k % 3) / 4.0, 0.2, (k % 2) * 0.5)
                for j in range(1, nops):
                    be.unit_write(fm, 1 + 3 * j, fix(ratios[j - 1]))      # pN (relative)
                    be.unit_write(fm, 2 + 3 * j, amp if (ring and j == 1) else fix(depths[j - 1]))
                    be.unit_write(fm, 3 + 3 * j, fix(fbs[j - 1]))
                if k % 8 == 3:
                    be.unit_write(fm, 1, p + fix(0.5), 0, 1500 << 8)      # pitch glide
                be.unit_write(fm, 0, (k * 2654435761) % 65536)            # phase
            elif chain in ("noise-pan", "noise-filter-pan", "noisefilt-pan"):
                # wtosc playing the noise generator (the engine's 'noise' wave).  Pitches from -2 to +8 octaves:
                # a phase increment of 1 << 23 - a draw in every frame - is reached 6.5 octaves up at 48 kHz, so
                # five voices of 31 draw in every frame and the others hold a draw for several (wtosc.c:140-145)
                p = fix(((k * 7) % 31) / 3.0 - 2.0)
                units = [be.unit_init(key, K_WTOSC, 0, 0, 1, 0)]
                if chain == "noisefilt-pan":
                    # wtosc (noise); filter12; panmix as a2_PopulateVoice leaves it - the whole chain before the first
                    # write: ONE voice of the launch class wtosc-filter12-panmix (hats, snares, cymbals)
                    units.append(be.unit_init(key, K_FILTER12, 0, 1, 1, 0))
                    units.append(be.unit_init(key, K_PANMIX, PROCADD, 1, 2, 1))
                if chain != "noise-pan":
                    # ("noise-filter-pan" writes between its Initialize calls, which ends the voice being built: to a backend
                    # its panmix is a voice of its own behind a voice wtosc; filter12 - two voices of the general kernel)
                    if chain == "noise-filter-pan":
                        units.append(be.unit_init(key, K_FILTER12, 0, 1, 1, 0))
                    be.unit_write(units[1], 0, fix(1.0 + (k % 5) * 0.5))  # cutoff
                    be.unit_write(units[1], 1, fix(4.0))                  # q
                if chain != "noisefilt-pan":
                    units.append(be.unit_init(key, K_PANMIX, PROCADD, 1, 2, 1))
                oscs, pan = [], units[-1]
                be.unit_write(units[0], 0, self.noise_id)
                be.unit_write(units[0], 1, p)
                be.unit_write(units[0], 2, amp)
                be.unit_write(units[0], 3, (k * 2654435761) % 65536)      # phase: up to 2^32, any residue of 1 << 23
            else:
                raise ValueError(chain)
            for j, o in enumerate(oscs):
                be.unit_write(o, 0, self.private_ids[(k + j) % len(self.private_ids)] if private else
                              self.wave_ids[(7 * k + j) % len(self.wave_ids)])
                # (a third oscillator: an octave down)
                be.unit_write(o, 1, p - fix(1.0) if j == 2 else p + (fix(0.01) if j == 0 else -fix(0.01)) * (len(oscs) > 1))
                be.unit_write(o, 2, amp)
                be.unit_write(o, 3, (k * 2654435761) % 65536)
            if pan is not None:
                be.unit_write(pan, 1, fix(((k % 17) - 8) / 8.0))
            dst.append(units)

    # -- the engine's per-fragment voice walk (core.c:1847-1896), all VMs asleep --
    def walk(self, frames=64):
        be = self.be
        be.fragment(frames)
        if self.rootv:
            be.unit_process(self.rootv[0], 0, frames)
        def walk_group(g):
            be.unit_process(g["units"][0], 0, frames)
            for sub in g.get("subs", ()):
                walk_group(sub)
            for units in g["leaves"]:
                for u in units:
                    be.unit_process(u, 0, frames)
            be.inline_end(g["units"][0])
            for u in g["units"][1:]:
                be.unit_process(u, 0, frames)

        for g in self.groups:
            walk_group(g)
        for units in self.leaves:
            for u in units:
                be.unit_process(u, 0, frames)
        if self.rootv:
            be.inline_end(self.rootv[0])
            be.unit_process(self.rootv[1], 0, frames)
            be.unit_process(self.rootv[2], 0, frames)

    def run(self, fragments, batch=64, frames=64):
        """Walk `fragments` fragments, rendering every `batch`; returns int32
        [channels, fragments*frames]."""
        outs, pending = [], 0
        for _ in range(fragments):
            self.walk(frames)
            pending += 1
            if pending == batch:
                outs.append(self.be.render(pending * frames))
                pending = 0
        if pending:
            outs.append(self.be.render(pending * frames))
        return np.concatenate(outs, axis=1)
