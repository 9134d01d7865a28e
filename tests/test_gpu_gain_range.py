"""Every kernel's fixed point against the oracle OUTSIDE the musical range.

The signal path is 8.24 in int32 and every control register a 16.16 script value shifted left by 8; the reference clamps
none of them, it wraps.  The settled pan / volume gains and their clamp are stated once, in csrc/a2amd_settled.h
(tests/test_settled_header.py holds that statement to the reference's lines), and this file pins every kernel that calls
it; the per-frame gains, the amplitude product, the filter's output mix, the delay gains and the FM operator products are
still restated kernel by kernel.  Several of these rest on range arguments
(24-bit multiplies of a split gain, precomputed v0 / v1 / lim) that the other test files never leave: their gains are
positive and of musical size.  Here the gain registers - and only those: what becomes an address (pitch, phase, wave,
delay time, cutoff) stays where the other tests keep it - are negative, beyond +-1, at the values whose `<< 1` and
`<< 8` wrap and on both sides of the pan clamp's threshold.

Every GPU test renders one script on the oracle and on the GPU, compares the audio bit for bit, batch by batch, and
asserts who rendered (a2amd_last_batch, a2amd_last_batch_buses, a2amd_last_batch_noise[_filter]).  The tests without the
gpu mark state on the oracle / in numpy what the scripts are built on."""
import numpy as np
import pytest

from audiality2_amd import synth
from conftest import make_gpu, make_oracle
from gain_cases import GAINS, ONE
from test_gpu_bus_paths import Ramper, batch_starts, first_diff
from test_gpu_parity import last_batch
from test_noise_filt_quiet import FiltScene
from test_noise_filt_quiet import N_OTHER as NF_OTHER, N_PAN as NF_PAN
from test_noise_quiet import QuietScene
from test_noise_repeat import SEED0

fix = synth.fix
VOL, PAN = 0, 1                                  # panmix registers
A = 2                                            # wtosc 'a'
Q, LP, BP, HP = 1, 2, 3, 4                       # filter12 registers
DRY, FBG, LG, RG = 3, 4, 5, 6                    # fbdelay gain registers
WT = ("osc-pan", "osc2-pan", "osc-filter-pan", "osc2-filter-pan")
N = 131                                          # two full wavefronts of voices and a partial one

# (q, lp, bp, hp) by voice number mod 7
FILT = [
    (0, fix(127.0), fix(-127.0), fix(77.0)),
    (300, fix(-127.0), fix(127.0), fix(-127.0)),         # below 512: (65536 << 8) / q would not fit
    (fix(-5.0), fix(1.0), fix(0.5), fix(-0.25)),
    (fix(30000.0), fix(127.0), fix(127.0), fix(127.0)),
    (fix(0.001), fix(-1.0), 0, 0),
    (fix(4.0), fix(100.0), fix(-100.0), fix(127.5)),
    (fix(100.0), fix(-127.0), fix(-127.0), fix(-127.0)),
]
# per FM operator (a, fb), operator j of voice k takes FM[(k + 2 * j) % 5]; a ring unit's product is loud either way
FM = [(fix(100.3), fix(99.7)), (fix(120.1), fix(-100.6)), (fix(-127.2), fix(127.4)), (fix(300.0), fix(-127.9)),
      (fix(-0.8), fix(1.7))]
DELAY_GAINS = ((DRY, fix(127.0)), (FBG, fix(-40.0)), (LG, fix(100.0)), (RG, fix(-127.0)))
# taps of a fragment and more (k_bus_fbdchain's); the times are the ones test_gpu_parity's delay groups use
TAPS3 = [(63.1, 75.6, 100.4), (137.9, 63.1, 75.6), (100.4, 137.9, 63.1)]


def w32(x):
    """int32 wrap-around"""
    return ((int(x) + 2 ** 31) % 2 ** 32) - 2 ** 31


def make_loud(be, units, chain, k):
    """the gain registers of leaf voice number k, from the tables"""
    a, vol, pan = GAINS[k % len(GAINS)]
    if chain.startswith("fm"):
        fm, nops = units[0], synth.FM_KINDS[sorted(synth.FM_KINDS)[k % 8] if chain == "fmmix-pan" else chain[:-4]][1]
        for j in range(nops):
            oa, ofb = FM[(k + 2 * j) % len(FM)]
            be.unit_write(fm, 2 + 3 * j, oa)             # (without a duration: add_voices' amplitude ramps end here)
            be.unit_write(fm, 3 + 3 * j, ofb)
    else:
        nosc = 2 if chain.startswith("osc2") else 1
        for j in range(nosc):
            be.unit_write(units[j], A, a if j == 0 else GAINS[(k + 3) % len(GAINS)][0])
        if "filt" in chain:
            q, lp, bp, hp = FILT[k % len(FILT)]
            for reg, val in ((Q, q), (LP, lp), (BP, bp), (HP, hp)):
                be.unit_write(units[nosc], reg, val)
    be.unit_write(units[-1], VOL, vol)
    be.unit_write(units[-1], PAN, pan)


def loud_scene(be, chain, n=N):
    """Root (a driver) -> delay group of one delay, delay group of three, bus group (a driver), leaves: a quarter of
    the n voices of `chain` in each.  Every leaf's, every delay's and both drivers' gains from the tables."""
    sc = synth.Scene(be)
    sc.root()
    g1 = sc.add_group(delays=1)
    g3 = sc.add_group(fb=TAPS3, delays=3)
    bus = sc.add_bus_group()
    for g, cnt in ((g1, n // 4), (g3, n // 4), (bus, n // 4), (None, n - 3 * (n // 4))):
        sc.add_voices(cnt, chain=chain, group=g, total=n)
    k = 0
    for leaves in (g1["leaves"], g3["leaves"], bus["leaves"], sc.leaves):
        for units in leaves:
            make_loud(be, units, chain, k)
            k += 1
    assert k == n
    for g in (g1, g3):
        for d in g["units"][1:]:
            for reg, val in DELAY_GAINS:
                be.unit_write(d, reg, val)
    be.unit_write(sc.rootv[1], VOL, fix(-3.0))
    be.unit_write(sc.rootv[1], PAN, fix(-1.25))
    be.unit_write(bus["units"][1], VOL, fix(64.0))
    be.unit_write(bus["units"][1], PAN, ONE + 1)
    return sc, bus


# batch 0 takes the births, batch 1 is settled; in front of batch 2 both drivers are written (ramps of 700 frames: their
# own batch by records, then one batch on k_bus_driver's launch of one workgroup a voice); batch 4 is settled again
RAMP_AT, RAMP_FRAMES = 2, 700
PLANS = {"64": [[64] * 8] * 5, "37": [[37] * 8] * 2}


def class_script(be, chain, plan, info=None):
    sc, bus = loud_scene(be, chain)
    chunks = []
    for b, frags in enumerate(PLANS[plan]):
        if b == RAMP_AT:
            dur = (RAMP_FRAMES << 8) + 77
            be.unit_write(sc.rootv[1], PAN, fix(90.0), 33, dur)
            be.unit_write(sc.rootv[1], VOL, fix(100.0), 0, dur)
            be.unit_write(bus["units"][1], PAN, fix(-0.5), 0, dur)
            be.unit_write(bus["units"][1], VOL, fix(-127.9), 200, dur)
        for n in frags:
            sc.walk(n)
        chunks.append(be.render(sum(frags)))
        if info is not None:
            info.append((last_batch(be), be.last_batch_buses()))
    return chunks


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
                if isinstance(w, np.ndarray):
                    w.setflags(write=False)
        return memo[key]
    return get


def same(got, want, info=None):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert w.any(), b
        assert first_diff(g, w) is None, f"batch {b}: (ch, frame, gpu, oracle) = {first_diff(g, w)}; {info[b] if info else ''}"


def leaf_counts(bi):
    return tuple(int(getattr(bi, n)) for n in ("recs_voices", "win_voices", "n_moving_listed", "general_voices"))


def bus_counts(bu):
    return tuple(int(getattr(bu, n)) for n in ("driver_voices", "driver_ramping", "fbd_voices", "generic_voices"))


def _class_env(monkeypatch, **env):
    for k in ("A2AMD_NO_FAST", "A2AMD_FMVPW", "A2AMD_NO_MOVING", "A2AMD_NOISE_QUIET", "A2AMD_NZF_MIN"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("A2AMD_O2F_MIN", "8")        # (the class's quiet kernel from 8 voices on, not from 512)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------------------
# CPU: what the tables and the scripts are built on
# ---------------------------------------------------------------------------
def test_tables_reach_what_they_are_for():
    words = [(w32(a << 8), w32(v << 8), w32(p << 8)) for a, v, p in GAINS]
    assert any(a < 0 for a, v, p in words) and any(v < 0 for a, v, p in words)
    for sign in (1, -1):        # beyond +-1 with a volume of either sign
        assert any(abs(p) > 0xffffff and v * sign > 0 for a, v, p in words)
    # vol << 1 wraps (64 and above in 8.24), and a register value whose << 8 wraps
    assert any(abs(v) >= 64 << 24 and w32(v << 1) != v * 2 for a, v, p in words)
    assert any(w32(x << 8) != x << 8 for g in GAINS for x in g)
    # both sides of the clamp's threshold, as near as a register value gets: 0xffffff lies between two of them
    pans = {p for a, v, p in words}
    assert {0xffff00, 0x1000000, 0x1000100, -0xffff00, -0x1000000, -0x1000100} <= pans
    assert 0xffff00 < 0xffffff < 0x1000000
    qs = [q for q, lp, bp, hp in FILT]
    assert 0 in qs and any(0 < q < 512 for q in qs) and any(q < 0 for q in qs) and fix(30000.0) in qs
    mixes = {m for q, *mix in FILT for m in mix}
    assert {fix(127.0), fix(-127.0)} <= mixes
    # every voice number of a class scene has a combination of its own until 11 * 7 = 77: 131 voices meet all of them
    assert len({(k % len(GAINS), k % len(FILT)) for k in range(N)}) == len(GAINS) * len(FILT)


def test_the_oracle_wraps_where_the_tables_say(oracle_lib):
    """one wtosc; panmix voice per row of GAINS, alone under a neutral root: its two channels are the oscillator's output
    (the same voice at vol 1, pan 0) times panmix_process12's gains, worked out here in Python integers"""
    def render(row, plain):
        be = make_oracle(oracle_lib)
        sc = synth.Scene(be)
        sc.root()
        sc.add_voices(1, "osc-pan", total=1)
        a, vol, pan = GAINS[row]
        be.unit_write(sc.leaves[0][0], A, a)
        if not plain:
            be.unit_write(sc.leaves[0][1], VOL, vol)
            be.unit_write(sc.leaves[0][1], PAN, pan)
        else:
            be.unit_write(sc.leaves[0][1], PAN, 0)
        out = sc.run(2, batch=2)
        be.close()
        return out

    for row, (a, vol, pan) in enumerate(GAINS):
        osc = render(row, True)
        assert np.array_equal(osc[0], osc[1]) and osc.any()
        got = render(row, False)
        v, p = w32(vol << 8), w32(pan << 8)
        vp = w32((p * v) >> 24)
        v0, v1 = w32(v - vp), w32(v + vp)
        if abs(p) > 0xffffff:
            lim = w32(v << 1)
            v0, v1 = min(v0, lim), min(v1, lim)
        want = np.array([[w32((int(x) * g) >> 24) for x in osc[0]] for g in (v0, v1)], dtype=np.int32)
        assert np.array_equal(got, want), row


# ---------------------------------------------------------------------------
# the settled kernels, the bus kernels and the general kernel on the class scenes
# ---------------------------------------------------------------------------
CHAINS = WT + ("fmmix-pan",)


def _settled_asserts(chain, plan, info):
    n_batches = len(PLANS[plan])
    for b in range(n_batches):
        bi, bu = info[b]
        recs, win, moving, general = leaf_counts(bi)
        assert general == 0, (b, bi)
        if b == 0:
            # the births: every wavetable voice on the window or the records kernels' lists (k_leaf_fm* reads its own)
            assert recs + win == (N if chain in WT else 0), (b, bi)
            assert bus_counts(bu) == (0, 0, 0, 4), (b, bu)
            continue
        # no leaf carries a record: the settled kernels'
        assert (recs, win, moving) == (0, 0, 0), (b, bi)
        if chain == "osc2-filter-pan":
            assert (bi.o2f_launched, bi.o2f_voices, bi.o2f_class, bi.o2f_listed) == (1, N, N, 0), (b, bi)
        # the delay chains are k_bus_fbdchain's throughout; the drivers k_bus_driver's, but for the batch of their writes
        if b == RAMP_AT:
            assert bus_counts(bu) == (0, 0, 2, 2), (b, bu)
        else:
            # the host's bound (include/a2amd_bus.h): written at the frame batch RAMP_AT begins at, unsettled until
            # that + ((start + dur) >> 8) + 256 at the latest
            t = batch_starts(PLANS[plan])
            ramping = 2 * (b > RAMP_AT and t[b] < t[RAMP_AT] + RAMP_FRAMES + 256)
            assert bus_counts(bu) == (2, ramping, 2, 0), (b, bu)
    if plan == "64":
        assert [bus_counts(bu)[1] for _bi, bu in info] == [0, 0, 0, 2, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("chain", CHAINS)
def test_settled_and_bus_kernels_match_oracle(oracle_memo, monkeypatch, chain, plan):
    """k_leaf_oscpan / osc2pan / oscfiltpan / osc2filtpan / k_leaf_fm* over 131 loud voices under the root, a driver group
    and two delay groups; k_bus_fbdchain with loud gains on one delay and on three; k_bus_driver with loud volume and pan,
    settled and ramping; fragments of 64 and of 37 frames"""
    _class_env(monkeypatch)
    want = oracle_memo((chain, plan), lambda be: class_script(be, chain, plan))
    gpu = make_gpu(max_batch=8)
    info = []
    got = class_script(gpu, chain, plan, info)
    gpu.close()
    same(got, want, info)
    _settled_asserts(chain, plan, info)


@pytest.mark.gpu
def test_fm_kernel_with_a_voice_per_wavefront(oracle_memo, monkeypatch):
    _class_env(monkeypatch, A2AMD_FMVPW="1")
    want = oracle_memo(("fmmix-pan", "37"), lambda be: class_script(be, "fmmix-pan", "37"))
    gpu = make_gpu(max_batch=8)
    info = []
    got = class_script(gpu, "fmmix-pan", "37", info)
    gpu.close()
    same(got, want, info)
    _settled_asserts("fmmix-pan", "37", info)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", CHAINS)
def test_general_kernel_takes_everything(oracle_memo, monkeypatch, chain):
    """A2AMD_NO_FAST=255: no leaf and no bus owner has a class of its own, k_voices renders the whole tree.
    (a2amd_batch_info.general_voices counts the record-carrying voices OF THE FAST CLASSES that were sent to the general
    kernel - test_records_go_to_the_general_kernel below; with no fast class there is nothing to count, and what proves
    who rendered is that nobody else was given a voice.)"""
    _class_env(monkeypatch, A2AMD_NO_FAST="255")
    want = oracle_memo((chain, "64"), lambda be: class_script(be, chain, "64"))
    gpu = make_gpu(max_batch=8)
    info = []
    got = class_script(gpu, chain, "64", info)
    gpu.close()
    same(got, want, info)
    for b, (bi, bu) in enumerate(info):
        assert leaf_counts(bi) == (0, 0, 0, 0), (b, bi)
        assert (bi.o2f_launched, bi.o2f_class, bi.o2f_listed) == (0, 0, 0), (b, bi)
        assert bus_counts(bu) == (0, 0, 0, 4), (b, bu)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", WT)
def test_records_go_to_the_general_kernel(oracle_memo, monkeypatch, chain):
    """A2AMD_NO_FAST=64: the classes stand, the records kernels are off - in the batch of the births k_voices executes the
    loud writes of all 131 voices (general_voices), the settled kernels take over behind it"""
    _class_env(monkeypatch, A2AMD_NO_FAST="64")
    want = oracle_memo((chain, "37"), lambda be: class_script(be, chain, "37"))
    gpu = make_gpu(max_batch=8)
    info = []
    got = class_script(gpu, chain, "37", info)
    gpu.close()
    same(got, want, info)
    assert [leaf_counts(bi) for bi, _bu in info] == [(0, 0, 0, N), (0, 0, 0, 0)], info


# ---------------------------------------------------------------------------
# the quiet noise kernels
# ---------------------------------------------------------------------------
N_NOISE = 70


def noise_script(be, cls, repeat):
    """test_noise_quiet.QuietScene / test_noise_filt_quiet.FiltScene with the class's 70 voices made loud; the fragments
    behind the first device-seeded (a2amd_fragment_repeat_noise) on the GPU, walked on the oracle.
    Per batch (audio, noise word, batch infos)."""
    be.noise.value = SEED0
    q = QuietScene(be, N_NOISE) if cls == "noise-pan" else FiltScene(be, N_NOISE)
    voices = q.pan if cls == "noise-pan" else q.filt
    assert len(voices) == N_NOISE
    for k, units in enumerate(voices):
        a, vol, pan = GAINS[k % len(GAINS)]
        be.unit_write(units[0], A, a)
        if cls == "noisefilt-pan":
            qq, lp, bp, hp = FILT[k % len(FILT)]
            for reg, val in ((Q, qq), (LP, lp), (BP, bp), (HP, hp)):
                be.unit_write(units[1], reg, val)
        be.unit_write(units[-1], VOL, vol)
        be.unit_write(units[-1], PAN, pan)
    got = []

    def rest(n, frames=64):
        if repeat:
            be.fragment_repeat_noise(frames, n)
        else:
            for _ in range(n):
                q.sc.walk(frames)

    def snap(frames):
        a = be.render(frames)
        got.append((a, be.noise.value, (be.last_batch_noise(), be.last_batch_noise_filter()) if repeat else None))

    q.sc.walk(64)
    rest(3)
    snap(4 * 64)                    # the births
    rest(8)
    snap(8 * 64)
    rest(1)
    snap(64)
    rest(6, 37)
    snap(6 * 37)
    return got


def _noise_compare(got, want):
    assert len(got) == len(want)
    for b, ((a, na, _i), (w, nw, _j)) in enumerate(zip(got, want)):
        assert w.any()
        assert first_diff(a, w) is None, f"batch {b}: (ch, frame, gpu, oracle) = {first_diff(a, w)}"
        assert na == nw, f"batch {b}: noise word {na:#x} against the oracle's {nw:#x}"


@pytest.mark.gpu
@pytest.mark.parametrize("no_fast", [None, "255"])
@pytest.mark.parametrize("cls", ["noise-pan", "noisefilt-pan"])
def test_quiet_noise_kernels_match_oracle(oracle_memo, monkeypatch, cls, no_fast):
    """k_leaf_noisepan / k_leaf_noisefiltpan over 70 loud voices in device-seeded fragments - and the same scene with no
    fast class at all (A2AMD_NO_FAST=255)"""
    _class_env(monkeypatch, A2AMD_NZF_MIN="1", **({"A2AMD_NO_FAST": no_fast} if no_fast else {}))
    want = oracle_memo(("noise", cls), lambda be: noise_script(be, cls, False))
    gpu = make_gpu(max_batch=16)
    got = noise_script(gpu, cls, True)
    gpu.close()
    _noise_compare(got, want)
    for b, (_a, _n, (nz, nf)) in enumerate(got):
        mine, other = (nz, nf) if cls == "noise-pan" else (nf, nz)
        if no_fast or b == 0:
            assert (mine.quiet_launched, mine.quiet_voices) == (0, 0), (b, mine)
            assert (other.quiet_launched, other.quiet_voices) == (0, 0), (b, other)
        else:
            assert (mine.quiet_launched, mine.quiet_voices, mine.class_voices) == (1, N_NOISE, N_NOISE), (b, mine)
            if cls == "noisefilt-pan":      # FiltScene's five noise-pan voices beside them
                assert (nz.quiet_launched, nz.quiet_voices, nz.standin_voices) == (1, NF_PAN, NF_OTHER), (b, nz)


# ---------------------------------------------------------------------------
# the same classes driven by writes: the window kernels and the records kernels
# ---------------------------------------------------------------------------
DURS = [0, 100, 3000, 70000]
_SPECIAL = [fix(64.0), fix(-64.0), fix(127.99), fix(-128.0), fix(130.0), fix(300.0), fix(-300.0), ONE - 1, ONE, ONE + 1,
            -(ONE - 1), -ONE, -(ONE + 1), 0]


def loud_draw(rng):
    """a gain register value: of musical size and either sign, anywhere in 8.24's range, or one of the edges"""
    kind = int(rng.integers(0, 3))
    if kind == 0:
        return fix(float(rng.uniform(-1.5, 1.5)))
    if kind == 1:
        return fix(float(rng.uniform(-127.9, 127.9)))
    return int(_SPECIAL[int(rng.integers(0, len(_SPECIAL)))])


def loud_q(rng):
    return int(rng.choice([0, 300, fix(-5.0), fix(30000.0), fix(0.001), fix(float(rng.uniform(0.2, 9)))]))


def loud_wt_script(be, chain, nvoices=N, batches=3, bfrags=8, seed=23, info=None):
    """test_gpu_parity._wt_script's structure - writes between sub-fragment windows, ramps, births in the middle of a
    fragment, deaths, under the root and under two delay groups - with the gain values drawn by loud_draw / loud_q.
    Pitch, phase and wave draws are _wt_script's."""
    rng = np.random.default_rng(seed)
    sc = synth.Scene(be)
    sc.root()
    homes = [sc.add_group(), sc.add_group(fb=TAPS3[1]), None]
    for g in homes:
        sc.add_voices(nvoices // 3 + (g is None) * (nvoices % 3), chain=chain, group=g, total=nvoices)
    nosc = 2 if chain.startswith("osc2") else 1
    filt = nosc if "filter" in chain else None
    lists = [sc.leaves] + [g["leaves"] for g in sc.groups]
    k = 0
    for l in lists:
        for units in l:
            make_loud(be, units, chain, k)
            k += 1
    chunks = []
    frag = 0
    for _ in range(batches):
        for _ in range(bfrags):
            frag += 1
            nall = sum(len(l) for l in lists)
            busy = set(int(k) for k in rng.choice(nall, nall // 4, replace=False))
            newborn = None
            if frag % 3 == 2:
                g = homes[frag % len(homes)]
                dst = sc.leaves if g is None else g["leaves"]
                sc.add_voices(1, chain=chain, group=g, total=nvoices)
                newborn = (dst[-1], int(rng.integers(1, 63)))
            counter = [0]

            def leaf(units):
                k = counter[0]
                counter[0] += 1
                pan = units[-1]
                if newborn and units is newborn[0]:
                    for u in units:
                        be.unit_process(u, newborn[1], 64 - newborn[1])
                    return
                if k not in busy:
                    for u in units:
                        be.unit_process(u, 0, 64)
                    return
                cut = sorted(set(int(c) for c in rng.integers(1, 64, int(rng.integers(1, 4)))))
                at = 0
                for c in cut + [64]:
                    dur = int(rng.choice(DURS))
                    osc = units[int(rng.integers(0, nosc))]
                    reg = int(rng.integers(0, 4))
                    if reg == 0:
                        val = int(rng.choice([-1] + [sc.wave_ids[i] for i in (0, 3, 7, 11, 23)]))
                    elif reg == 1:
                        val = fix(float(rng.uniform(-3, 3)))
                    elif reg == 2:
                        val = loud_draw(rng)
                    else:
                        val = int(rng.integers(0, 65536))
                    be.unit_write(osc, reg, val, int(rng.integers(0, 256)), dur)
                    if rng.random() < 0.6:
                        be.unit_write(pan, int(rng.integers(0, 2)), loud_draw(rng), 0, dur)
                    if filt is not None and rng.random() < 0.5:
                        freg = int(rng.integers(0, 5))
                        fval = fix(float(rng.uniform(-1, 5))) if freg == 0 else loud_q(rng) if freg == 1 else loud_draw(rng)
                        be.unit_write(units[filt], freg, fval, int(rng.integers(0, 256)), dur)
                    for u in units:
                        be.unit_process(u, at, c - at)
                    at = c

            be.fragment(64)
            be.unit_process(sc.rootv[0], 0, 64)
            for g in sc.groups:
                be.unit_process(g["units"][0], 0, 64)
                for units in g["leaves"]:
                    leaf(units)
                be.inline_end(g["units"][0])
                for d in g["units"][1:]:
                    be.unit_process(d, 0, 64)
            for units in sc.leaves:
                leaf(units)
            be.inline_end(sc.rootv[0])
            be.unit_process(sc.rootv[1], 0, 64)
            be.unit_process(sc.rootv[2], 0, 64)
            if frag % 4 == 3:
                l = lists[int(rng.integers(0, len(lists)))]
                if len(l) > 4:
                    k = int(rng.integers(0, len(l)))
                    for u in l[k]:
                        be.unit_deinit(u)
                    del l[k]
        chunks.append(be.render(bfrags * 64))
        if info is not None:
            info.append(last_batch(be))
    return chunks


def loud_fm_script(be, nvoices=N, batches=3, bfrags=8, seed=29):
    """test_gpu_parity._fm_script's structure with every amplitude, depth and feedback drawn by loud_draw"""
    rng = np.random.default_rng(seed)
    sc = synth.Scene(be)
    sc.root()
    sc.add_voices(nvoices, chain="fmmix-pan")
    for k, units in enumerate(sc.leaves):
        make_loud(be, units, "fmmix-pan", k)
    nops = [synth.FM_KINDS[sorted(synth.FM_KINDS)[k % 8]][1] for k in range(nvoices)]
    chunks = []
    frag = 0
    for _ in range(batches):
        for _ in range(bfrags):
            frag += 1
            busy = set(int(k) for k in rng.choice(len(sc.leaves), len(sc.leaves) // 4, replace=False))
            be.fragment(64)
            be.unit_process(sc.rootv[0], 0, 64)
            newborn = None
            if frag % 5 == 2:
                n0 = len(sc.leaves)
                sc.add_voices(1, chain="fm4r-pan" if frag % 2 else "fm2-pan", total=nvoices)
                newborn = (sc.leaves[n0], int(rng.integers(1, 63)))
                nops.append(4 if frag % 2 else 2)
            for k, units in enumerate(sc.leaves):
                fm, pan = units
                if newborn and units is newborn[0]:
                    be.unit_process(fm, newborn[1], 64 - newborn[1])
                    be.unit_process(pan, newborn[1], 64 - newborn[1])
                    continue
                if k not in busy:
                    be.unit_process(fm, 0, 64)
                    be.unit_process(pan, 0, 64)
                    continue
                cut = sorted(set(int(c) for c in rng.integers(1, 64, int(rng.integers(1, 4)))))
                at = 0
                for c in cut + [64]:
                    dur = int(rng.choice(DURS))
                    reg = int(rng.integers(0, 1 + 3 * nops[k]))
                    val = fix(float(rng.uniform(-1, 3))) if reg % 3 == 1 else loud_draw(rng)
                    if reg == 0:
                        val = int(rng.integers(0, 65536))
                    be.unit_write(fm, reg, val, int(rng.integers(0, 256)), dur)
                    if rng.random() < 0.6:
                        be.unit_write(pan, int(rng.integers(0, 2)), loud_draw(rng), 0, dur)
                    be.unit_process(fm, at, c - at)
                    be.unit_process(pan, at, c - at)
                    at = c
            be.inline_end(sc.rootv[0])
            be.unit_process(sc.rootv[1], 0, 64)
            be.unit_process(sc.rootv[2], 0, 64)
            if frag % 4 == 3 and len(sc.leaves) > 8:
                k = int(rng.integers(0, len(sc.leaves)))
                for u in sc.leaves[k]:
                    be.unit_deinit(u)
                del sc.leaves[k]
                del nops[k]
        chunks.append(be.render(bfrags * 64))
    return chunks


@pytest.mark.gpu
@pytest.mark.parametrize("win", ["1", "0"])
@pytest.mark.parametrize("chain", WT)
def test_window_and_records_kernels_execute_loud_writes(oracle_memo, monkeypatch, chain, win):
    """k_win_ctl / k_win_render / k_win_render_f (A2AMD_WIN=1) and k_leaf_recs (A2AMD_WIN=0)"""
    _class_env(monkeypatch, A2AMD_WIN=win)
    want = oracle_memo(("writes", chain), lambda be: loud_wt_script(be, chain))
    gpu = make_gpu(max_batch=8)
    info = []
    got = loud_wt_script(gpu, chain, info=info)
    gpu.close()
    same(got, want, info)
    for b, bi in enumerate(info):
        if win == "1":
            assert bi.win_voices > N // 4 and bi.recs_voices == 0, (b, bi)
        else:
            assert bi.recs_voices > N // 4 and bi.win_voices == 0, (b, bi)


@pytest.mark.gpu
@pytest.mark.parametrize("vpw", [None, "1"])
def test_fm_kernel_executes_loud_writes(oracle_memo, monkeypatch, vpw):
    _class_env(monkeypatch, **({"A2AMD_FMVPW": vpw} if vpw else {}))
    want = oracle_memo(("writes", "fm"), loud_fm_script)
    gpu = make_gpu(max_batch=8)
    got = loud_fm_script(gpu)
    assert last_batch(gpu).general_voices == 0
    gpu.close()
    same(got, want)


# ---------------------------------------------------------------------------
# the pan clamp across the end of a pan ramp
# ---------------------------------------------------------------------------
# panmix decides "clamped" in front of a2_PrepareRamper, from pan.value or pan.target (panmix.c:117-135): on the way from
# beyond +-1 to 0.25 a window is clamped, first frame to last, as long as it BEGINS beyond +-1, whatever the target; and
# with a negative volume lim = vol << 1 lies BELOW both gains, so the flag alone changes every sample.
H_BFRAGS, H_BATCHES, H_WRITE = 4, 9, 2
H_VOLS, H_FROM, H_TO = (fix(-1.0), fix(-100.0)), (fix(1.5), fix(-1.5)), fix(0.25)
# where the ramp's last window lies: (the fragment, counted from the write; the frames of every fragment of the script).
# The duration that puts it there is that many fragments, 21 frames and 77 / 256 of a frame.  With fragments of 37 frames
# the deltas truncate and the ramp stops short of the target; with fragments of 64 it cannot - every window moves the
# value by a multiple of 64, and the way from +-1.5 to 0.25 is one.  The value is beyond +-1 for the first two fifths of
# the way: in "same-fragment" the one window there is; in the next three during the first fragments of the batch of the
# write (the records' kernels); in "third-batch" into the batch behind it, where the voices carry no record and are
# rendered as gliding ones - by the window kernels' stand-in, by the settled kernels themselves under A2AMD_NO_MOVING=1,
# by k_bus_driver's launch of one workgroup a voice.
H_WHERE = {"same-fragment": (0, 64), "last-of-batch": (3, 37), "first-of-batch": (4, 37), "middle-of-batch": (5, 37),
           "third-batch": (17, 64)}


def h_dur(where):
    k, frames = H_WHERE[where]
    return ((k * frames + 21) << 8) + 77


def handover_voices(be, sc, chains, group):
    """four voices a chain: both volumes, both starting pans"""
    out = []
    for chain in chains:
        for vol in H_VOLS:
            for pan in H_FROM:
                sc.add_voices(1, chain=chain, group=group, total=16)
                units = group["leaves"][-1]
                be.unit_write(units[-1], VOL, vol)
                be.unit_write(units[-1], PAN, pan)
                out.append(units)
    return out


def handover_script(be, where, immediate_at=None, info=None):
    """16 wavetable leaves under a bus group (vol -1, pan 1.5) under the root (vol -100, pan -1.5): in front of batch
    H_WRITE every pan - the leaves' and the two drivers' - starts its way to 0.25.  immediate_at: a fragment, counted
    from the write, in front of which every pan is written once more, at once, to the same target."""
    frames = H_WHERE[where][1]
    sc = synth.Scene(be)
    sc.root()
    bus = sc.add_bus_group()
    voices = handover_voices(be, sc, WT, bus)
    pans = [units[-1] for units in voices] + [bus["units"][1], sc.rootv[1]]
    be.unit_write(bus["units"][1], VOL, H_VOLS[0])
    be.unit_write(bus["units"][1], PAN, H_FROM[0])
    be.unit_write(sc.rootv[1], VOL, H_VOLS[1])
    be.unit_write(sc.rootv[1], PAN, H_FROM[1])
    chunks = []
    for b in range(H_BATCHES):
        if b == H_WRITE:
            for u in pans:
                be.unit_write(u, PAN, H_TO, 0, h_dur(where))
        for f in range(H_BFRAGS):
            if immediate_at is not None and (b - H_WRITE) * H_BFRAGS + f == immediate_at:
                for u in pans:
                    be.unit_write(u, PAN, H_TO)
            sc.walk(frames)
        chunks.append(be.render(H_BFRAGS * frames))
        if info is not None:
            info.append((last_batch(be), be.last_batch_buses()))
    return chunks


def pan_model(where, start):
    """the pan ramper through the fragments from the write on: per fragment (value and flag in front of
    a2_PrepareRamper, value behind the window, the ramp's last window?)"""
    frames = H_WHERE[where][1]
    pan = Ramper(start)
    pan.set(H_TO, 0, h_dur(where))
    out = []
    for _ in range((H_BATCHES - H_WRITE) * H_BFRAGS):
        before = pan.value
        flag = abs(pan.target) > 0xffffff or abs(pan.value) > 0xffffff
        last = pan.prepare(frames) is not None
        pan.run(frames)
        out.append((before, flag, pan.value, last))
    return out


@pytest.mark.parametrize("where", list(H_WHERE))
def test_pan_flag_premise_on_the_oracle(oracle_memo, where):
    """What the hand-over tests stand on, on the restated ramper and the oracle alone.

    The flag is live by the VALUE alone - the target is inside +-1 - in every window that begins beyond +-1: the one
    window of "same-fragment", the first fragments of the others, in "third-batch" beyond the batch of the write.  A
    restatement that looks at pan.target only goes wrong there, and with a negative volume it is heard.

    The ramp's last window stops short of the target - its delta truncates - and the window BEHIND it meets that value,
    not the target, when it decides the flag.  This is NOT a case of its own, whatever the target: the ramper stops less
    than one LSB a frame short, |stop - target| < 64, and the target is a register value shifted left by 8, so stop and
    target lie on the same side of +-0xffffff.  The oracle agrees: writing the target once more, at once, in front of
    that fragment changes no sample from there on.  (In front of the ramp's last window it does.)"""
    k, frames = H_WHERE[where]
    tgt = w32(H_TO << 8)
    for start in H_FROM:
        m = pan_model(where, start)
        assert [j for j, (_b, _f, _a, last) in enumerate(m) if last] == [k]
        before, flag, after, _last = m[k]
        # stopped short: the deltas truncated - with fragments of 37 frames
        assert abs(after - tgt) < frames and (after != tgt) == (frames == 37)
        assert m[k + 1][0] == after and not m[k + 1][1] and m[k + 1][2] == tgt
        live = [j for j, (bf, f, _a, _l) in enumerate(m) if f]
        assert live == [j for j, (bf, _f, _a, _l) in enumerate(m) if abs(bf) > 0xffffff]
        assert live and live[0] == 0 and (max(live) >= H_BFRAGS) == (where == "third-batch")
    # behind its last window a ramp's stale value never raises the flag by itself: every target next to the threshold,
    # from either side
    for t in (ONE - 1, ONE, ONE + 1, -(ONE - 1), -ONE, -(ONE + 1), 0):
        for start in (fix(1.5), fix(-1.5), fix(0.3)):
            pan = Ramper(start)
            pan.set(t, 0, h_dur(where))
            while pan.timer:
                pan.prepare(37)
                pan.run(37)
            # (value or target: a stale value inside adds nothing to a target beyond, one beyond would to a target inside)
            assert abs(pan.value) <= 0xffffff or abs(pan.target) > 0xffffff, (t, start)
    ramp = oracle_memo(("handover", where), lambda be: handover_script(be, where))
    again = oracle_memo(("handover", where, k + 1), lambda be: handover_script(be, where, immediate_at=k + 1))
    early = oracle_memo(("handover", where, k), lambda be: handover_script(be, where, immediate_at=k))
    a, b, c = (np.concatenate(x, axis=1)[:, H_WRITE * H_BFRAGS * frames:] for x in (ramp, again, early))
    assert np.array_equal(a, b)
    assert np.array_equal(a[:, :k * frames], c[:, :k * frames])
    assert not np.array_equal(a[:, k * frames:(k + 1) * frames], c[:, k * frames:(k + 1) * frames])
    assert a[0, k * frames:(k + 1) * frames].any() and a[1, k * frames:(k + 1) * frames].any()


@pytest.mark.gpu
@pytest.mark.parametrize("no_moving", ["", "1"])
@pytest.mark.parametrize("where", list(H_WHERE))
def test_pan_ramp_end_hands_over_to_the_settled_kernels(oracle_memo, monkeypatch, where, no_moving):
    """osc-pan, osc2-pan, osc-filter-pan, osc2-filter-pan and two bus drivers: the batches before the ramp, across its end
    and behind it, each against the oracle's.  A2AMD_NO_MOVING=1: the settled kernels step the gliding voices themselves,
    fragment by fragment, instead of leaving them to the window kernels."""
    _class_env(monkeypatch, A2AMD_O2F_MIN="1", **({"A2AMD_NO_MOVING": "1"} if no_moving else {}))
    want = oracle_memo(("handover", where), lambda be: handover_script(be, where))
    gpu = make_gpu(max_batch=H_BFRAGS)
    info = []
    got = handover_script(gpu, where, info=info)
    gpu.close()
    same(got, want, info)
    # the host's bounds: a leaf written at frame T is listed as gliding while a batch begins before
    # T + 64 + (dur >> 8) + 192 (a2amd_unit_write), a driver before T + (dur >> 8) + 256 (a2amd_bus.h)
    t0, frames = H_WRITE * H_BFRAGS * H_WHERE[where][1], h_dur(where) >> 8
    for b, (bi, bu) in enumerate(info):
        recs, win, moving, general = leaf_counts(bi)
        t = b * H_BFRAGS * H_WHERE[where][1]
        gliding = b > H_WRITE and t < t0 + frames + 256
        assert general == 0, (b, bi)
        if b in (0, H_WRITE):
            assert recs + win == 16 and moving == 0, (b, bi)
            assert bus_counts(bu) == (0, 0, 0, 2), (b, bu)
        else:
            assert recs == 0 and (gliding or win == 0), (b, bi)
            assert moving == (16 if gliding and not no_moving else 0), (b, bi)
            # (any write to a driver's panmix counts for its bound, the ones without a duration at frame 0 too)
            assert bus_counts(bu) == (2, 2 * (gliding or t < 256), 0, 0), (b, bu)
    assert [leaf_counts(bi)[2] for bi, _bu in info][-1] == 0        # the last batch is the settled kernels' again


def noise_handover_script(be, cls, where, repeat):
    """the two quiet noise classes: four voices each way (both volumes, both starting pans) among the scene's others;
    the ramps written in front of a walked fragment, device-seeded fragments behind it"""
    be.noise.value = SEED0
    q = QuietScene(be, 9) if cls == "noise-pan" else FiltScene(be, 9)
    voices = (q.pan if cls == "noise-pan" else q.filt)[:8:2]
    for k, units in enumerate(voices):
        be.unit_write(units[-1], VOL, H_VOLS[k & 1])
        be.unit_write(units[-1], PAN, H_FROM[k >> 1])
    got = []
    fr = H_WHERE[where][1]

    def rest(n):
        if repeat:
            be.fragment_repeat_noise(fr, n)
        else:
            for _ in range(n):
                q.sc.walk(fr)

    def snap():
        got.append((be.render(H_BFRAGS * fr), be.noise.value,
                    (be.last_batch_noise(), be.last_batch_noise_filter()) if repeat else None))

    q.sc.walk(fr)
    rest(H_BFRAGS - 1)
    snap()
    rest(H_BFRAGS)
    snap()
    for units in voices:
        be.unit_write(units[-1], PAN, H_TO, 0, h_dur(where))
    q.sc.walk(fr)
    rest(H_BFRAGS - 1)
    snap()
    for _ in range(H_BATCHES - H_WRITE - 1):
        rest(H_BFRAGS)
        snap()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("where", list(H_WHERE))
@pytest.mark.parametrize("cls", ["noise-pan", "noisefilt-pan"])
def test_pan_ramp_end_hands_over_to_the_quiet_noise_kernels(oracle_memo, monkeypatch, cls, where):
    _class_env(monkeypatch, A2AMD_NZF_MIN="1")
    want = oracle_memo(("noise-handover", cls, where), lambda be: noise_handover_script(be, cls, where, False))
    gpu = make_gpu(max_batch=H_BFRAGS)
    got = noise_handover_script(gpu, cls, where, True)
    gpu.close()
    _noise_compare(got, want)
    t0, frames = H_WRITE * H_BFRAGS * H_WHERE[where][1], h_dur(where) >> 8
    for b, (_a, _n, (nz, nf)) in enumerate(got):
        mine = nz if cls == "noise-pan" else nf
        gliding = b > H_WRITE and b * H_BFRAGS * H_WHERE[where][1] < t0 + frames + 256
        quiet = 0 if b in (0, H_WRITE) else 9 - 4 * gliding
        assert (mine.quiet_launched, mine.quiet_voices) == (int(quiet > 0), quiet), (b, mine)
    assert got[-1][2][0 if cls == "noise-pan" else 1].quiet_voices == 9


# ---------------------------------------------------------------------------
# the general kernel's units on arbitrary samples
# ---------------------------------------------------------------------------
K_DC, K_WAVESHAPER, K_DCBLOCK, K_LIMITER, K_XSINK, K_XSOURCE = 14, 15, 16, 17, 18, 19
P_FRAGS = 4
WS_AMOUNTS = [(fix(3000.0), fix(-200.0)), (fix(32000.0), fix(1.0)), (fix(0.5), fix(-3.0)), (fix(-32000.0), fix(20000.0))]


def probe_input(seed=1):
    """int32 [2, 256]: INT32_MIN, INT32_MAX, +-2^k and +-2^k +- 1 for k = 22 .. 30, a full-scale square, full-width
    random words; channel 1 carries the same in another order and with other random words"""
    rng = np.random.default_rng(seed)
    edges = [-(1 << 31), (1 << 31) - 1]
    for k in range(22, 31):
        for s in (1, -1):
            edges += [s * (1 << k), s * (1 << k) + 1, s * (1 << k) - 1]
    square = [(1 << 31) - 1, -(1 << 31)] * 16
    n = P_FRAGS * 64
    chans = []
    for c in range(2):
        body = (edges if c == 0 else edges[::-1]) + (square if c == 0 else [-x - 1 for x in square])
        rnd = rng.integers(-(1 << 31), 1 << 31, n - len(body), dtype=np.int64)
        chans.append(np.concatenate([np.array(body, dtype=np.int64), rnd]) if c == 0 else
                     np.concatenate([rnd[:40], np.array(body, dtype=np.int64), rnd[40:]]))
    x = np.stack(chans).astype(np.int32)
    assert x.shape == (2, n)
    return x


def ws_divisors(x, amount):
    """waveshaper.c:57-112 (fixed point): the divisor of every sample of x at register value `amount`, as int64"""
    a = w32(amount << 8)
    asqr = np.int64(w32(((a >> 4) * (a >> 4)) >> 24))
    v = x.astype(np.int64)
    vsqr = ((v * v) >> 22).astype(np.int32).astype(np.int64)        # (the reference keeps the low word)
    return ((asqr * vsqr) >> 16) + (1 << 24)


def test_probe_input_never_divides_by_zero():
    """the waveshaper is the one probed unit that divides by something its input decides.  (The limiter divides by its
    peak follower, which never falls below the threshold, and the threshold is clamped to 256 at the least on both
    backends: no input makes that zero.)"""
    x = probe_input()
    assert {-(1 << 31), (1 << 31) - 1} <= set(x[0].tolist()) and {-(1 << 31), (1 << 31) - 1} <= set(x[1].tolist())
    for k in range(22, 31):
        for s in (1, -1):
            for d in (-1, 0, 1):
                assert s * (1 << k) + d in x[0] and s * (1 << k) + d in x[1]
    for pair in WS_AMOUNTS:
        for amount in pair:
            d = ws_divisors(x, amount)
            assert (d != 0).all(), amount
            # (INT64_MIN / -1 is the other way a division traps: the dividend is below 2^62 in magnitude)
    # the wrap this is about is there: a divisor that is not positive
    assert any((ws_divisors(x, a) <= 0).any() for pair in WS_AMOUNTS for a in pair)


def probe_script(be, batch):
    """voices  xsource 0 n; UNIT; xsink m 0; panmix m 2 >  under the root: what the clients hand to the source goes through
    UNIT, the sink taps what comes out, the panmix mixes it.  Returns (audio per render, {(voice, fragment): tap})."""
    x = probe_input()
    sc = synth.Scene(be, nwaves=1)
    sc.root()
    voices = []

    def voice(name, kind, nin, nout, flags=0, writes=(), later=()):
        key = sc._key()
        # (an adding 1 -> 2 unit adds to a second channel that nothing in its voice has written - whatever another voice
        # left in the engine's shared scratch buffers: its source fills two channels so that there is something defined)
        nsrc = 2 if flags and (nin, nout) == (1, 2) else nin
        units = [be.unit_init(key, K_XSOURCE, 0, 0, nsrc, 0), be.unit_init(key, kind, flags, nin, nout, 0),
                 be.unit_init(key, K_XSINK, 0, nout, 0, 0), be.unit_init(key, synth.K_PANMIX, synth.PROCADD, nout, 2, 1)]
        for reg, val in writes:
            be.unit_write(units[1], reg, val)
        be.unit_write(units[3], PAN, fix(0.3) if len(voices) % 2 else fix(-0.6))
        be.unit_clients(units[0], 2)
        be.unit_clients(units[2], 1)
        voices.append((name, units, nsrc, later))

    for n in (1, 2):
        for i, (first, second) in enumerate(WS_AMOUNTS):
            voice(f"waveshaper{n}-{i}", K_WAVESHAPER, n, n, writes=[(0, first)], later=[(0, second, 0)])
        voice(f"dcblock{n}", K_DCBLOCK, n, n, writes=[(0, fix(2.0))])
        voice(f"limiter{n}-a", K_LIMITER, n, n, writes=[(0, 0), (1, 0)], later=[(0, fix(-5.0), 0), (1, fix(-1.0), 0)])
        voice(f"limiter{n}-b", K_LIMITER, n, n, writes=[(0, fix(30000.0)), (1, fix(30000.0))], later=[(1, fix(0.05), 3000)])
        for i, (q, lp, bp, hp) in enumerate(FILT):
            voice(f"filter{n}-{i}", synth.K_FILTER12, n, n, writes=[(0, fix(2.0)), (Q, q), (LP, lp), (BP, bp), (HP, hp)],
                  later=[(Q, FILT[(i + 1) % len(FILT)][0], 3000)])
    # panmix in its four channel shapes, replacing and adding, on both sides of the clamp and of zero
    for nin, nout in ((1, 1), (1, 2), (2, 1), (2, 2)):
        for add in (0, synth.PROCADD):
            for i in (1, 3, 5, 9):
                _a, vol, pan = GAINS[i]
                voice(f"panmix{nin}{nout}{'+' if add else ''}-{i}", synth.K_PANMIX, nin, nout, flags=add,
                      writes=[(VOL, vol), (PAN, pan)], later=[(PAN, GAINS[(i + 1) % len(GAINS)][2], 3000)])
    # fbdelay 1 -> 1 and 2 -> 2 with taps of a few frames (edge.a2s' times) and the loud gains
    for n in (1, 2):
        for taps in ((3.3, 1.7, 2.9), (0, 11, 0.02)):
            voice(f"fbdelay{n}-{taps[0]}", synth.K_FBDELAY, n, n,
                  writes=[(r, fix(ms)) for r, ms in enumerate(taps)] + list(DELAY_GAINS), later=[(FBG, fix(40.0), 0)])
    chunks, taps, pending = [], {}, 0
    for frag in range(P_FRAGS):
        be.fragment(64)
        be.unit_process(sc.rootv[0], 0, 64)
        cuts = [0, 64] if frag % 2 else [0, 13, 64]
        for name, units, nin, later in voices:
            if frag == 2:
                for reg, val, dur in later:
                    be.unit_write(units[1], reg, val, 0, dur)
            for a, b in zip(cuts[:-1], cuts[1:]):
                be.unit_inject(units[0], a, x[:nin, frag * 64 + a:frag * 64 + b])
                for u in units:
                    be.unit_process(u, a, b - a)
        be.inline_end(sc.rootv[0])
        be.unit_process(sc.rootv[1], 0, 64)
        be.unit_process(sc.rootv[2], 0, 64)
        pending += 1
        if pending == batch or frag == P_FRAGS - 1:
            chunks.append(be.render(pending * 64))
            for name, units, nin, later in voices:
                for f in range(pending):
                    taps[name, frag - pending + 1 + f] = be.unit_tapped(units[2], f)
            pending = 0
    return chunks, taps


def test_probe_runs_on_the_oracle(oracle_memo):
    chunks, taps = oracle_memo(("probe",), lambda be: probe_script(be, P_FRAGS))
    one = oracle_memo(("probe", 1), lambda be: probe_script(be, 1))
    assert np.array_equal(np.concatenate(chunks, axis=1), np.concatenate(one[0], axis=1))
    assert sorted(taps) == sorted(one[1]) and all(np.array_equal(taps[k], one[1][k]) for k in taps)
    assert all(t.any() for t in taps.values())
    # the wrapped divisors were met: a waveshaper's output of the other sign than its input's
    x = probe_input()
    t = np.concatenate([taps["waveshaper1-1", f] for f in range(P_FRAGS)], axis=1)[0]
    assert ((t.astype(np.int64) * x[0].astype(np.int64)) < 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [P_FRAGS, 1])
def test_general_kernel_units_on_arbitrary_samples(oracle_memo, batch):
    """k_voices' waveshaper, dcblock, limiter, filter12, panmix (1->1, 1->2, 2->1, 2->2, replacing and adding) and
    fbdelay on full-width samples: every unit's output as the sink taps it and the mix, against the oracle's"""
    want, wtaps = oracle_memo(("probe",) if batch == P_FRAGS else ("probe", 1), lambda be: probe_script(be, batch))
    gpu = make_gpu(max_batch=batch)
    got, gtaps = probe_script(gpu, batch)
    gpu.close()
    assert sorted(gtaps) == sorted(wtaps)
    for k in sorted(wtaps):
        assert np.array_equal(gtaps[k], wtaps[k]), f"{k}: the unit's output differs, first (ch, frame, gpu, oracle) = " \
            f"{first_diff(gtaps[k], wtaps[k])}"
    same(got, want)
