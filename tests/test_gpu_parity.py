"""Parity of the HIP path (through the C ABI of liba2amd.so) with the CPU
oracle and with the fixtures captured from the compiled reference.
Bit-exact: everything on this path is integer arithmetic."""
import ctypes
import os

import numpy as np
import pytest

from audiality2_amd import synth
from audiality2_amd.replay import Trace, replay
from conftest import GOLDEN, ROOT, fnv1a_fragments, make_gpu, make_oracle, KNOWN_DEVIATIONS, differing_fragments

pytestmark = pytest.mark.gpu

CASES = ["sustain", "filter", "delaybus", "scripted", "edge", "fm", "fmtest3", "fmtest4", "fx", "loud", "dctest", "wstest", "envwire", "unload", "k2intro", "k2intro44", "k2epilogue", "k2loader", "k2trance", "pulsetronic",
         # the reference's own test/data scripts (make_goldens.py: td_*)
         "td_envtest", "td_envtest2", "td_envtest3", "td_envtest4", "td_pitchenvtest", "td_ramptest", "td_ramptest2",
         "td_ramptestenv", "td_evtest", "td_recursetest", "td_microtonal", "td_noisephase", "td_evilnoises"]


class BatchInfo(ctypes.Structure):
    """a2amd_batch_info (include/a2amd.h): which kernels the last batch's wavetable leaf voices went to"""
    _fields_ = [(n, ctypes.c_uint32) for n in (
        "o2f_launched", "o2f_voices", "o2f_vpg", "o2f_max_vpg", "o2f_class", "o2f_listed", "recs_voices", "win_voices",
        "win_slabs", "n_moving_listed", "general_voices")]

    def __repr__(self):
        return "BatchInfo(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_) + ")"


def last_batch(gpu):
    bi = BatchInfo()
    gpu.lib.a2amd_last_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(BatchInfo)]
    gpu.lib.a2amd_last_batch.restype = ctypes.c_int
    assert gpu.lib.a2amd_last_batch(gpu.ctx, ctypes.byref(bi)) == 0
    return bi


def is_gpu(be):
    return hasattr(be.lib, "a2amd_last_batch")


def auto_o2f_vpg(n, maxv):
    """voices per workgroup the launcher deals n voices of 2 x wtosc-filter12-panmix by (issue_kernels, a2amd_sched.cpp):
    the fewest whole rounds of 256 workgroups with at most maxv voices each"""
    rounds = max(1, (n + 256 * maxv - 1) // (256 * maxv))
    return min(max((n + 256 * rounds - 1) // (256 * rounds), 1), maxv)


def first_diff(a, b):
    d = np.nonzero(a != b)
    if not len(d[0]):
        return None
    i = int(np.argmin(d[1]))
    return int(d[0][i]), int(d[1][i]), int(a[d[0][i], d[1][i]]), int(b[d[0][i], d[1][i]])


@pytest.mark.parametrize("batch", [1, 7, 64, "64-records-kernels"])
@pytest.mark.parametrize("name", CASES)
def test_reference_traces_on_gpu(oracle_lib, monkeypatch, name, batch):
    """The reference's own call traces (its five benchmark songs and our test scripts),
    rendered on the GPU in batches of 1, 7 and 64 fragments, hash-equal to the audio the reference produced - with the
    window kernels (a2amd_win.hip; forced for the suite, conftest.py) and, at 64, with the records kernels (k_leaf_recs:
    what a scene of fewer than a few thousand voices gets by default)."""
    if batch == "64-records-kernels":
        monkeypatch.setenv("A2AMD_WIN", "0")
        batch = 64
    if name in ("k2intro", "k2intro44", "k2epilogue", "k2loader", "k2trance", "pulsetronic") and batch == 1:
        pytest.skip("covered by the batched run; one launch set per fragment is slow over 4500 fragments")
    tr = Trace(os.path.join(GOLDEN, f"{name}.trace.xz"))
    cfg = tr.config
    gpu = make_gpu(cfg["samplerate"], cfg["basepitch"], cfg["channels"], max_batch=batch)
    out = replay(tr, gpu, batch=batch, check_noise=True)
    gpu.close()
    want = np.load(os.path.join(GOLDEN, f"{name}.hash.npy"))
    got = fnv1a_fragments(out)
    bad = differing_fragments(name, got, want)
    if len(bad) or name in KNOWN_DEVIATIONS:
        # documented deviations from the reference (conftest.KNOWN_DEVIATIONS)
        # must still be what the oracle renders
        ora = make_oracle(oracle_lib, cfg["samplerate"], cfg["basepitch"], cfg["channels"])
        ref = replay(tr, ora, batch=64)
        ora.close()
        assert len(bad) == 0 and first_diff(out, ref) is None, (
            f"{name}: {len(bad)} fragments differ from the reference, first {bad[:4]}; "
            f"first sample diff (ch, frame, gpu, oracle) = {first_diff(out, ref)}")


@pytest.mark.parametrize("chain,n", [("osc-pan", 1024), ("osc-filter-pan", 512), ("osc2-pan", 300),
                                     ("fmmix-pan", 333), ("fm4-pan", 70), ("fm1-pan", 5000)])
def test_scenes_match_oracle(oracle_lib, chain, n):
    """BASELINE config shapes at oracle-friendly sizes, 24 fragments."""
    outs = []
    for be in (make_gpu(max_batch=8), make_oracle(oracle_lib)):
        sc = synth.Scene(be)
        sc.root()
        sc.add_voices(n, chain=chain)
        outs.append(sc.run(24, batch=8))
        be.close()
    assert first_diff(outs[0], outs[1]) is None


@pytest.mark.parametrize("vpw", [1, 7, 64])
def test_fm_leaf_kernel_wavefront_shapes(oracle_lib, monkeypatch, vpw):
    """The fm->panmix leaf kernel gives each wavefront `vpw` voices of one unit
    kind (the host pads the kind groups); any shape renders the same audio."""
    monkeypatch.setenv("A2AMD_FMVPW", str(vpw))
    outs = []
    for be in (make_gpu(max_batch=8), make_oracle(oracle_lib)):
        sc = synth.Scene(be)
        sc.root()
        sc.add_voices(203, chain="fmmix-pan")
        g = sc.add_group()
        sc.add_voices(41, chain="fm3p-pan", group=g)
        outs.append(sc.run(19, batch=8, frames=64))
        be.close()
    assert first_diff(outs[0], outs[1]) is None


def test_groups_with_delays_match_oracle(oracle_lib):
    """Config 4 shape: 2-oscillator leaves under inline->fbdelay->fbdelay groups,
    long and short (< one fragment) delay taps."""
    outs = []
    for be in (make_gpu(max_batch=16), make_oracle(oracle_lib)):
        sc = synth.Scene(be)
        sc.root()
        g1 = sc.add_group()
        g2 = sc.add_group(fb=(1.2, 0.5, 137.9), gains=(0.2, 0.3, 0.3))
        sc.add_voices(40, chain="osc2-pan", group=g1, total=128)
        sc.add_voices(40, chain="osc2-pan", group=g2, total=128)
        sc.add_voices(48, chain="osc-filter-pan", total=128)
        outs.append(sc.run(150, batch=16))
        be.close()
    assert first_diff(outs[0], outs[1]) is None


def test_partial_fragments_and_voice_death(oracle_lib):
    outs = []
    for be in (make_gpu(max_batch=4), make_oracle(oracle_lib)):
        sc = synth.Scene(be)
        sc.root()
        sc.add_voices(70)
        a = sc.run(5, batch=4, frames=37)
        for units in sc.leaves[:30]:
            for u in units:
                be.unit_deinit(u)
        sc.leaves = sc.leaves[30:]
        b = sc.run(6, batch=4, frames=64)
        sc.add_voices(10, chain="osc-filter-pan")
        c = sc.run(3, batch=4, frames=1)
        outs.append(np.concatenate([a, b, c], axis=1))
        be.close()
    assert first_diff(outs[0], outs[1]) is None


def test_fragment_repeat_equals_explicit_walk(oracle_lib):
    """a2amd_fragment_repeat (all VMs asleep) == issuing every Process call."""
    gpu = make_gpu(max_batch=32)
    sc = synth.Scene(gpu)
    sc.root()
    sc.add_voices(256)
    first = sc.run(1, batch=1)
    rc = gpu.lib.a2amd_fragment_repeat(gpu.ctx, 64, 31)
    assert rc == 0, gpu._err(gpu.ctx)
    rest = gpu.render(31 * 64)
    gpu.close()
    ora = make_oracle(oracle_lib)
    so = synth.Scene(ora)
    so.root()
    so.add_voices(256)
    want = so.run(32, batch=32)
    ora.close()
    assert first_diff(np.concatenate([first, rest], axis=1), want) is None


def test_mixed_quiet_and_active_voices_across_batches(oracle_lib):
    """Voices move between the fast kernels (quiet, settled), their per-fragment
    path (ramps in flight) and the general kernel (records this batch) from one
    64-fragment batch to the next; time-sliced launches must not disturb the
    state of voices they skip."""
    outs = []
    for be in (make_gpu(max_batch=64), make_oracle(oracle_lib)):
        sc = synth.Scene(be)
        sc.root()
        sc.add_voices(150, chain="osc-pan", total=256)
        sc.add_voices(106, chain="osc-filter-pan", total=256)
        rng = np.random.default_rng(11)
        chunks = []
        for batch in range(4):
            for f in range(64):
                if f in (0, 5, 33) and batch > 0:
                    for k in rng.choice(256, 40, replace=False):
                        units = sc.leaves[k]
                        dur = int(rng.choice([0, 3000, 40000, 900000]))
                        be.unit_write(units[0], 1, synth.fix(float(rng.uniform(-2, 2))), 17, dur)   # p
                        be.unit_write(units[0], 2, synth.fix(float(rng.uniform(0, .05))), 0, dur)   # a
                        be.unit_write(units[-1], 1, synth.fix(float(rng.uniform(-1.5, 1.5))), 200, dur)  # pan
                        if len(units) == 3:
                            be.unit_write(units[1], 1, synth.fix(float(rng.uniform(1, 9))), 0, dur)  # q
                            be.unit_write(units[1], 0, synth.fix(float(rng.uniform(0, 4))), 0, dur)  # cutoff
                sc.walk(64)
            chunks.append(be.render(64 * 64))
        outs.append(np.concatenate(chunks, axis=1))
        be.close()
    assert first_diff(outs[0], outs[1]) is None


def _fm_script(be, nvoices=190, batches=3, bfrags=16, seed=5):
    """FM voices the way a script drives them: control writes between
    sub-fragment windows, ramps of all lengths, phase resets, voices born in the
    middle of a fragment and voices dying, every few fragments per voice."""
    rng = np.random.default_rng(seed)
    sc = synth.Scene(be)
    sc.root()
    sc.add_voices(nvoices, chain="fmmix-pan")
    nops = [synth.FM_KINDS[sorted(synth.FM_KINDS)[k % 8]][1] for k in range(nvoices)]
    born = [0] * nvoices
    chunks = []
    frag = 0
    for _ in range(batches):
        for _ in range(bfrags):
            frag += 1
            busy = set(int(k) for k in rng.choice(len(sc.leaves), len(sc.leaves) // 5, replace=False))
            be.fragment(64)
            be.unit_process(sc.rootv[0], 0, 64)
            # a voice is born in the middle of this fragment now and then
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
                    dur = int(rng.choice([0, 100, 3000, 70000, 2000000]))
                    reg = int(rng.integers(0, 1 + 3 * nops[k]))
                    val = synth.fix(float(rng.uniform(-1, 3))) if reg % 3 == 1 else synth.fix(float(rng.uniform(0, 1.5)))
                    if reg == 0:
                        val = int(rng.integers(0, 65536))
                    be.unit_write(fm, reg, val, int(rng.integers(0, 256)), dur)
                    if rng.random() < 0.4:
                        be.unit_write(pan, int(rng.integers(0, 2)), synth.fix(float(rng.uniform(-1.5, 1.5))), 0, dur)
                    be.unit_process(fm, at, c - at)
                    be.unit_process(pan, at, c - at)
                    at = c
            be.inline_end(sc.rootv[0])
            be.unit_process(sc.rootv[1], 0, 64)
            be.unit_process(sc.rootv[2], 0, 64)
            # ... and one dies
            if frag % 4 == 3 and len(sc.leaves) > 8:
                k = int(rng.integers(0, len(sc.leaves)))
                for u in sc.leaves[k]:
                    be.unit_deinit(u)
                del sc.leaves[k]
                del nops[k]
        chunks.append(be.render(bfrags * 64))
    return np.concatenate(chunks, axis=1)


@pytest.mark.parametrize("vpw", [1, 64])
def test_fm_leaf_kernel_executes_records(oracle_lib, monkeypatch, vpw):
    monkeypatch.setenv("A2AMD_FMVPW", str(vpw))
    gpu = make_gpu(max_batch=16)
    got = _fm_script(gpu)
    gpu.close()
    ora = make_oracle(oracle_lib)
    want = _fm_script(ora)
    ora.close()
    assert want.any()
    assert first_diff(got, want) is None


def _wt_script(be, chain, nvoices=300, batches=3, bfrags=16, seed=11, groups=0, walk=False, noise=False, on_batch=None):
    """Wavetable voices the way a script drives them (BASELINE variants 2b / 3b):
    control writes between sub-fragment windows - pitch, amplitude, pan, volume
    ramps of all lengths, phase resets, switches between mip-mapped waves and off
    - voices born in the middle of a fragment and voices dying, under the root
    and under delay groups.  walk=True: through the host walk's short cuts
    (a2amd_voice_process per window, a byte in the default map for a default
    window once the library allows it) where the backend has them.  noise=True:
    oscillators also switch to the noise generator and back - how many draws of
    the engine's one RNG a window takes depends on the phase the oscillator had
    reached as a wavetable oscillator (the host's phase shadow)."""
    rng = np.random.default_rng(seed)
    quick = {}

    def window(units, off, n):
        if walk:
            quick[units[0]] = be.voice_process(units, off, n)
        else:
            for u in units:
                be.unit_process(u, off, n)

    def default(units):
        if walk and quick.get(units[0]) == 1:
            be.mark_default(units)
        else:
            window(units, 0, 64)

    sc = synth.Scene(be)
    sc.root()
    homes = [sc.add_group() for _ in range(groups)] or [None]
    for g in homes:
        sc.add_voices(nvoices // len(homes), chain=chain, group=g, total=nvoices)
    nosc = 2 if chain.startswith("osc2") else 1
    filt = nosc if "filter" in chain else None      # chain position of the filter12
    lists = [sc.leaves] + [g["leaves"] for g in sc.groups]
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
                    window(units, newborn[1], 64 - newborn[1])
                    return
                if k not in busy:
                    default(units)
                    return
                cut = sorted(set(int(c) for c in rng.integers(1, 64, int(rng.integers(1, 4)))))
                at = 0
                for c in cut + [64]:
                    dur = int(rng.choice([0, 100, 3000, 70000, 2000000]))
                    osc = units[int(rng.integers(0, nosc))]
                    reg = int(rng.integers(0, 4))
                    if reg == 0:        # off, or another mip-mapped wave
                        val = int(rng.choice([-1] + [sc.wave_ids[i] for i in (0, 3, 7, 11, 23)] +
                                             ([sc.noise_id] * 3 if noise else [])))
                    elif reg == 1:
                        val = synth.fix(float(rng.uniform(-3, 3)))
                    elif reg == 2:
                        val = synth.fix(float(rng.uniform(0, 1.5)))
                    else:
                        val = int(rng.integers(0, 65536))
                    be.unit_write(osc, reg, val, int(rng.integers(0, 256)), dur)
                    if rng.random() < 0.4:
                        be.unit_write(pan, int(rng.integers(0, 2)), synth.fix(float(rng.uniform(-1.5, 1.5))), 0, dur)
                    if filt is not None and rng.random() < 0.5:
                        freg = int(rng.integers(0, 5))      # cutoff (set or ramp), q, lp, bp, hp
                        fval = synth.fix(float(rng.uniform(-1, 5))) if freg == 0 else \
                            synth.fix(float(rng.uniform(0.2, 9))) if freg == 1 else synth.fix(float(rng.uniform(0, 1)))
                        be.unit_write(units[filt], freg, fval, int(rng.integers(0, 256)), dur)
                    window(units, at, c - at)
                    at = c

            be.fragment(64)
            be.unit_process(sc.rootv[0], 0, 64)
            for g in sc.groups:
                be.unit_process(g["units"][0], 0, 64)
                for units in g["leaves"]:
                    leaf(units)
                be.inline_end(g["units"][0])
                be.unit_process(g["units"][1], 0, 64)
                be.unit_process(g["units"][2], 0, 64)
            for units in sc.leaves:
                leaf(units)
            be.inline_end(sc.rootv[0])
            be.unit_process(sc.rootv[1], 0, 64)
            be.unit_process(sc.rootv[2], 0, 64)
            if frag % 4 == 3:       # ... and one dies
                l = lists[int(rng.integers(0, len(lists)))]
                if len(l) > 4:
                    k = int(rng.integers(0, len(l)))
                    for u in l[k]:
                        be.unit_deinit(u)
                    quick.pop(l[k][0], None)
                    del l[k]
        chunks.append(be.render(bfrags * 64))
        if on_batch:
            on_batch()
    return np.concatenate(chunks, axis=1)


@pytest.mark.parametrize("chain,groups", [("osc-pan", 0), ("osc2-pan", 3), ("osc-filter-pan", 0), ("osc2-filter-pan", 2)])
@pytest.mark.parametrize("bfrags", [1, 16])
def test_host_walk_short_cuts_match_oracle(oracle_lib, chain, groups, bfrags):
    """a2amd_voice_process + a2amd_default_map (what the drop-in's Process callbacks
    use): whole-voice windows, default windows reported by one byte store also
    while the voice's pitch is still ramping (the phase shadow replays those
    fragments when it is next needed), against the oracle driven unit by unit."""
    gpu = make_gpu(max_batch=16)
    got = _wt_script(gpu, chain, groups=groups, bfrags=bfrags, batches=48 // bfrags, walk=True, noise=True)
    gpu.close()
    ora = make_oracle(oracle_lib)
    want = _wt_script(ora, chain, groups=groups, bfrags=bfrags, batches=48 // bfrags, walk=True, noise=True)
    ora.close()
    assert want.any()
    assert first_diff(got, want) is None


@pytest.mark.parametrize("chain,groups", [("osc-pan", 0), ("osc2-pan", 0), ("osc2-pan", 3), ("osc-filter-pan", 0),
                                          ("osc-filter-pan", 2), ("osc2-filter-pan", 0), ("osc2-filter-pan", 3)])
@pytest.mark.parametrize("rvpw", [1, 5, 64])
def test_wavetable_leaf_kernel_executes_records(oracle_lib, monkeypatch, chain, groups, rvpw):
    """k_leaf_recs: wtosc[+wtosc][->filter12]->panmix voices that carry records in a
    batch (writes between windows, windows inside a fragment, births, deaths; with a
    filter also cutoff sets and ramps, q ramps, lp/bp/hp) are rendered by the
    records-executing leaf kernel, not the general one; the 2 x wtosc->filter12->panmix
    voice (the usual subtractive note) always is; with one, a few and 64 voices per
    wavefront."""
    monkeypatch.setenv("A2AMD_WIN", "0")        # (the kernels this test is about: k_leaf_recs)
    monkeypatch.setenv("A2AMD_RVPW", str(rvpw))
    gpu = make_gpu(max_batch=16)
    got = _wt_script(gpu, chain, groups=groups)
    gpu.close()
    ora = make_oracle(oracle_lib)
    want = _wt_script(ora, chain, groups=groups)
    ora.close()
    assert want.any()
    assert first_diff(got, want) is None


@pytest.mark.parametrize("chain,groups", [("osc-filter-pan", 0), ("osc-filter-pan", 2), ("osc2-filter-pan", 3)])
@pytest.mark.parametrize("rvpw", [1, 3, 4, 16])
def test_records_kernel_filter_with_lane_per_voice(oracle_lib, monkeypatch, chain, groups, rvpw):
    """The lane = voice filter (round 4): from 16 384 voices up the records kernels run filter12's recurrence with lane =
    voice - the walk lists each window's filter and pan parameters, the recurrence runs over rows in LDS,
    the pan stage reads them back.  Forced on here (A2AMD_VFILT=1) at sizes the oracle follows: the same
    random script of writes, ramps, cutoff sets and sweeps, q ramps, mix changes, births and deaths, with 1,
    3, 4 and 16 voices per wavefront (a pool that fills up in mid-voice turns the wavefront round early)."""
    monkeypatch.setenv("A2AMD_WIN", "0")        # (the kernels this test is about: k_leaf_recs)
    monkeypatch.setenv("A2AMD_VFILT", "1")
    monkeypatch.setenv("A2AMD_RVPW", str(rvpw))
    gpu = make_gpu(max_batch=16)
    got = _wt_script(gpu, chain, groups=groups)
    gpu.close()
    ora = make_oracle(oracle_lib)
    want = _wt_script(ora, chain, groups=groups)
    ora.close()
    assert want.any()
    assert first_diff(got, want) is None


def test_records_kernel_filter_lane_per_voice_matches_scalar_filter_at_size(monkeypatch):
    """... and A/B against the scalar recurrence on the same script at 6 000 voices, 64-fragment batches."""
    monkeypatch.setenv("A2AMD_WIN", "0")        # (the kernels this test is about: k_leaf_recs)
    outs = []
    for vf in ("0", "1"):
        monkeypatch.setenv("A2AMD_VFILT", vf)
        gpu = make_gpu(max_batch=64)
        outs.append(_wt_script(gpu, "osc-filter-pan", nvoices=6000, batches=2, bfrags=64, groups=8))
        gpu.close()
    assert outs[0].any() and first_diff(outs[0], outs[1]) is None


@pytest.mark.parametrize("raw", ["0", "1"])
def test_private_sample_waves_as_coefficients_and_as_samples(oracle_lib, monkeypatch, raw):
    """SURVEY 8(d)'s private-wave case at oracle size: 24 uploaded sample waves of 20 000 samples (not a power
    of two: the phase wraps by a real modulo), 700 wtosc -> panmix voices over them at mixed pitches / mip
    levels.  The settled kernel reads a wave either as Hermite coefficient entries (A2AMD_RAW=0) or as its
    int16 samples (A2AMD_RAW=1: what the footprint policy picks for banks no cache holds) - both bit-equal
    to the oracle, over 3 x 16 fragments with a short fragment in between."""
    monkeypatch.setenv("A2AMD_RAW", raw)
    outs = []
    for be in (make_gpu(max_batch=16), make_oracle(oracle_lib)):
        sc = synth.Scene(be)
        sc.root()
        sc.private_waves(24, length=20000, period=256)
        sc.add_voices(700, chain="osc-pan", private=True)
        a = sc.run(16, batch=16)
        b = sc.run(1, batch=1, frames=23)
        c = sc.run(32, batch=16)
        outs.append(np.concatenate([a, b, c], axis=1))
        be.close()
    assert outs[1].any()
    assert first_diff(outs[0], outs[1]) is None


def test_wavetable_records_kernel_matches_general_kernel(monkeypatch):
    """... and A/B against the general kernel on the same script at a size the
    oracle would take long over (A2AMD_NO_FAST=64 sends the records to k_voices)."""
    monkeypatch.setenv("A2AMD_WIN", "0")        # (the kernels this test is about: k_leaf_recs)
    outs = []
    for no in ("0", "64"):
        monkeypatch.setenv("A2AMD_NO_FAST", no)
        gpu = make_gpu(max_batch=64)
        outs.append(_wt_script(gpu, "osc2-pan", nvoices=6000, batches=2, bfrags=64, groups=8))
        gpu.close()
    assert outs[0].any() and first_diff(outs[0], outs[1]) is None


@pytest.mark.parametrize("chain,groups", [("osc-pan", 0), ("osc2-pan", 8), ("osc-filter-pan", 4), ("osc2-filter-pan", 0)])
def test_window_and_records_kernels_agree_at_size(monkeypatch, chain, groups):
    """Round 5: the window kernels (a2amd_win.hip: control pass lane = voice, render pass lane = frame) against the
    records kernels (k_leaf_recs) on the same random script - writes, ramps, sub-fragment windows, births, deaths - at
    the size where the library switches from the one to the other by itself, in one slab and cut into slabs (the
    record cursor carried between them), with one stream and with a stream per list."""
    outs, infos = {}, {}
    for tag, env in (("records", {"A2AMD_WIN": "0"}), ("windows", {"A2AMD_WIN": "1"}),
                     ("slabs", {"A2AMD_WIN": "1", "A2AMD_WIN_SLABS": "3"}), ("auto", {})):
        for k in ("A2AMD_WIN", "A2AMD_WIN_SLABS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        gpu = make_gpu(max_batch=64)
        infos[tag] = []
        outs[tag] = _wt_script(gpu, chain, nvoices=5000, batches=2, bfrags=64, groups=groups,
                               on_batch=lambda: infos[tag].append(last_batch(gpu)))
        gpu.close()
        print(chain, tag, infos[tag])
    # the path each leg took (a switch read once per process would make the legs one and the same)
    for bi in infos["records"]:
        assert bi.recs_voices > 0 and bi.win_voices == 0 and bi.win_slabs == 0, bi
    for bi in infos["windows"]:
        assert bi.win_voices > 0 and bi.recs_voices == 0 and bi.win_slabs == 1, bi
    for bi in infos["slabs"]:
        assert bi.win_voices > 0 and bi.recs_voices == 0 and bi.win_slabs == 3, bi      # (64 fragments in slabs of 22)
    for a, b in zip(infos["records"], infos["windows"]):
        assert a.recs_voices == b.win_voices, (a, b)
    for bi in infos["auto"]:
        assert (bi.win_voices > 0) != (bi.recs_voices > 0), bi
    assert outs["records"].any()
    for tag in ("windows", "slabs", "auto"):
        assert first_diff(outs[tag], outs["records"]) is None, tag


@pytest.mark.parametrize("chain,groups", [("osc-pan", 0), ("osc2-pan", 3), ("osc-filter-pan", 2), ("osc2-filter-pan", 0),
                                          ("osc2-filter-pan", 3)])
def test_window_kernels_cut_into_slabs_match_oracle(oracle_lib, monkeypatch, chain, groups):
    """The window kernels with the batch cut into slabs (A2AMD_WIN_SLABS=3: 32 fragments in slabs of 11, 11 and 10; the
    control pass of slab k + 1 beside the render pass of slab k, the record cursor of every voice carried from slab to
    slab) against the ORACLE, at a size it follows: the random script of writes, ramps, sub-fragment windows, births and
    deaths of the records-kernel tests."""
    monkeypatch.setenv("A2AMD_WIN", "1")
    monkeypatch.setenv("A2AMD_WIN_SLABS", "3")
    gpu = make_gpu(max_batch=32)
    infos = []
    got = _wt_script(gpu, chain, groups=groups, batches=2, bfrags=32, on_batch=lambda: infos.append(last_batch(gpu)))
    gpu.close()
    print(chain, groups, infos)
    for bi in infos:
        assert bi.win_slabs == 3 and bi.win_voices > 0 and bi.recs_voices == 0, bi
        if chain == "osc2-filter-pan":       # (a small scene: every voice of the class is the window kernels')
            assert not bi.o2f_launched and 0 < bi.o2f_listed and bi.o2f_listed + bi.general_voices <= bi.o2f_class, bi
    ora = make_oracle(oracle_lib)
    want = _wt_script(ora, chain, groups=groups, batches=2, bfrags=32)
    ora.close()
    assert want.any()
    assert first_diff(got, want) is None


def test_wave_drop_and_pool_reuse(oracle_lib):
    """Waves come and go (a2_UploadWave / a2_Release while oscillators play
    them): a dropped wave silences its oscillators, its region of the device
    pool is handed to the next upload, re-uploading a key replaces the data."""
    from audiality2_amd.replay import MIPLEVELS
    rng = np.random.default_rng(9)

    def run(be):
        sc = synth.Scene(be, nwaves=2)
        sc.root()
        chunks = []

        def up(key, n):
            w = (rng.integers(-20000, 20000, n)).astype(np.int16)
            sizes, data = synth.wave_pyramid(w)
            return be.wave_upload(key, synth.WMIPWAVE, synth.LOOPED, n, sizes + [0] * (MIPLEVELS - len(sizes)), data)

        def voices(wid, n):
            first = len(sc.leaves)
            sc.add_voices(n, chain="osc-pan", total=64)
            for units in sc.leaves[first:]:
                be.unit_write(units[0], 0, wid)
            return first

        a = up(0x900, 1500)
        voices(a, 6)
        chunks.append(sc.run(3, batch=2))
        be.wave_drop(0x900)                      # oscillators on it fall silent
        chunks.append(sc.run(2, batch=2))
        b = up(0x901, 1500)                      # fits the region wave a left
        voices(b, 5)
        chunks.append(sc.run(3, batch=4))
        c = up(0x901, 700)                       # same key again: replaced
        voices(c, 4)
        chunks.append(sc.run(3, batch=1))
        return np.concatenate(chunks, axis=1)

    rng = np.random.default_rng(9)
    gpu = make_gpu(max_batch=4)
    got = run(gpu)
    gpu.close()
    rng = np.random.default_rng(9)
    ora = make_oracle(oracle_lib)
    want = run(ora)
    ora.close()
    assert want.any() and first_diff(got, want) is None


def test_voice_table_grows_between_batches(oracle_lib):
    """Voices keep arriving after the first render until the device tables have
    to be reallocated (first capacity: 1024 voices / units): the entries of the
    voices that did not change must survive the move (regression: an engine
    spawning 1 024 voices over several fragments faulted on the GPU)."""
    outs = []
    for be in (make_gpu(max_batch=4), make_oracle(oracle_lib)):
        sc = synth.Scene(be)
        sc.root()
        chunks = []
        for step in range(6):
            sc.add_voices(300, chain="osc-pan" if step % 2 else "osc-filter-pan", total=2048)
            chunks.append(sc.run(2, batch=2))
        outs.append(np.concatenate(chunks, axis=1))
        be.close()
    assert first_diff(outs[0], outs[1]) is None


def _scene_fuzz(be, seed, nvoices, batches, bfrags, more_chains=(), on_batch=None):
    """Thousands of voices of mixed classes; in every batch random voices get
    control writes with random timing, some die, new ones arrive: every leaf
    kernel sees quiet, ramping and record-carrying voices side by side."""
    rng = np.random.default_rng(seed)
    sc = synth.Scene(be)
    sc.root()
    chains = ["osc-pan", "osc-filter-pan", "osc2-pan", "fmmix-pan", "fm2-pan"] + list(more_chains)
    g = sc.add_group()
    for i, ch in enumerate(chains):
        sc.add_voices(nvoices // len(chains), chain=ch, total=nvoices, group=g if i == 2 else None)
    chunks = []
    for b in range(batches):
        for f in range(bfrags):
            if rng.random() < 0.4:
                pool = sc.leaves + g["leaves"]
                for k in rng.choice(len(pool), min(len(pool), int(rng.integers(1, 60))), replace=False):
                    units = pool[int(k)]
                    dur = int(rng.choice([0, 200, 5000, 60000, 1500000]))
                    start = int(rng.integers(0, 256))
                    be.unit_write(units[-1], int(rng.integers(0, 2)), synth.fix(float(rng.uniform(-1.4, 1.4))), start, dur)
                    be.unit_write(units[0], 2, synth.fix(float(rng.uniform(0, .02))), start, dur)
                    if rng.random() < 0.5:
                        be.unit_write(units[0], 1, synth.fix(float(rng.uniform(-2, 2))), start, dur)
            sc.walk(64)
        chunks.append(be.render(bfrags * 64))
        if on_batch:
            on_batch()
        # between batches: some voices die, some are born
        for _ in range(int(rng.integers(0, 12))):
            if len(sc.leaves) > 10:
                k = int(rng.integers(0, len(sc.leaves)))
                for u in sc.leaves[k]:
                    be.unit_deinit(u)
                del sc.leaves[k]
        sc.add_voices(int(rng.integers(0, 15)), chain=str(rng.choice(chains)), total=nvoices)
    return np.concatenate(chunks, axis=1)


@pytest.mark.parametrize("seed,nvoices,bfrags", [(1, 3000, 16), (2, 800, 64), (3, 6000, 5), (4, 1500, 1)])
def test_scene_fuzz_matches_oracle(oracle_lib, seed, nvoices, bfrags):
    batches = 4 if bfrags > 1 else 12
    gpu = make_gpu(max_batch=bfrags)
    got = _scene_fuzz(gpu, seed, nvoices, batches, bfrags)
    gpu.close()
    ora = make_oracle(oracle_lib)
    want = _scene_fuzz(ora, seed, nvoices, batches, bfrags)
    ora.close()
    assert want.any() and first_diff(got, want) is None


@pytest.mark.parametrize("seed,nvoices,bfrags,quiet", [(5, 3600, 16, True), (6, 1800, 8, False)])
def test_scene_fuzz_with_osc2_filter_voices_matches_oracle(oracle_lib, seed, nvoices, bfrags, quiet):
    """The same fuzz with 2 x wtosc-filter12-panmix as a sixth chain: 600 voices of it (k_leaf_osc2filtpan beside the
    window kernels: quiet, gliding and record-carrying voices of the class in one batch) and 300 (below A2AMD_O2F_MIN:
    all of them the window kernels')."""
    gpu = make_gpu(max_batch=bfrags)
    infos = []
    got = _scene_fuzz(gpu, seed, nvoices, 4, bfrags, more_chains=["osc2-filter-pan"], on_batch=lambda: infos.append(last_batch(gpu)))
    gpu.close()
    print(seed, infos)
    for bi in infos:
        assert bool(bi.o2f_launched) == quiet and bi.o2f_class >= nvoices // 6 - 48, bi
        assert bi.win_voices > 0 and (quiet or bi.o2f_listed == bi.o2f_class), bi
    assert any(bi.o2f_listed > 0 for bi in infos)
    ora = make_oracle(oracle_lib)
    want = _scene_fuzz(ora, seed, nvoices, 4, bfrags, more_chains=["osc2-filter-pan"])
    ora.close()
    assert want.any() and first_diff(got, want) is None


def test_linearity_at_full_size():
    """Size-independent property at BASELINE size (16384 voices, config 3
    shape would take the oracle minutes): the bus is a wrap-around sum, so the
    render of voices A+B equals render(A) + render(B) mod 2^32 on the root's
    inline bus; the root chain is identity at vol 1, pan 0."""
    def render(sel):
        gpu = make_gpu(max_batch=4)
        sc = synth.Scene(gpu)
        sc.root()
        sc.nvoices = sel[0]
        sc.add_voices(sel[1] - sel[0], chain="osc-filter-pan", total=16384)
        out = sc.run(1, batch=1)
        assert gpu.lib.a2amd_fragment_repeat(gpu.ctx, 64, 3) == 0
        out = np.concatenate([out, gpu.render(3 * 64)], axis=1)
        gpu.close()
        return out
    whole = render((0, 16384))
    parts = render((0, 9000)).astype(np.int64) + render((9000, 16384)).astype(np.int64)
    parts = ((parts + 2**31) % 2**32 - 2**31).astype(np.int32)
    assert whole.any()
    assert first_diff(whole, parts) is None


def _clients_script(be, fragments=14, batch=5, seed=11):
    """A group driver voice (inline; panmix 2->2; xinsert 2 > : a2_NewGroup's
    shape) whose xinsert gets clients while it plays: READ-only ones (the input
    is tapped, a2_SinkCallback), WRITE-only ones (their output is injected,
    a2_SourceCallback), both, none again - with the group walked in split
    windows in some fragments.  Returns (audio, {fragment: tapped input})."""
    rng = np.random.default_rng(seed)
    sc = synth.Scene(be, nwaves=4)
    sc.root()
    k = sc._key()
    g = dict(units=[be.unit_init(k, synth.K_INLINE, 0, 0, 2, 0),
                    be.unit_init(k, synth.K_PANMIX, 0, 2, 2, 0),
                    be.unit_init(k, synth.K_XINSERT, synth.PROCADD, 2, 2, 1)], leaves=[])
    sc.groups.append(g)
    sc.add_voices(5, chain="osc-pan", group=g, total=64)
    sc.add_voices(3, chain="osc-pan", total=64)
    il, pm, xi = g["units"]
    modes = {2: 1, 4: 3, 8: 2, 11: 0}
    mode, chunks, taps, pending = 0, [], {}, []
    for frag in range(fragments):
        be.fragment(64)
        be.unit_process(sc.rootv[0], 0, 64)
        cuts = [0, 64] if frag % 3 else [0, 20, 47, 64]
        for a, b in zip(cuts[:-1], cuts[1:]):
            be.unit_process(il, a, b - a)
            for units in g["leaves"]:
                for u in units:
                    be.unit_process(u, a, b - a)
            be.inline_end(il)
            if a == 20:
                be.unit_write(pm, 0, synth.fix(float(rng.uniform(0.2, 1.0))), 0, 256 * 30)
            be.unit_process(pm, a, b - a)
            if frag in modes and a == 0:
                mode = modes[frag]
                be.unit_clients(xi, mode)
            if mode & 2:
                be.unit_inject(xi, a, rng.integers(-1 << 22, 1 << 22, (2, b - a)))
                if frag % 2:        # a second WRITE client's output adds up
                    be.unit_inject(xi, a, rng.integers(-1 << 20, 1 << 20, (2, b - a)))
            be.unit_process(xi, a, b - a)
        for units in sc.leaves:
            for u in units:
                be.unit_process(u, 0, 64)
        be.inline_end(sc.rootv[0])
        be.unit_process(sc.rootv[1], 0, 64)
        be.unit_process(sc.rootv[2], 0, 64)
        if mode & 1:
            pending.append(frag)
        if frag % batch == batch - 1 or frag == fragments - 1:
            first = frag - frag % batch
            chunks.append(be.render(batch * 64))
            for f in pending:
                taps[f] = be.unit_tapped(xi, f - first)
            pending = []
    # client callbacks need every window: no "everybody sleeps" fragments while there are clients
    be.unit_clients(xi, 1)
    assert getattr(be.lib, be.prefix + "fragment_repeat")(be.ctx, 64, 2) == -4       # A2AMD_EUNSUPPORTED
    be.unit_clients(xi, 0)
    return np.concatenate(chunks, axis=1), taps


def test_xinsert_clients_tap_and_inject(oracle_lib):
    """sink and source clients on an xinsert in the middle of the
    graph (xi_process, src/units/xinsert.c:60-142): same audio, and the sink is
    handed the same input, as on the CPU."""
    gpu = make_gpu(max_batch=8)
    got, gtaps = _clients_script(gpu)
    gpu.close()
    ora = make_oracle(oracle_lib)
    want, wtaps = _clients_script(ora)
    ora.close()
    assert first_diff(got, want) is None
    assert sorted(gtaps) == sorted(wtaps) == [2, 3, 4, 5, 6, 7]
    for f in wtaps:
        assert wtaps[f].any()
        assert np.array_equal(gtaps[f], wtaps[f]), f"tapped input differs in fragment {f}"


def _xio_voices_script(be, fragments=9, batch=4, seed=3):
    """'xsource; panmix' and 'wtosc; xsink; panmix' leaves (the voice shapes of
    test/data/testprograms.a2s StreamVoice / CaptureVoice) plus an adding
    xsource behind an oscillator, clients coming and going."""
    K_XSINK, K_XSOURCE = 18, 19
    rng = np.random.default_rng(seed)
    sc = synth.Scene(be, nwaves=2)
    sc.root()
    sc.add_voices(2, chain="osc-pan", total=64)
    ka, kb, kc, kd = sc._key(), sc._key(), sc._key(), sc._key()
    va = [be.unit_init(ka, K_XSOURCE, 0, 0, 1, 0), be.unit_init(ka, synth.K_PANMIX, synth.PROCADD, 1, 2, 1)]
    vb = [be.unit_init(kb, synth.K_WTOSC, 0, 0, 1, 0), be.unit_init(kb, K_XSINK, 0, 1, 0, 0),
          be.unit_init(kb, synth.K_PANMIX, synth.PROCADD, 1, 2, 1)]
    vc = [be.unit_init(kc, synth.K_WTOSC, 0, 0, 1, 0), be.unit_init(kc, K_XSOURCE, synth.PROCADD, 0, 1, 0),
          be.unit_init(kc, synth.K_PANMIX, synth.PROCADD, 1, 2, 1)]
    # ... and an xinsert in the middle of a chain (in place on the voice's scratch bus)
    vd = [be.unit_init(kd, synth.K_WTOSC, 0, 0, 1, 0), be.unit_init(kd, synth.K_XINSERT, 0, 1, 1, 0),
          be.unit_init(kd, synth.K_PANMIX, synth.PROCADD, 1, 2, 1)]
    for v in (vb, vc, vd):
        be.unit_write(v[0], 0, sc.wave_ids[0])
        be.unit_write(v[0], 1, synth.fix(-0.3))
        be.unit_write(v[0], 2, synth.fix(0.2))
    chunks, taps, pending = [], {}, []
    for frag in range(fragments):
        be.fragment(64)
        be.unit_process(sc.rootv[0], 0, 64)
        for units in sc.leaves:
            for u in units:
                be.unit_process(u, 0, 64)
        if frag == 1:
            be.unit_clients(va[0], 2)
            be.unit_clients(vb[1], 1)
        if frag == 3:
            be.unit_clients(vc[1], 2)
        if frag == 2:
            be.unit_clients(vd[1], 3)
        if frag == 7:
            be.unit_clients(vd[1], 1)
        if frag == 6:
            be.unit_clients(va[0], 0)
            be.unit_clients(vb[1], 0)
        cuts = [0, 64] if frag % 2 else [0, 13, 64]
        for a, b in zip(cuts[:-1], cuts[1:]):
            if 1 <= frag < 6:
                be.unit_inject(va[0], a, rng.integers(-1 << 22, 1 << 22, (1, b - a)))
            if frag >= 3:
                be.unit_inject(vc[1], a, rng.integers(-1 << 22, 1 << 22, (1, b - a)))
            if 2 <= frag < 7:
                be.unit_inject(vd[1], a, rng.integers(-1 << 21, 1 << 21, (1, b - a)))
            for v in (va, vb, vc, vd):
                for u in v:
                    be.unit_process(u, a, b - a)
        be.inline_end(sc.rootv[0])
        be.unit_process(sc.rootv[1], 0, 64)
        be.unit_process(sc.rootv[2], 0, 64)
        if 1 <= frag < 6:
            pending.append(frag)
        if frag % batch == batch - 1 or frag == fragments - 1:
            first = frag - frag % batch
            chunks.append(be.render(batch * 64))
            for f in pending:
                taps[f] = be.unit_tapped(vb[1], f - first)
            for f in range(max(first, 2), frag + 1):
                taps[100 + f] = be.unit_tapped(vd[1], f - first)
            pending = []
    return np.concatenate(chunks, axis=1), taps


def test_xsource_and_xsink_units(oracle_lib):
    gpu = make_gpu(max_batch=4)
    got, gtaps = _xio_voices_script(gpu)
    gpu.close()
    ora = make_oracle(oracle_lib)
    want, wtaps = _xio_voices_script(ora)
    ora.close()
    assert want.any() and first_diff(got, want) is None
    assert sorted(gtaps) == sorted(wtaps) == [1, 2, 3, 4, 5] + [100 + f for f in range(2, 9)]
    for f in wtaps:
        assert wtaps[f].any() and np.array_equal(gtaps[f], wtaps[f]), f"tapped input differs in fragment {f}"


# ---------------------------------------------------------------------------
# round 2: the product loop bench.py times (quiet batches recorded again and again,
# asynchronous readback, graph reuse) and the launch shapes it times
# ---------------------------------------------------------------------------
def _async_steps(gpu, sc, nsteps, B, first=True):
    """bench.py's step loop: fragment_repeat + render(... READBACK|ASYNC) + collect,
    at most two batches in flight.  Returns int32 [2, nsteps*B*64]."""
    import ctypes as C
    lib = gpu.lib
    lib.a2amd_fragment_repeat.argtypes = [C.c_void_p, C.c_uint, C.c_uint]
    lib.a2amd_collect.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_int32)), C.c_uint]
    outs, inflight = [], 0

    def collect():
        out = np.zeros((2, B * 64), dtype=np.int32)
        p = (C.POINTER(C.c_int32) * 2)()
        for c in range(2):
            p[c] = out[c].ctypes.data_as(C.POINTER(C.c_int32))
        assert lib.a2amd_collect(gpu.ctx, p, B * 64) == B * 64, gpu._err(gpu.ctx)
        outs.append(out)

    for s in range(nsteps):
        n = B
        if first and s == 0:
            sc.walk(64)
            n = B - 1
        if n:
            assert lib.a2amd_fragment_repeat(gpu.ctx, 64, n) == 0, gpu._err(gpu.ctx)
        assert gpu._render(gpu.ctx, 4 | 1 | 2 | 8 | 32, None, 0) == B * 64, gpu._err(gpu.ctx)
        inflight += 1
        if inflight == 2:
            collect()
            inflight -= 1
    while inflight:
        collect()
        inflight -= 1
    return np.concatenate(outs, axis=1)


def _oracle_fragments(oracle_lib, build, nfrags):
    import ctypes as C
    ora = make_oracle(oracle_lib)
    oracle_lib.a2o_fragment_repeat.argtypes = [C.c_void_p, C.c_uint, C.c_uint]
    sc = build(ora)
    sc.walk(64)
    outs, done, pending = [], 0, 1
    while done < nfrags:
        n = min(64 - pending, nfrags - done - pending)
        if n:
            assert oracle_lib.a2o_fragment_repeat(ora.ctx, 64, n) == 0
        outs.append(ora.render((pending + n) * 64).copy())
        done += pending + n
        pending = 0
    ora.close()
    return np.concatenate(outs, axis=1)


def test_async_readback_quiet_graph_path_matches_oracle(oracle_lib):
    """Seven steps of 16 fragments through fragment_repeat / render(ASYNC) / collect:
    the second identical quiet batch takes the no-upload path and builds the graph,
    later ones replay it; births in between drop it and the path is found again."""
    def build(be):
        sc = synth.Scene(be)
        sc.root()
        g = sc.add_group(preset="fmtest4")
        sc.add_voices(96, chain="osc2-pan", group=g, total=512)
        sc.add_voices(160, chain="osc-pan", total=512)
        sc.add_voices(64, chain="osc-filter-pan", total=512)
        return sc
    gpu = make_gpu(max_batch=16)
    sc = build(gpu)
    a = _async_steps(gpu, sc, 4, 16)
    sc.add_voices(32, chain="osc-pan", total=512)        # births: slow path, graphs dropped
    sc.walk(64)
    b0 = gpu.render(64)
    b = _async_steps(gpu, sc, 3, 16, first=False)
    gpu.close()
    got = np.concatenate([a, b0, b], axis=1)

    ora = make_oracle(oracle_lib)
    sc = build(ora)
    parts = [sc.run(64, batch=64)]
    sc.add_voices(32, chain="osc-pan", total=512)
    parts.append(sc.run(1 + 48, batch=49))
    ora.close()
    want = np.concatenate(parts, axis=1)
    assert first_diff(got, want) is None


@pytest.mark.parametrize("vpw,ysplit", [(4, 1), (8, 32), (32, 8), (64, 32), (8, 8)])
@pytest.mark.parametrize("chain", ["osc-pan", "osc2-pan"])
def test_leaf_launch_shapes_at_bench_batch_match_oracle(oracle_lib, monkeypatch, chain, vpw, ysplit):
    """The time-sliced leaf kernels at the batch length bench.py times (256 fragments:
    up to 32 slices, each starting from the closed-form phase) over every launch shape
    the host may pick, 2 x 256 fragments, against the oracle."""
    monkeypatch.setenv("A2AMD_VPW", str(vpw))
    monkeypatch.setenv("A2AMD_YSPLIT", str(ysplit))
    n = 2304 if chain == "osc-pan" else 1536

    def build(be):
        sc = synth.Scene(be)
        sc.root()
        sc.add_voices(n, chain=chain, total=4096)
        return sc
    gpu = make_gpu(max_batch=256)
    got = _async_steps(gpu, build(gpu), 2, 256)
    gpu.close()
    want = _oracle_fragments(oracle_lib, build, 512)
    assert first_diff(got, want) is None


@pytest.mark.parametrize("vpw,ysplit", [(4, 1), (4, 8), (32, 8), (8, 3)])
@pytest.mark.parametrize("chain", ["osc-pan", "osc2-pan"])
def test_voices_still_ramping_are_dealt_over_the_time_slices(oracle_lib, monkeypatch, chain, vpw, ysplit):
    """Voices without records in a batch whose rampers are still on their way (long
    pitch glides, fades, pan sweeps started batches ago - what envelopes do) take the
    leaf kernels' per-fragment path; each time slice walks the whole batch for its share
    of them.  Ramps of every length end inside and between the batches."""
    monkeypatch.setenv("A2AMD_VPW", str(vpw))
    monkeypatch.setenv("A2AMD_YSPLIT", str(ysplit))

    def build(be):
        sc = synth.Scene(be)
        sc.root()
        sc.add_voices(900, chain=chain, total=2048)
        for k, units in enumerate(sc.leaves):
            frames = (700, 3000, 5000, 9000, 14000)[k % 5]
            if k % 3 == 0:
                be.unit_write(units[0], 1, synth.fix(((k % 61) - 30) / 12.0 + 0.7), 0, frames << 8)      # pitch glide
            if k % 3 == 1:
                be.unit_write(units[k % (len(units) - 1)], 2, synth.fix(0.0004 * (k % 7)), 0, frames << 8)   # fade
            if k % 4 == 2:
                be.unit_write(units[-1], 1, synth.fix(((k % 9) - 4) / 3.0), 0, frames << 8)                  # pan sweep
            if k % 7 == 3:
                be.unit_write(units[-1], 0, synth.fix(0.5), 0, frames << 8)                                  # volume
        return sc
    gpu = make_gpu(max_batch=64)
    got = _async_steps(gpu, build(gpu), 4, 64)
    gpu.close()
    want = _oracle_fragments(oracle_lib, build, 256)
    assert first_diff(got, want) is None


@pytest.mark.parametrize("fvpw", [1, 8, 32])
def test_filter_leaf_launch_shapes_at_bench_batch_match_oracle(oracle_lib, monkeypatch, fvpw):
    monkeypatch.setenv("A2AMD_FVPW", str(fvpw))

    def build(be):
        sc = synth.Scene(be)
        sc.root()
        sc.add_voices(1100, chain="osc-filter-pan", total=4096)
        return sc
    gpu = make_gpu(max_batch=256)
    got = _async_steps(gpu, build(gpu), 2, 256)
    gpu.close()
    want = _oracle_fragments(oracle_lib, build, 512)
    assert first_diff(got, want) is None


@pytest.mark.parametrize("fvpw", [6, 64])
def test_filter_leaf_paths_mixed_buses_filter_shapes_and_short_fragments(oracle_lib, monkeypatch, fvpw):
    """k_leaf_oscfiltpan's round-3 paths side by side: wavefronts whose voices are all settled (their own
    loop, per voice count 1..6) next to wavefronts with a voice that is not (a q ramp, an amplitude ramp:
    the general loop); workgroups whose voices share one bus (sums meet in LDS) next to workgroups that
    straddle buses; workgroups of pure low pass filters (the row keeps l) next to ones with band / high
    pass mixed in; full fragments, then short ones, then single frames."""
    monkeypatch.setenv("A2AMD_FVPW", str(fvpw))
    outs = []
    for be in (make_gpu(max_batch=32), make_oracle(oracle_lib)):
        sc = synth.Scene(be)
        sc.root()
        groups = [sc.add_bus_group() for _ in range(3)]
        for g, n in zip(groups, (37, 100, 203)):
            sc.add_voices(n, chain="osc-filter-pan", group=g, total=1024)
        sc.add_voices(150, chain="osc-filter-pan", total=1024)
        leaves = [u for g in groups for u in g["leaves"]] + sc.leaves
        for k, units in enumerate(leaves):
            osc, filt, pan = units
            if 128 <= k < 200 and k % 3 == 0:        # band / high pass mixed in: the full output expression
                be.unit_write(filt, 3, synth.fix(0.4))
                be.unit_write(filt, 4, synth.fix(-0.3))
            if k % 53 == 7:                          # q on its way somewhere for 40 ms
                be.unit_write(filt, 1, synth.fix(9.0), 0, 40 << 8)
            if k % 61 == 11:                         # amplitude ramp: the oscillator is not settled
                be.unit_write(osc, 2, synth.fix(0.001), 0, 25 << 8)
        a = sc.run(40, batch=32, frames=64)
        b = sc.run(7, batch=32, frames=23)
        c = sc.run(3, batch=32, frames=1)
        d = sc.run(36, batch=32, frames=64)
        outs.append(np.concatenate([a, b, c, d], axis=1))
        be.close()
    assert first_diff(outs[0], outs[1]) is None


@pytest.mark.parametrize("f2vpw", [1, 8, 32, 36, 48, 64])
def test_osc2_filter_leaf_launch_shapes_at_bench_batch_match_oracle(oracle_lib, monkeypatch, f2vpw):
    """Round 6: k_leaf_osc2filtpan, the quiet kernel of wtosc; wtosc (adding); filter12; panmix (rounds 2-5 rendered
    that voice through the records / window kernels whether or not it carried records), at the batch length bench.py
    times, 2 x 256 fragments against the oracle, over the shapes the launcher may pick - 1 voice per workgroup ... 36
    (every oscillator wavefront in its all-settled loop with at most FILT2_LAUNCHV = 3 voices) - and two it does not:
    48 (4 voices per wavefront: the all-settled loop's 4-voice instantiation, in the kernel but too slow to be dealt)
    and 64 (5 - 6 voices: past FILT2_FASTV, the general loop renders settled voices too)."""
    monkeypatch.setenv("A2AMD_F2VPW", str(f2vpw))

    def build(be):
        sc = synth.Scene(be)
        sc.root()
        sc.add_voices(900, chain="osc2-filter-pan", total=4096)
        return sc
    gpu = make_gpu(max_batch=256)
    got = _async_steps(gpu, build(gpu), 2, 256)
    bi = last_batch(gpu)
    gpu.close()
    print(f2vpw, bi)
    assert bi.o2f_launched and bi.o2f_voices == 900 and bi.o2f_vpg == f2vpw, bi
    assert bi.win_voices == 0 and bi.recs_voices == 0 and bi.general_voices == 0, bi
    want = _oracle_fragments(oracle_lib, build, 512)
    assert want.any()
    assert first_diff(got, want) is None


@pytest.mark.parametrize("f2vpw", [4, 36, 64])
@pytest.mark.parametrize("no_moving", ["1", ""])
def test_osc2_filter_leaf_paths_mixed_buses_filter_shapes_and_short_fragments(oracle_lib, monkeypatch, f2vpw, no_moving):
    """k_leaf_osc2filtpan's paths side by side (the one-oscillator kernel's test above, with the second oscillator):
    wavefronts whose voices are all settled next to wavefronts with a voice whose FIRST oscillator, SECOND oscillator,
    q or pan is on its way somewhere (the general loop: the oscillator through osc_fragment_s, exact for any state);
    workgroups on one bus / straddling buses; pure low pass / band and high pass mixed in; full fragments, short
    ones, single frames.  no_moving = 1 (A2AMD_NO_MOVING): gliding voices stay this kernel's; otherwise they get the
    stand-in record and the window kernels take them for as long as they glide (and the quiet kernel skips them)."""
    monkeypatch.setenv("A2AMD_F2VPW", str(f2vpw))
    if no_moving:
        monkeypatch.setenv("A2AMD_NO_MOVING", no_moving)
    else:
        monkeypatch.delenv("A2AMD_NO_MOVING", raising=False)
    outs, infos = [], []
    for be in (make_gpu(max_batch=32), make_oracle(oracle_lib)):
        sc = synth.Scene(be)
        sc.root()
        # (four bus groups of different sizes and the root's own voices: 640 of the class - from A2AMD_O2F_MIN = 512 on
        # the class has its quiet kernel, below that every voice of it is the records / window kernels')
        groups = [sc.add_bus_group() for _ in range(4)]
        for g, n in zip(groups, (37, 100, 203, 150)):
            sc.add_voices(n, chain="osc2-filter-pan", group=g, total=1024)
        sc.add_voices(150, chain="osc2-filter-pan", total=1024)
        leaves = [u for g in groups for u in g["leaves"]] + sc.leaves
        for k, units in enumerate(leaves):
            osca, oscb, filt, pan = units
            if 128 <= k < 200 and k % 3 == 0:        # band / high pass mixed in: the full output expression
                be.unit_write(filt, 3, synth.fix(0.4))
                be.unit_write(filt, 4, synth.fix(-0.3))
            if k % 53 == 7:                          # q on its way somewhere for 40 ms
                be.unit_write(filt, 1, synth.fix(9.0), 0, 40 << 8)
            if k % 61 == 11:                         # amplitude ramp on the first oscillator
                be.unit_write(osca, 2, synth.fix(0.001), 0, 25 << 8)
            if k % 59 == 5:                          # pitch glide on the second: across a mip level for some
                be.unit_write(oscb, 1, synth.fix(((k % 61) - 30) / 12.0 + 1.3), 0, 30 << 8)
            if k % 47 == 9:                          # amplitude ramp on the second only
                be.unit_write(oscb, 2, synth.fix(0.0007), 0, 33 << 8)
            if k % 43 == 3:                          # pan sweep past the clamp
                be.unit_write(pan, 1, synth.fix(1.4), 0, 20 << 8)
            # ... and the same five kinds over 3 000 - 6 500 frames: still under way in the second batch and after (a glide
            # that ends inside the first batch - all of the above - is never listed: the launch lists are new in that batch)
            if k % 53 == 8:
                be.unit_write(filt, 1, synth.fix(8.0), 0, 3000 << 8)
            if k % 61 == 12:
                be.unit_write(osca, 2, synth.fix(0.0012), 0, 6500 << 8)
            if k % 59 == 6:
                be.unit_write(oscb, 1, synth.fix(((k % 61) - 30) / 12.0 + 1.1), 0, 5000 << 8)
            if k % 47 == 10:
                be.unit_write(oscb, 2, synth.fix(0.0009), 0, 4000 << 8)
            if k % 43 == 4:
                be.unit_write(pan, 1, synth.fix(-1.3), 0, 6000 << 8)
        parts = []
        for nfr, frames in ((40, 64), (7, 23), (3, 1), (36, 64)):
            for at in range(0, nfr, 32):
                parts.append(sc.run(min(32, nfr - at), batch=32, frames=frames))
                if is_gpu(be):
                    infos.append(last_batch(be))
        outs.append(np.concatenate(parts, axis=1))
        be.close()
    print(f2vpw, repr(no_moving), infos)
    assert len(infos) == 6
    for bi in infos:
        # the quiet kernel ran, over the whole class, in the shape this leg is about
        assert bi.o2f_launched and bi.o2f_voices == bi.o2f_class == 640 and bi.o2f_vpg == f2vpw, bi
        assert bi.recs_voices == 0, bi
    # (the batch a voice is born in is the window kernels': its birth and first settings are records)
    assert infos[0].win_voices == 640 and infos[0].n_moving_listed == 0, infos[0]
    # (63 voices have a long glide, 37 of them one that lasts into the last batch)
    for i, bi in enumerate(infos[1:], 1):
        assert bi.general_voices == 0, bi
        if no_moving:       # every gliding voice stays the quiet kernel's: its general loop
            assert bi.n_moving_listed == 0 and bi.win_voices == 0, (i, bi)
        else:               # ... is the window kernels' for as long as it glides
            assert bi.win_voices == bi.n_moving_listed > 0, (i, bi)
    assert outs[1].any()
    assert first_diff(outs[0], outs[1]) is None


def _o2f_scene(be, n, groups=(0.2, 0.35), amp_total=64):
    """n voices of wtosc; wtosc; filter12; panmix: a share of them under each of len(groups) bus groups, the rest under
    the root; band and high pass mixed in for every seventh voice.  (amp_total: add_voices' `total` - the amplitude is
    4.0 / total per oscillator, and filter12 takes its input >> 5: loud enough to leave more than a bit or two of it)"""
    sc = synth.Scene(be)
    sc.root()
    left = n
    for share in groups:
        g = sc.add_bus_group()
        k = int(n * share)
        sc.add_voices(k, chain="osc2-filter-pan", group=g, total=amp_total)
        left -= k
    sc.add_voices(left, chain="osc2-filter-pan", total=amp_total)
    for k, units in enumerate(_o2f_leaves(sc)):
        if k % 7 == 3:
            be.unit_write(units[2], 3, synth.fix(0.4))
            be.unit_write(units[2], 4, synth.fix(-0.3))
    return sc


def _o2f_leaves(sc):
    return [u for g in sc.groups for u in g["leaves"]] + sc.leaves


def _o2f_glides(be, leaves, step, dur):
    """the five kinds of glide k_leaf_osc2filtpan's general loop / the window kernels' closed forms know, on every
    `step`-th voice in turn, over `dur` frames"""
    for k, units in enumerate(leaves):
        osca, oscb, filt, pan = units
        if k % step:
            continue
        kind = (k // step) % 5
        if kind == 0:
            be.unit_write(filt, 1, synth.fix(2.0 + (k % 7)), 0, dur << 8)
        elif kind == 1:
            be.unit_write(osca, 2, synth.fix(0.02 + 0.001 * (k % 9)), 0, dur << 8)
        elif kind == 2:
            be.unit_write(oscb, 1, synth.fix(((k % 61) - 30) / 12.0 + 0.9), 0, dur << 8)
        elif kind == 3:
            be.unit_write(oscb, 2, synth.fix(0.015), 0, dur << 8)
        else:
            be.unit_write(pan, 1, synth.fix(1.4 if k % 2 else -1.2), 0, dur << 8)


def _o2f_walk(sc, rng, frames=64, busy=0, born=()):
    """One fragment of the engine's walk over a scene of _o2f_scene: `busy` voices picked at random get control writes
    between two windows inside the fragment (pitch, amplitude, phase, another wave; cutoff set or swept, q, the filter's
    mix; volume and pan - set, or ramped over up to 7 800 frames), the voices in `born` their first window from a frame
    inside the fragment on, every other voice the default window."""
    be = sc.be
    leaves = _o2f_leaves(sc)
    pick = set(int(k) for k in rng.choice(len(leaves), min(busy, len(leaves)), replace=False)) if busy else set()
    todo = {id(u): k for k, u in enumerate(leaves)}

    def leaf(units):
        k = todo[id(units)]
        for b, off in born:
            if b is units:
                for u in units:
                    be.unit_process(u, off, frames - off)
                return
        if k not in pick or frames < 2:
            for u in units:
                be.unit_process(u, 0, frames)
            return
        osca, oscb, filt, pan = units
        cut = int(rng.integers(1, frames))
        for u in units:
            be.unit_process(u, 0, cut)
        dur = int(rng.choice([0, 100, 3000, 70000, 2000000]))
        start = int(rng.integers(0, 256))
        what = int(rng.integers(0, 8))
        osc = (osca, oscb)[int(rng.integers(0, 2))]
        if what == 0:
            be.unit_write(osc, 0, sc.wave_ids[int(rng.choice([0, 3, 7, 11, 23]))], start, 0)
        elif what == 1:
            be.unit_write(osc, 1, synth.fix(float(rng.uniform(-3, 3))), start, dur)
        elif what == 2:
            be.unit_write(osc, 2, synth.fix(float(rng.uniform(0, 0.1))), start, dur)
        elif what == 3:
            be.unit_write(osc, 3, int(rng.integers(0, 65536)), start, 0)
        elif what == 4:
            be.unit_write(filt, 0, synth.fix(float(rng.uniform(-1, 5))), start, dur)
        elif what == 5:
            be.unit_write(filt, 1, synth.fix(float(rng.uniform(0.2, 9))), start, dur)
        elif what == 6:
            be.unit_write(filt, int(rng.integers(2, 5)), synth.fix(float(rng.uniform(0, 1))), start, dur)
        else:
            be.unit_write(pan, int(rng.integers(0, 2)), synth.fix(float(rng.uniform(-1.5, 1.5))), start, dur)
        for u in units:
            be.unit_process(u, cut, frames - cut)

    be.fragment(frames)
    be.unit_process(sc.rootv[0], 0, frames)
    for g in sc.groups:
        be.unit_process(g["units"][0], 0, frames)
        for units in g["leaves"]:
            leaf(units)
        be.inline_end(g["units"][0])
        for u in g["units"][1:]:
            be.unit_process(u, 0, frames)
    for units in sc.leaves:
        leaf(units)
    be.inline_end(sc.rootv[0])
    be.unit_process(sc.rootv[1], 0, frames)
    be.unit_process(sc.rootv[2], 0, frames)


@pytest.mark.parametrize("win", ["1", "0"])
@pytest.mark.parametrize("n", [511, 512, 513])
def test_osc2_filter_class_at_the_small_scene_threshold(oracle_lib, monkeypatch, n, win):
    """A2AMD_O2F_MIN (512 by default): below it every voice of 2 x wtosc-filter12-panmix is the records / window kernels',
    from it on a voice without records is k_leaf_osc2filtpan's.  511, 512 and 513 voices over two bus groups and the root,
    some gliding, some scripted, three batches of 8 fragments, with the window kernels and with the records kernels."""
    monkeypatch.setenv("A2AMD_WIN", win)
    monkeypatch.delenv("A2AMD_O2F_MIN", raising=False)
    outs, infos = [], []
    for be in (make_gpu(max_batch=8), make_oracle(oracle_lib)):
        rng = np.random.default_rng(n)
        sc = _o2f_scene(be, n)
        _o2f_glides(be, _o2f_leaves(sc), 9, 900)
        parts = []
        for b in range(3):
            for f in range(8):
                _o2f_walk(sc, rng, busy=0 if b == 0 else 20)
            parts.append(be.render(8 * 64))
            if is_gpu(be):
                infos.append(last_batch(be))
        outs.append(np.concatenate(parts, axis=1))
        be.close()
    print(n, win, infos)
    for b, bi in enumerate(infos):
        assert bi.o2f_class == n and bool(bi.o2f_launched) == (n >= 512), bi
        assert (bi.win_voices if win == "1" else bi.recs_voices) == bi.o2f_listed and bi.general_voices == 0, bi
        assert (bi.recs_voices if win == "1" else bi.win_voices) == 0, bi
        if n < 512 or b == 0:
            assert bi.o2f_listed == n, bi       # (b == 0: every voice carries the records of its birth)
        else:
            assert 20 <= bi.o2f_listed < 300 and bi.o2f_voices == n and bi.o2f_vpg == auto_o2f_vpg(n, bi.o2f_max_vpg), bi
    assert outs[1].any()
    assert first_diff(outs[0], outs[1]) is None


@pytest.mark.parametrize("win", ["1", "0"])
def test_osc2_filter_voices_cross_the_small_scene_threshold_both_ways(oracle_lib, monkeypatch, win):
    """The hand-over of a voice between the records / window kernels and k_leaf_osc2filtpan when its class crosses
    A2AMD_O2F_MIN between batches: 510 voices; births inside a batch take the class to 514; deaths take it to 509.  Voices
    glide (q, both oscillators' amplitude, pitch, pan: for 1 400 frames, begun again in every second batch) and carry
    records in every batch, so filter state, oscillator phases and rampers in mid-flight change hands in both directions;
    which kernel had the class is asserted batch by batch."""
    monkeypatch.setenv("A2AMD_WIN", win)
    monkeypatch.delenv("A2AMD_O2F_MIN", raising=False)
    #        class size the batch is rendered with (a voice that dies is its class's until the batch it dies in is over)
    plan = [510, 510, 514, 514, 514, 509, 509]
    outs, infos = [], []
    for be in (make_gpu(max_batch=8), make_oracle(oracle_lib)):
        rng = np.random.default_rng(77)
        sc = _o2f_scene(be, 510)
        parts = []
        for b in range(len(plan)):
            if b % 2 == 1:
                _o2f_glides(be, _o2f_leaves(sc), 11 + b, 1400)
            for f in range(8):
                born = []
                if b == 2 and f in (1, 2, 5, 6):        # a note begins inside a fragment: 510 -> 514 in this batch
                    g = sc.groups[f % 2] if f < 5 else None
                    sc.add_voices(1, chain="osc2-filter-pan", group=g, total=64)
                    born = [((g["leaves"] if g else sc.leaves)[-1], 5 + 9 * f)]
                _o2f_walk(sc, rng, busy=24, born=born)
                if b == 4 and f in (0, 2, 3, 6, 7):     # ... and notes end: 509 from the next batch on
                    l = (sc.groups[0]["leaves"], sc.groups[1]["leaves"], sc.leaves)[f % 3]
                    k = int(rng.integers(0, len(l)))
                    for u in l[k]:
                        be.unit_deinit(u)
                    del l[k]
            parts.append(be.render(8 * 64))
            if is_gpu(be):
                infos.append(last_batch(be))
        outs.append(np.concatenate(parts, axis=1))
        be.close()
    print(win, infos)
    for b, bi in enumerate(infos):
        assert bi.o2f_class == plan[b] and bool(bi.o2f_launched) == (plan[b] >= 512), (b, bi)
        assert (bi.win_voices if win == "1" else bi.recs_voices) == bi.o2f_listed and bi.general_voices == 0, (b, bi)
        if plan[b] < 512:
            assert bi.o2f_listed == plan[b], (b, bi)
        else:
            assert 24 <= bi.o2f_listed < 300 and bi.o2f_voices == plan[b], (b, bi)
    assert outs[1].any()
    assert first_diff(outs[0], outs[1]) is None


@pytest.mark.parametrize("n", [512, 513, 768, 769, 770, 771, "256*max", "256*max+1"])
def test_osc2_filter_leaf_automatic_shapes_match_oracle(oracle_lib, monkeypatch, n):
    """The shape the launcher picks by itself (no A2AMD_F2VPW) at the class sizes where it steps: 2 -> 3 voices per
    workgroup at 513, 3 -> 4 at 769; a last workgroup - and a last oscillator wavefront - of 1, 2 and 3 voices (769, 770,
    771 at 4 per workgroup); one round of 256 workgroups full to the last voice at 256 x a2d_osc2filtpan_max_vpg(), two
    rounds from one voice more.  Few fragments, so the oracle stays cheap: 3 (the voices' births: the window kernels',
    the quiet kernel launched over a class it skips entirely), then 5 and 2 quiet ones."""
    monkeypatch.delenv("A2AMD_F2VPW", raising=False)
    monkeypatch.delenv("A2AMD_O2F_MIN", raising=False)
    maxv = 36       # (checked against what the library reports below)
    nv = 256 * maxv if n == "256*max" else 256 * maxv + 1 if n == "256*max+1" else n
    outs, infos = [], []
    for be in (make_gpu(max_batch=8), make_oracle(oracle_lib)):
        sc = _o2f_scene(be, nv, amp_total=max(64, nv // 16))
        parts = []
        for nfr in (3, 5, 2):
            parts.append(sc.run(nfr, batch=8))
            if is_gpu(be):
                infos.append(last_batch(be))
        outs.append(np.concatenate(parts, axis=1))
        be.close()
    print(n, infos)
    for bi in infos:
        assert bi.o2f_max_vpg == maxv, "the test's sizes were chosen for a2d_osc2filtpan_max_vpg() == 36"
        assert bi.o2f_launched and bi.o2f_voices == bi.o2f_class == nv and bi.o2f_vpg == auto_o2f_vpg(nv, maxv), bi
    assert [bi.win_voices for bi in infos] == [nv, 0, 0], infos
    assert infos[0].o2f_vpg == {512: 2, 513: 3, 768: 3, 769: 4, 770: 4, 771: 4, "256*max": 36, "256*max+1": 19}[n]
    assert outs[1].any()
    assert first_diff(outs[0], outs[1]) is None


def _repeat_batch(be, sc, frames, count):
    """one fragment walked by calls and count - 1 repeats of it (fragment_repeat), rendered as ONE batch on the GPU and
    in pieces of at most 64 fragments by the oracle"""
    fr = be.lib.a2amd_fragment_repeat if is_gpu(be) else be.lib.a2o_fragment_repeat
    fr.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint]
    sc.walk(frames)
    parts, done, pending = [], 0, 1
    step = count if is_gpu(be) else 64
    while done < count:
        n = min(step - pending, count - done - pending)
        if n:
            assert fr(be.ctx, frames, n) == 0
        parts.append(be.render((pending + n) * frames).copy())
        done += pending + n
        pending = 0
    return np.concatenate(parts, axis=1)


@pytest.mark.parametrize("no_moving", ["", "1"])
@pytest.mark.parametrize("f2vpw", [0, 48, 64])
def test_osc2_filter_leaf_batch_lengths_and_fragment_lengths_match_oracle(oracle_lib, monkeypatch, f2vpw, no_moving):
    """k_leaf_osc2filtpan over batches that are not a whole number of its fragment chunks - 1 fragment, 7, 255 - and over
    fragments of 64 frames, 23, 17 and single frames, in the shape the launcher picks (600 voices: 3 per workgroup), in
    the 4-voice all-settled loop (48) and in the general loop for settled voices (64); voices gliding for 9 000 frames are
    the window kernels' for that long, or (no_moving) the quiet kernel's own."""
    if f2vpw:
        monkeypatch.setenv("A2AMD_F2VPW", str(f2vpw))
    else:
        monkeypatch.delenv("A2AMD_F2VPW", raising=False)
    if no_moving:
        monkeypatch.setenv("A2AMD_NO_MOVING", no_moving)
    else:
        monkeypatch.delenv("A2AMD_NO_MOVING", raising=False)
    batches = [(1, 64), (7, 64), (255, 23), (5, 1), (255, 64), (1, 1), (9, 17), (1, 64)]
    outs, infos = [], []
    for be in (make_gpu(max_batch=255), make_oracle(oracle_lib)):
        sc = _o2f_scene(be, 600, groups=(0.1, 0.3, 0.25))
        _o2f_glides(be, _o2f_leaves(sc), 13, 9000)
        parts = []
        for count, frames in batches:
            parts.append(_repeat_batch(be, sc, frames, count))
            if is_gpu(be):
                infos.append(last_batch(be))
        outs.append(np.concatenate(parts, axis=1))
        be.close()
    print(f2vpw, repr(no_moving), infos)
    for b, bi in enumerate(infos):
        assert bi.o2f_launched and bi.o2f_voices == 600 and bi.o2f_vpg == (f2vpw or 3), (b, bi)
        assert bi.recs_voices == 0 and bi.general_voices == 0, (b, bi)
        if b == 0:
            assert bi.win_voices == 600, bi
        elif no_moving:
            assert bi.win_voices == 0 and bi.n_moving_listed == 0, (b, bi)
        elif b in (1, 2, 3):        # (frames 64 ... 6 382 of the glides' 9 000)
            assert bi.win_voices == bi.n_moving_listed > 0, (b, bi)       # (47 voices glide)
    assert outs[1].any()
    assert first_diff(outs[0], outs[1]) is None


@pytest.mark.parametrize("groups", [0, 3])
def test_osc2_filter_small_scene_records_without_the_records_kernel_match_oracle(oracle_lib, monkeypatch, groups):
    """A2AMD_NO_FAST=64 (records to the general kernel) in a small scene: a 2 x wtosc-filter12-panmix voice that carries
    records is the general kernel's, one without is the records kernel's (below A2AMD_O2F_MIN the class has no quiet
    kernel) - each voice on ONE of the two lists.  (Until this test the voice with records stood on both and was rendered
    twice: upload() marked it as listed only where the records kernels took it.)"""
    monkeypatch.setenv("A2AMD_WIN", "0")
    monkeypatch.setenv("A2AMD_NO_FAST", "64")
    gpu = make_gpu(max_batch=16)
    infos = []
    got = _wt_script(gpu, "osc2-filter-pan", groups=groups, on_batch=lambda: infos.append(last_batch(gpu)))
    gpu.close()
    print(groups, infos)
    for bi in infos:
        assert not bi.o2f_launched and bi.win_voices == 0 and bi.general_voices > 0, bi
        assert bi.o2f_listed + bi.general_voices <= bi.o2f_class, f"a voice on two lists: {bi}"
    ora = make_oracle(oracle_lib)
    want = _wt_script(ora, "osc2-filter-pan", groups=groups)
    ora.close()
    assert want.any()
    assert first_diff(got, want) is None


def test_subtractive_note_at_full_size_matches_oracle_golden():
    """16 384 x wtosc; wtosc; filter12; panmix (round 5's review: the shape of every benchmark/k2*.a2s lead, "a quiet
    kernel of its own") at FULL size, 2 steps of 256 fragments, against the per-fragment hashes the CPU oracle
    rendered in the build container (tests/golden/make_bench_golden.py)."""
    import bench
    want = np.load(bench.golden_path(16384, "osc2-filter-pan", 0))
    gpu = make_gpu(max_batch=256)
    sc = bench.build_scene(gpu, 16384, "osc2-filter-pan", 0)
    got = fnv1a_fragments(_async_steps(gpu, sc, 2, 256))
    gpu.close()
    assert len(want) >= len(got)
    bad = np.nonzero(got != want[:len(got)])[0]
    assert not len(bad), f"{len(bad)} fragments differ, first {bad[:8]}"


@pytest.mark.parametrize("nfilt", [8, 13])
def test_long_chains_match_oracle(oracle_lib, nfilt):
    """Round 6: a voice's chain may hold 16 units (8 before; the reference's list has no cap, core.c:163-300 - 16 is what a
    command record's 4-bit chain position addresses).  wtosc; wtosc (adding); nfilt x filter12 in series (each in place:
    the voice's scratch, as the engine wires a 1 -> 1 unit); panmix = 11 and 16 units, 60 voices, control writes to the
    LAST filter and the pan between batches (records whose unit field is 9 - 15), against the oracle; a 17th unit is
    refused loudly."""
    from audiality2_amd.synth import K_WTOSC, K_FILTER12, K_PANMIX, PROCADD, fix
    outs = []
    for be in (make_gpu(max_batch=16), make_oracle(oracle_lib)):
        sc = synth.Scene(be)
        sc.root()
        voices = []
        for k in range(60):
            key = sc._key()
            units = [be.unit_init(key, K_WTOSC, 0, 0, 1, 0), be.unit_init(key, K_WTOSC, PROCADD, 0, 1, 0)]
            units += [be.unit_init(key, K_FILTER12, 0, 1, 1, 0) for _ in range(nfilt)]
            units.append(be.unit_init(key, K_PANMIX, PROCADD, 1, 2, 1))
            p = fix(((k % 31) - 15) / 12.0)
            for j, o in enumerate(units[:2]):
                be.unit_write(o, 0, sc.wave_ids[(5 * k + j) % len(sc.wave_ids)])
                be.unit_write(o, 1, p + (fix(0.02) if j else 0))
                be.unit_write(o, 2, fix(0.02))
            for j, f in enumerate(units[2:-1]):
                be.unit_write(f, 0, p + fix(3.0 + 0.1 * j))      # cutoff, well above the note: eight low passes in a row
                be.unit_write(f, 1, fix(1.0))
            be.unit_write(units[-1], 1, fix(((k % 9) - 4) / 4.0))
            voices.append(units)
            sc.leaves.append(units)
        parts = [sc.run(16, batch=16)]
        for k, units in enumerate(voices):
            if k % 3 == 0:
                be.unit_write(units[-2], 0, fix(2.0), 0, 20 << 8)           # the last filter's cutoff, ramping
            if k % 4 == 1:
                be.unit_write(units[-1], 1, fix(-0.5), 0, 15 << 8)          # the pan: chain position nfilt + 2
            if k % 5 == 2:
                be.unit_write(units[-2], 1, fix(4.0), 0, 10 << 8)           # the last filter's q
        parts.append(sc.run(32, batch=16))
        outs.append(np.concatenate(parts, axis=1))
        if be is not None and len(outs) == 1:
            # (one more unit than the record format addresses)
            key = sc._key()
            for _ in range(16):
                be.unit_init(key, K_FILTER12, 0, 1, 1, 0)
            with pytest.raises(Exception):
                be.unit_init(key, K_PANMIX, PROCADD, 1, 2, 1)
        be.close()
    assert outs[1].any()
    assert first_diff(outs[0], outs[1]) is None


@pytest.mark.parametrize("config", [1, 2, 3])
def test_baseline_configs_at_full_size_match_oracle_golden(config):
    """BASELINE configs[1..3] at FULL size (1 024 / 16 384 / 65 536 voices, 512
    fbdelays in configs[3]), 8 steps of 256 fragments = 2.73 s of audio, against the
    per-fragment hashes the CPU oracle rendered in the build container
    (tests/golden/make_bench_golden.py; minutes of oracle time)."""
    import bench
    cfg = bench.CONFIGS[config]
    want = np.load(bench.golden_path(cfg["voices"], cfg["chain"], cfg["groups"]))
    gpu = make_gpu(max_batch=256)
    sc = bench.build_scene(gpu, cfg["voices"], cfg["chain"], cfg["groups"])
    got = fnv1a_fragments(_async_steps(gpu, sc, 8, 256))
    gpu.close()
    assert len(want) >= len(got)        # (the golden covers every step of bench.py's default run; 8 steps here)
    bad = np.nonzero(got != want[:len(got)])[0]
    assert not len(bad), f"configs[{config}]: {len(bad)} fragments differ, first {bad[:8]}"


@pytest.mark.parametrize("raw", ["", "0"])
def test_private_wave_scene_at_full_size_matches_oracle_golden(monkeypatch, raw):
    """bench.py --config 5 (SURVEY 8d's private-wave case): 65 536 wtosc -> panmix voices over 2 048 uploaded
    sample waves of 65 536 samples - 0.54 GB of wave data, 3.2 GB of coefficient entries, addressed past
    2^31 bytes - two steps of 256 fragments against the oracle's hashes; as the footprint policy plays it
    (from the samples) and with the coefficient entries forced."""
    import bench
    if raw:
        monkeypatch.setenv("A2AMD_RAW", raw)
    else:
        monkeypatch.delenv("A2AMD_RAW", raising=False)
    cfg = bench.CONFIGS[5]
    want = np.load(bench.golden_path(cfg["voices"], cfg["chain"], cfg["groups"], private=cfg["private"]))
    gpu = make_gpu(max_batch=256)
    sc = bench.build_scene(gpu, cfg["voices"], cfg["chain"], cfg["groups"], private=cfg["private"])
    got = fnv1a_fragments(_async_steps(gpu, sc, 2, 256))
    gpu.close()
    bad = np.nonzero(got != want)[0]
    assert not len(bad), f"private-wave scene: {len(bad)} fragments differ, first {bad[:8]}"


def test_config3_full_size_is_linear_in_the_voice_subsets():
    """Size-independent property at configs[3]'s full size: the mix is a wrap-around
    integer sum, the group chains (fbdelay with constant gains) and the root chain
    (unity gains) are linear up to their truncating shifts ... which are NOT linear,
    so the exact statement is per group: a scene holding only groups [0, 128) plus a
    scene holding only groups [128, 256) renders, group bus by group bus, what the
    full scene renders - and with the root at vol 1.0, pan 0 (panmix.c:259: an exact
    identity on each channel) the master buses add up bit for bit."""
    import bench
    cfg = bench.CONFIGS[3]
    outs = []
    for lo, hi in ((0, 256), (0, 128), (128, 256)):
        gpu = make_gpu(max_batch=256)
        sc = synth.Scene(gpu)
        sc.root()
        per = cfg["voices"] // cfg["groups"]
        for gi in range(cfg["groups"]):
            if lo <= gi < hi:
                grp = sc.add_group(preset="fmtest4")
                sc.add_voices(per, chain=cfg["chain"], group=grp, total=cfg["voices"])
            else:
                sc.nvoices += per       # (voice parameters depend on the voice's number)
        outs.append(_async_steps(gpu, sc, 3, 256))
        gpu.close()
    full, a, b = (o.astype(np.int64) for o in outs)
    s = ((a + b + 2 ** 31) % 2 ** 32 - 2 ** 31)
    assert first_diff(full.astype(np.int32), s.astype(np.int32)) is None


@pytest.mark.parametrize("batch", [16, 64, 256])
def test_delay_chain_kernel_rounds_match_oracle(oracle_lib, batch):
    """k_bus_fbdchain: five group voices inline->fbdelay->fbdelay - every chain has exactly
    two delays - with taps of 1.4 .. 29 fragments (rounds of 1, 3 and 9 fragments, several
    rounds per batch) and fmtest4's (one round), one with a tap shorter than a fragment
    (general kernel), delay times rewritten half way; the frame-parallel rounds must give
    what the oracle's sample-by-sample loop gives.  Chains of one, three, four and five
    delays, an adding middle delay and the taps at the edges of the class are in
    tests/test_gpu_bus_paths.py."""
    outs = []
    for be in (make_gpu(max_batch=batch), make_oracle(oracle_lib)):
        sc = synth.Scene(be)
        sc.root()
        groups = [sc.add_group(fb=(1.9, 2.4, 3.1), gains=(0.4, 0.3, 0.3)),
                  sc.add_group(fb=(4.2, 5.0, 6.3), gains=(0.5, 0.25, 0.25)),
                  sc.add_group(fb=(12.7, 20.0, 38.9), gains=(0.3, 0.4, 0.2)),
                  sc.add_group(fb=(1.2, 0.5, 137.9), gains=(0.2, 0.3, 0.3)),
                  sc.add_group(preset="fmtest4")]
        for g in groups:
            sc.add_voices(24, chain="osc2-pan", group=g, total=256)
        a = sc.run(3 * batch + 5, batch=batch)
        # a tap of the second group drops below one fragment (-> general kernel), one
        # of the fourth grows above (-> delay kernel)
        be.unit_write(groups[1]["units"][1], 1, synth.fix(0.9))
        be.unit_write(groups[3]["units"][2], 1, synth.fix(3.3))
        be.unit_write(groups[3]["units"][2], 0, synth.fix(2.0))
        be.unit_write(groups[3]["units"][1], 0, synth.fix(7.7))
        be.unit_write(groups[3]["units"][1], 1, synth.fix(3.5))
        b = sc.run(2 * batch + 3, batch=batch)
        outs.append(np.concatenate([a, b], axis=1))
        be.close()
    assert first_diff(outs[0], outs[1]) is None


def _dist_one_rank():
    """(body of the test below; runs in a process of its own)"""
    import ctypes as C
    outs = []
    for use_dist in (False, True):
        gpu = make_gpu(max_batch=32)
        if use_dist:
            lib = gpu.lib
            lib.a2amd_dist_unique_id.argtypes = [C.c_void_p]
            lib.a2amd_dist_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
            idbuf = (C.c_uint8 * 128)()
            assert lib.a2amd_dist_unique_id(idbuf) == 0
            assert lib.a2amd_dist_init(gpu.ctx, idbuf, 0, 1) == 0, gpu._err(gpu.ctx)
        sc = synth.Scene(gpu)
        sc.root()
        g = sc.add_group(preset="fmtest4")
        sc.add_voices(64, chain="osc2-pan", group=g, total=512)
        g2 = sc.add_group()
        sc.add_voices(32, chain="osc-filter-pan", group=g2, total=512)
        sc.add_voices(200, chain="osc-pan", total=512)
        sc.add_voices(16, chain="fm2-pan", total=512)
        outs.append(_async_steps(gpu, sc, 5, 32))
        gpu.close()
    assert outs[0].any()
    assert first_diff(outs[0], outs[1]) is None


def test_dist_render_with_one_rank_equals_plain_render():
    """a2amd_dist_init(): the multi-GPU batch (subtrees, ONE ncclReduce of the root bus on
    the render stream, root chain on rank 0) with a communicator of one rank - all this
    box can form - must render what the plain path renders, batch after batch (the reduce
    of one rank's partial onto itself, bus hygiene between the split phases, graphs of
    the split phases).  In a process of its own, as an application would be: this test
    process may by now hold two ROCm runtimes (the system's, which liba2amd.so is linked
    against, and the copy bundled with torch, which other tests import), and RCCL then
    finds the wrong one."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]; import test_gpu_parity as t; "
                        "t._dist_one_rank()" % (os.path.dirname(os.path.abspath(__file__)), ROOT)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]


def test_render_group_of_two_contexts_equals_one_context():
    """a2amd_dist_init_local() / a2amd_render_group(): ONE voice tree spread over two
    contexts of this process (each with its own copy of the root voice; the groups and
    the voices under the root dealt alternately), their root-bus partials summed, the
    root chain on context 0 - must render what one context holding all of it renders.
    (Both contexts on this box's one GPU: the exchange is the device-local add; with
    distinct GPUs the same entry point issues the RCCL group reduce.)"""
    import ctypes as C
    B, steps, ngroups, per = 16, 4, 6, 24

    def populate(sc, mine):
        for gi in range(ngroups):
            if mine(gi):
                grp = sc.add_group(preset="fmtest4") if gi % 2 else sc.add_group()
                sc.add_voices(per, chain="osc2-pan" if gi % 3 else "osc-filter-pan", group=grp, total=512)
            else:
                sc.nvoices += per
        for k in range(4):          # ... and voices straight under the root
            if mine(ngroups + k):
                sc.add_voices(16, chain="osc-pan", total=512)
            else:
                sc.nvoices += 16

    one = make_gpu(max_batch=B)
    sc = synth.Scene(one)
    sc.root()
    populate(sc, lambda i: True)
    want = _async_steps(one, sc, steps, B)
    one.close()

    a, b = make_gpu(max_batch=B), make_gpu(max_batch=B)
    lib = a.lib
    lib.a2amd_dist_init_local.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    lib.a2amd_render_group.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_uint, C.POINTER(C.POINTER(C.c_int32)), C.c_uint]
    lib.a2amd_fragment_repeat.argtypes = [C.c_void_p, C.c_uint, C.c_uint]
    ctxs = (C.c_void_p * 2)(a.ctx, b.ctx)
    assert lib.a2amd_dist_init_local(ctxs, 2) == 0, a._err(a.ctx)
    scs = []
    for be, parity in ((a, 0), (b, 1)):
        s2 = synth.Scene(be)
        s2.root()
        populate(s2, lambda i, parity=parity: i % 2 == parity)
        scs.append(s2)
    outs = []
    for s in range(steps):
        n = B
        if s == 0:
            for s2 in scs:
                s2.walk(64)
            n = B - 1
        for be in (a, b):
            assert lib.a2amd_fragment_repeat(be.ctx, 64, n) == 0, be._err(be.ctx)
        out = np.zeros((2, B * 64), dtype=np.int32)
        p = (C.POINTER(C.c_int32) * 2)()
        for c in range(2):
            p[c] = out[c].ctypes.data_as(C.POINTER(C.c_int32))
        assert lib.a2amd_render_group(ctxs, 2, 15, p, B * 64) == B * 64, a._err(a.ctx)
        outs.append(out)
    a.close()
    b.close()
    got = np.concatenate(outs, axis=1)
    assert want.any() and first_diff(got, want) is None


# ---------------------------------------------------------------------------
# round 3: BASELINE configs[4] - 8 top-level groups (a2_NewGroup,
# src/interface.c:888) x 128 sub-groups x 256 wtosc->filter12->panmix voices = 262 144
# voices, group g -> GPU g, ONE reduce of the root voice's inline bus per buffer
# ---------------------------------------------------------------------------
def _cfg4_group(contexts, devices=None, fragments=64):
    """The whole configs[4] scene dealt over `contexts` contexts (top-level group g on
    context g * contexts // 8) through a2amd_dist_init_local / a2amd_render_group;
    returns the per-fragment hashes of the audio context 0 delivers."""
    import ctypes as C
    import audiality2_amd
    import bench
    cfg = bench.CONFIGS[4]
    total, per = 262144, 262144 // contexts
    bes = [audiality2_amd.open_backend(48000, None, 2, device=(devices[i] if devices else 0), max_batch=fragments)
           for i in range(contexts)]
    lib = bes[0].lib
    lib.a2amd_dist_init_local.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    lib.a2amd_render_group.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_uint, C.POINTER(C.POINTER(C.c_int32)), C.c_uint]
    lib.a2amd_fragment_repeat.argtypes = [C.c_void_p, C.c_uint, C.c_uint]
    ctxs = (C.c_void_p * contexts)(*[be.ctx for be in bes])
    if contexts > 1:
        assert lib.a2amd_dist_init_local(ctxs, contexts) == 0, bes[0]._err(bes[0].ctx)
    for i, be in enumerate(bes):
        # rank i of `contexts`: its voices are numbered from i * per, amplitudes follow the whole job's size
        sc = bench.build_scene(be, per, cfg["chain"], 0, world=contexts, rank=i, tree=cfg["tree"])
        sc.walk(64)
        assert lib.a2amd_fragment_repeat(be.ctx, 64, fragments - 1) == 0, be._err(be.ctx)
    out = np.zeros((2, fragments * 64), dtype=np.int32)
    p = (C.POINTER(C.c_int32) * 2)()
    for c in range(2):
        p[c] = out[c].ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.a2amd_render_group(ctxs, contexts, 15, p, fragments * 64) == fragments * 64, bes[0]._err(bes[0].ctx)
    for be in bes:
        be.close()
    return fnv1a_fragments(out)


def _cfg4_golden():
    import bench
    cfg = bench.CONFIGS[4]
    return np.load(bench.golden_path(262144, cfg["chain"], 0, cfg["tree"]))


@pytest.mark.parametrize("contexts", [1, 8])
def test_config4_full_size_matches_oracle_golden(contexts):
    """All 262 144 voices of configs[4] on this box's GPU: in ONE context, and as the
    8-GPU job lays it out - one context per top-level group, each with its own copy of
    the root voice, the eight root-bus partials summed, the root chain on context 0
    (a2amd_render_group; on one GPU the sum is the device-local add) - against the 64
    fragments the CPU oracle rendered of the whole scene (make_bench_golden.py 4)."""
    want = _cfg4_golden()
    got = _cfg4_group(contexts, fragments=len(want))
    bad = np.nonzero(got != want)[0]
    assert not len(bad), f"configs[4] over {contexts} context(s): {len(bad)} fragments differ, first {bad[:8]}"


def _cfg4_rccl(n):
    """(body of the test below, in a process of its own: see test_dist_render_with_one_rank...)"""
    want = _cfg4_golden()
    got = _cfg4_group(n, devices=list(range(n)), fragments=len(want))
    bad = np.nonzero(got != want)[0]
    assert not len(bad), f"configs[4] over {n} GPUs: {len(bad)} fragments differ, first {bad[:8]}"


@pytest.mark.parametrize("n", [2, 4, 8])
def test_config4_over_distinct_gpus_matches_oracle_golden(n):
    """The same with the contexts on DISTINCT GPUs: ncclCommInitAll + one grouped
    ncclReduce(int32, sum) of the root bus over xGMI inside a2amd_render_group.  Needs
    n visible GPUs (the single-GPU test box skips; an 8-GPU node runs all three)."""
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() < n:
        pytest.skip(f"{torch.cuda.device_count()} GPU(s) visible, {n} needed")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]; import test_gpu_parity as t; "
                        "t._cfg4_rccl(%d)" % (os.path.dirname(os.path.abspath(__file__)), ROOT, n)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]


# ---- a wave built on the device from what the device rendered --------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("length,looped,mip", [(2000, False, False), (733, True, False), (3001, False, True), (4096, True, True),
                                               (130, True, True), (5, True, True), (1, False, True), (64, False, True)])
def test_wave_built_from_a_capture_equals_the_uploaded_wave(oracle_lib, length, looped, mip):
    """a2amd_capture_begin / _end + a2amd_wave_upload_captured (the device-resident half of a2_RenderWave)
    through the C ABI, without the engine: a context renders `length` frames of a small scene - fragments of 64 and a
    partial last one, several batches - with the capture on; a second context builds a wave from the capture ON THE
    DEVICE (level 0 = samples >> 8, pads, mip levels: src/waves.c:89-130, 174-177).  A third context and the oracle
    get the same wave the host way: the rendered PCM converted and mip-mapped by synth.wave_pyramid (the numpy
    restatement of those functions, pinned on the reference's built-in waves) and uploaded.  The same voices, over all
    mip levels, on each of the three: identical audio.  One-shot and looped, plain and mip-mapped, lengths below the
    pad (130), below a mip level's reach (5, 1), a whole number of fragments (64, 4096)."""
    from audiality2_amd.replay import a2amd_wavedesc
    sub = make_gpu(max_batch=8)
    lib = sub.lib
    lib.a2amd_capture_begin.argtypes = [ctypes.c_void_p]
    lib.a2amd_capture_end.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    lib.a2amd_capture_frames.argtypes = [ctypes.c_void_p]
    lib.a2amd_capture_frames.restype = ctypes.c_uint
    lib.a2amd_capture_free.argtypes = [ctypes.c_void_p]
    lib.a2amd_wave_upload_captured.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(a2amd_wavedesc), ctypes.c_void_p]
    assert lib.a2amd_capture_begin(sub.ctx) == 0
    sc = synth.Scene(sub)
    sc.root()
    sc.add_voices(24, chain="osc-filter-pan")
    pcm, left, pending = [], length, 0
    while left:
        n = min(64, left)
        sc.walk(n)
        left -= n
        pending += n
        if pending >= 7 * 64 or not left:
            pcm.append(sub.render(pending))
            pending = 0
    pcm = np.concatenate(pcm, axis=1)[0]
    cap = ctypes.c_void_p()
    assert lib.a2amd_capture_end(sub.ctx, ctypes.byref(cap)) == 0 and cap.value
    assert lib.a2amd_capture_frames(cap) == length == len(pcm)
    sub.close()                                     # (the capture outlives its context)
    assert length < 64 or np.abs(pcm).max() > 256
    levels = synth.MIPLEVELS if mip else 1
    sizes, data = synth.wave_pyramid((pcm >> 8).astype(np.int16), looped=looped, levels=levels)
    wtype, flags, period = (synth.WMIPWAVE if mip else synth.WWAVE), (synth.LOOPED if looped else 0), 64
    outs = []
    for how in ("captured", "uploaded", "oracle"):
        be = make_oracle(oracle_lib) if how == "oracle" else make_gpu(max_batch=8)
        s2 = synth.Scene(be)
        if how == "captured":
            d = a2amd_wavedesc()
            d.type, d.flags, d.period = wtype, flags, period
            for lv in range(levels):
                d.size[lv] = sizes[lv]
            wid = lib.a2amd_wave_upload_captured(be.ctx, 0x7777, ctypes.byref(d), cap)
            assert wid >= 0, be._err(be.ctx)
        else:
            wid = be.wave_upload(0x7777, wtype, flags, period, sizes + [0] * (synth.MIPLEVELS - len(sizes)), data)
        s2.private_ids = [wid]
        s2.root()
        s2.add_voices(61, chain="osc-pan", private=True)
        outs.append(s2.run(24, batch=8))
        be.close()
    lib.a2amd_capture_free(cap)
    assert np.array_equal(outs[1], outs[2]), "uploaded wave: GPU vs oracle"
    assert np.array_equal(outs[0], outs[1]), "wave built from the capture vs the uploaded one"
    if length >= 64:
        assert outs[0].any()
