"""Rendered waves with "normalize" and / or "xfade", post-processed on the device (DESIGN 3a,
include/a2amd_wavepost.h): the peak search per written chunk, the gain, the float conversion and the crossfade of
src/waves.c:155-346, 405-451 - bit for bit, so nothing here has a tolerance.

The CPU part pins the arithmetic - a2amd_wavepost_host() (plain C++, written like the reference) and
synth.wave_postprocess() (numpy, the closed form the kernel uses) - on what the compiled reference made of the
same writes (tests/golden/wavepost_cases.npz, tools/make_wavepost_fixture.py).  The GPU part builds waves from
captures through the C ABI, and through the engine with the drop-in units."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from audiality2_amd import synth
from audiality2_amd.replay import WAVEPRE, WAVEPOST
from audiality2_amd.synth import LOOPED, NORMALIZE, XFADE, REVMIX
from conftest import GOLDEN, ROOT, make_gpu, make_oracle

N, X, L = NORMALIZE, XFADE, LOOPED
EUNSUPPORTED, EINVAL = -4, -2
SH_VALUES = [1, 2, 3, 5, 7, 63, 100, 333, 1000, 2047, 21600, 65537, 70400, 1000003]


def fixture_cases():
    z = np.load(os.path.join(GOLDEN, "wavepost_cases.npz"))
    out, p, e = [], 0, 0
    for name, (n, chunk, flags, wtype) in zip(z["names"], z["meta"]):
        n, chunk, flags = int(n), int(chunk), int(flags)
        m = WAVEPRE + n + WAVEPOST
        out.append((str(name), z["pcm"][p:p + n], chunk, flags, z["expect"][e:e + m]))
        p += n
        e += m
    assert p == len(z["pcm"]) and e == len(z["expect"])
    return out


def host_post(lib, pcm, chunk, flags):
    """a2amd_wavepost_host(): (return code, int16 level 0)"""
    lib.a2amd_wavepost_host.restype = ctypes.c_int
    lib.a2amd_wavepost_host.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
    pcm = np.ascontiguousarray(pcm, dtype=np.int32)
    out = np.full(max(1, len(pcm)), 0x5a5a, dtype=np.int16)
    rc = lib.a2amd_wavepost_host(pcm.ctypes.data, len(pcm), chunk, flags, out.ctypes.data)
    return rc, out[:len(pcm)]


def with_pads(level0, flags):
    return synth.wave_pyramid(level0, looped=bool(flags & L), levels=1)[1][0]


# ---- CPU: the arithmetic --------------------------------------------------------------------------------------
def test_fixture_holds_the_cases_it_is_meant_to():
    """(the fixture itself: every case of the list is there and is what its name says)"""
    cases = {c[0]: c for c in fixture_cases()}
    assert len(cases) == 16 and sum(len(c[1]) for c in cases.values()) < 16 * 3000
    assert os.path.getsize(os.path.join(GOLDEN, "wavepost_cases.npz")) < 65536
    for name, pcm, chunk, flags, want in cases.values():
        assert len(pcm) <= 3000 and (not len(pcm) or np.abs(pcm.astype(np.int64)).max() < 1 << 23), name

    def peak_chunk(name):
        pcm, chunk = cases[name][1], cases[name][2]
        return int(np.abs(pcm).argmax()) // chunk, (len(pcm) + chunk - 1) // chunk
    assert peak_chunk("normalize_peak_in_the_middle_chunk") == (1, 3)
    assert peak_chunk("normalize_peak_in_the_last_short_chunk") == (2, 3) and 600 % 256
    q = cases["normalize_quiet_with_a_silent_chunk"]
    assert not q[1][256:512].any() and np.abs(q[1]).max() < 8388352 / 2      # (a gain of 2 or more, but for the silent chunk)
    assert np.array_equal(q[4][WAVEPRE:-WAVEPOST], (q[1] >> 8).astype(np.int16))
    assert 0 < np.abs(cases["normalize_gain_capped_at_1000"][1]).max() < 8389
    neg = cases["normalize_negative_peak"][1]
    assert -int(neg.min()) > int(neg.max()) and (neg == neg.min()).sum() == 1
    assert not cases["normalize_all_silent"][1].any()
    assert [len(cases[k][1]) for k in ("xfade_even", "xfade_odd", "xfade_two_samples", "xfade_three_samples")] == [512, 733, 2, 3]
    assert cases["normalize_xfade_looped_mipwave"][3] == N | X | L
    assert {c[2] for c in cases.values()} >= {256, 100, 1}
    big = cases["normalize_chunk_larger_than_the_wave"]
    assert big[2] > len(big[1])


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0])
def test_host_arithmetic_equals_the_reference(gpu_lib, case):
    """a2amd_wavepost_host() and synth.wave_postprocess() on what the compiled reference made of the same writes:
    level 0, and with the pads of a2_fix_pad the whole of the reference's buffer."""
    name, pcm, chunk, flags, want = case
    rc, got = host_post(gpu_lib, pcm, chunk, flags)
    assert rc == 0
    assert np.array_equal(got, want[WAVEPRE:WAVEPRE + len(pcm)]), "a2amd_wavepost_host"
    assert np.array_equal(with_pads(got, flags), want)
    py = synth.wave_postprocess(pcm, chunk, flags)
    assert py.dtype == np.int16 and np.array_equal(py, got), "synth.wave_postprocess"


@pytest.mark.parametrize("sh", SH_VALUES)
def test_closed_form_window_gain_equals_serial_accumulation(gpu_lib, sh):
    """The reference adds the window's step up sample by sample in double and takes it off again from the middle on
    (waves.c:329-336); the kernel multiplies.  The step comes from a float (24 significant bits), so every partial
    sum is exact: the two are the same numbers - and the same waves, a2amd_wavepost_host() (serial) against
    synth.wave_postprocess() (closed form) on a wave of 2 sh + 1 samples."""
    dg = np.float64(np.float32(1.0) / np.float32(sh))
    size = 2 * sh + 1
    up = np.add.accumulate(np.concatenate([[0.0], np.full(sh, dg)]))            # g after 0 .. sh additions
    down = np.add.accumulate(np.concatenate([[up[sh]], np.full(size - sh - 1, -dg)]))
    serial = np.concatenate([up[:sh], down])
    i = np.arange(size, dtype=np.int64)
    closed = np.where(i < sh, i, 2 * sh - i).astype(np.float64) * dg
    assert serial.shape == closed.shape and np.array_equal(serial, closed)
    rng = np.random.default_rng(sh)
    pcm = rng.integers(-(1 << 23) + 1, 1 << 23, size=size, dtype=np.int32)
    rc, got = host_post(gpu_lib, pcm, 256, X)
    assert rc == 0 and np.array_equal(got, synth.wave_postprocess(pcm, 256, X))


def test_host_arithmetic_refusals(gpu_lib):
    pcm = np.arange(-5, 5, dtype=np.int32) << 16
    assert host_post(gpu_lib, pcm, 256, REVMIX)[0] == EUNSUPPORTED
    assert host_post(gpu_lib, pcm, 256, N | X | REVMIX)[0] == EUNSUPPORTED
    assert host_post(gpu_lib, pcm[:1], 256, X)[0] == EUNSUPPORTED
    assert host_post(gpu_lib, pcm[:0], 256, X)[0] == EUNSUPPORTED
    assert host_post(gpu_lib, pcm, 0, N)[0] == EUNSUPPORTED
    rc, out = host_post(gpu_lib, pcm, 0, N)
    assert rc == EUNSUPPORTED and (out == 0x5a5a).all()         # (nothing written on a refusal)
    rc, out = host_post(gpu_lib, pcm, 0, X)                     # (the chunk matters to normalize only)
    assert rc == 0 and np.array_equal(out, synth.wave_postprocess(pcm, 0, X))
    rc, out = host_post(gpu_lib, pcm, 0, 0)
    assert rc == 0 and np.array_equal(out, (pcm >> 8).astype(np.int16))
    gpu_lib.a2amd_wavepost_host.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
    assert gpu_lib.a2amd_wavepost_host(None, 4, 256, 0, out.ctypes.data) == EINVAL
    assert gpu_lib.a2amd_wavepost_host(pcm.ctypes.data, 4, 256, 0, None) == EINVAL
    for bad in ((REVMIX, 256), (X, 256), (N, 0)):
        with pytest.raises(ValueError):
            synth.wave_postprocess(pcm[:1] if bad[0] == X else pcm, bad[1], bad[0])


def test_wrapping_negation_keeps_int32_min_out_of_the_peak(gpu_lib):
    """-INT32_MIN wraps to itself and stays negative (waves.c:281): the sample never raises the peak, and what it
    becomes is what the reference's conversion (cvttss2si: 0x80000000 for what does not fit) makes of it."""
    pcm = np.array([1000000, -2147483648, -4000000, 3000000], dtype=np.int32)
    rc, got = host_post(gpu_lib, pcm, 256, N)
    g2 = (np.float32(8388352.0) / np.float32(4000000)) / np.float32(256.0)       # (peak 4000000, not 2^31)
    want = np.array([int(np.float32(v) * g2) for v in pcm], dtype=np.int64).astype(np.int16)
    assert abs(int(want[2])) in (32766, 32767) and want[0] > 8000
    assert rc == 0 and got.tolist() == want.tolist() == synth.wave_postprocess(pcm, 256, N).tolist()
    # ... and a gain above 1 takes it out of range
    pcm = np.array([10000, -2147483648, -20000, 15000], dtype=np.int32)
    rc, got = host_post(gpu_lib, pcm, 256, N)
    assert rc == 0 and got[1] == 0 and got.tolist() == synth.wave_postprocess(pcm, 256, N).tolist()


# ---- GPU: through the C ABI ---------------------------------------------------------------------------------------
def render_captured(length, mute_after=None):
    """`length` frames of 24 osc-filter-pan voices in a context with the capture on - fragments of 64 and a partial
    last one, several batches.  mute_after: every voice's amplitude and volume written to 0 at that frame (and the
    voices at a sixteenth of their level: 24 of them at the default reach beyond 24 bits, where a buffer's gain is
    below 1 whatever the silent one says).
    Returns (the closed backend, capture, the PCM of channel 0 as the host got it)."""
    sub = make_gpu(max_batch=8)
    sub.capture_begin()
    sc = synth.Scene(sub)
    sc.root()
    sc.add_voices(24, chain="osc-filter-pan", total=24 * 16 if mute_after is not None else None)
    pcm, done, pending = [], 0, 0
    while done < length:
        n = min(64, length - done, mute_after - done if mute_after and done < mute_after else 64)
        if mute_after is not None and done == mute_after:
            # (a walk like Scene.walk(), with the writes where the voices' programs would make them)
            sub.fragment(n)
            sub.unit_process(sc.rootv[0], 0, n)
            for units in sc.leaves:
                sub.unit_write(units[0], 2, 0)          # wtosc a
                sub.unit_write(units[2], 0, 0)          # panmix vol
                for u in units:
                    sub.unit_process(u, 0, n)
            sub.inline_end(sc.rootv[0])
            sub.unit_process(sc.rootv[1], 0, n)
            sub.unit_process(sc.rootv[2], 0, n)
        else:
            sc.walk(n)
        done += n
        pending += 1
        if pending == 7 or done == length:
            pcm.append(sub.render(pending * 64))
            pending = 0
    pcm = np.concatenate(pcm, axis=1)[0]
    cap = sub.capture_end()
    assert cap is not None and sub.capture_frames(cap) == length == len(pcm)
    sub.close()                                     # (the capture outlives its context)
    return sub, cap, pcm


def play(be, wid):
    """61 osc-pan voices over all mip levels on wave `wid`"""
    sc = synth.Scene(be)
    sc.private_ids = [wid]
    sc.root()
    sc.add_voices(61, chain="osc-pan", private=True)
    return sc.run(24, batch=8)


@pytest.mark.gpu
@pytest.mark.parametrize("length,flags,chunk,mute_after", [
    (733, N | X | L, 256, None), (3001, N, 256, None), (3001, X, 100, None), (4096, N | X | L, 256, None),
    (130, N | X | L, 64, None), (2, X, 256, None), (3, N | X, 1, None), (700, N, 256, 300),
    (900, N | X | L, 100, 900)])
def test_wave_built_from_a_capture_with_post_processing(oracle_lib, length, flags, chunk, mute_after):
    """A context renders `length` frames with the capture on; a second one builds a mip-mapped wave from the capture
    with a2amd_wave_upload_captured_post() - peaks, gain, conversion, crossfade, pads, mip levels, all on the
    device; a third context and the oracle get synth.wave_postprocess() + wave_pyramid() of the PCM uploaded.
    The same 61 voices over all mip levels sound identical on the three, and the built wave cost no H2D byte.
    (700, N, 256) with the voices muted from frame 300 on: the last chunk is silent, so the gain is exactly 1.
    (900, N | X | L, 100), one more than the list this test was specified with: the quiet scene never muted, so the
    gain is above 1 (the 24 voices at their default level are beyond 24 bits: those cases attenuate)."""
    sub, cap, pcm = render_captured(length, mute_after)
    level0 = synth.wave_postprocess(pcm, chunk, flags)
    if mute_after is not None and mute_after >= length:
        assert 256 < np.abs(pcm).max() < 8388352 // 2 and all(pcm[lo:lo + chunk].any() for lo in range(0, length, chunk))
        assert np.abs(synth.wave_postprocess(pcm, chunk, N).astype(np.int32)).max() >= 32766
    elif mute_after is not None:
        assert 256 < np.abs(pcm[:mute_after]).max() < 8388352 and not pcm[512:].any()
        assert np.array_equal(level0, (pcm >> 8).astype(np.int16))
    elif length >= 64:
        assert np.abs(pcm).max() > 256
        if flags & N:
            assert np.abs(level0.astype(np.int32)).max() > 8000 and not np.array_equal(level0, (pcm >> 8).astype(np.int16))
    sizes, data = synth.wave_pyramid(level0, looped=bool(flags & L), levels=synth.MIPLEVELS)
    outs = []
    for how in ("captured", "uploaded", "oracle"):
        be = make_oracle(oracle_lib) if how == "oracle" else make_gpu(max_batch=8)
        if how == "captured":
            synth.Scene(be)                         # (the built-in waves first: the new wave lands behind other data)
            before = be.wave_stats()
            wid = be.wave_upload_captured(0x7777, synth.WMIPWAVE, flags, 64, sizes, cap, chunk=chunk)
            after = be.wave_stats()
            assert after[0] == before[0] and after[1] == before[1] and after[2] == before[2] + 1, (before, after)
        else:
            wid = be.wave_upload(0x7777, synth.WMIPWAVE, flags, 64, sizes, data)
        outs.append(play(be, wid))
        be.close()
    sub.capture_free(cap)
    assert np.array_equal(outs[1], outs[2]), "uploaded wave: GPU vs oracle"
    assert np.array_equal(outs[0], outs[1]), "wave built from the capture vs the uploaded one"
    if length >= 64:
        assert outs[0].any()


@pytest.mark.gpu
def test_post_entry_point_without_flags_and_refusals(oracle_lib):
    """a2amd_wave_upload_captured_post() with neither flag is a2amd_wave_upload_captured(); A2_REVMIX, A2_XFADE on one
    sample and A2_NORMALIZE without a chunk are refused with A2AMD_EUNSUPPORTED and change nothing - the same key
    uploads the ordinary way afterwards; the old entry point still refuses A2_NORMALIZE."""
    _, cap, pcm = render_captured(130)
    _, cap1, pcm1 = render_captured(1)
    be = make_gpu(max_batch=8)
    synth.Scene(be)
    sizes = [(130 + (1 << lv) - 1) >> lv for lv in range(synth.MIPLEVELS)]
    sizes1 = [1] * synth.MIPLEVELS
    start = be.wave_stats()
    for fl, c, sz, chunk in ((REVMIX, cap, sizes, 256), (N | X | REVMIX, cap, sizes, 256), (X, cap1, sizes1, 256),
                             (N, cap, sizes, 0), (N | X, cap, [129] + sizes[1:], 256)):
        assert be.wave_upload_captured(0x7777, synth.WMIPWAVE, fl, 64, sz, c, chunk=chunk, check=False) == EUNSUPPORTED
    for fl in (N, X, N | X, REVMIX):
        assert be.wave_upload_captured(0x7777, synth.WMIPWAVE, fl, 64, sizes, cap, chunk=None, check=False) == EUNSUPPORTED
    assert be.wave_stats() == start
    # the same key the ordinary way ...
    _, data = synth.wave_pyramid((pcm >> 8).astype(np.int16), looped=True, levels=synth.MIPLEVELS)
    wid = be.wave_upload(0x7777, synth.WMIPWAVE, L, 64, sizes, data)
    st = be.wave_stats()
    assert wid >= 0 and st[1] == start[1] + 1 and st[2] == start[2]
    outs = [play(be, wid)]
    be.close()
    # ... and built from the capture by either entry point: the same wave
    for chunk in (None, 0):
        be = make_gpu(max_batch=8)
        synth.Scene(be)
        outs.append(play(be, be.wave_upload_captured(0x7777, synth.WMIPWAVE, L, 64, sizes, cap, chunk=chunk)))
        assert be.wave_stats()[2] == 1
        be.close()
    be.capture_free(cap)
    be.capture_free(cap1)
    assert outs[0].any() and np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


# ---- GPU: the engine in the loop ------------------------------------------------------------------------------------
REF_RENDER = os.path.join(ROOT, "oracle", "_ref", "ref_render")
UNITS_SO = os.path.join(ROOT, "audiality2_amd", "liba2amd_units.so")
A2S = os.path.join(ROOT, "tests", "a2s")


@pytest.mark.gpu
def test_post_processed_rendered_waves_stay_on_the_device(tmp_path):
    """wavepost.a2s renders five waves at load time (a2_RenderWave from the compiler): looped + normalize + xfade and
    mip-mapped; normalize with a silent stretch; xfade of odd length; looped + normalize + xfade rendered by voices
    that play the first; a plain one.  The reference alone, the drop-in, and the drop-in with the waves uploaded
    from the engine's copies (A2AMD_NO_RESIDENT=1) render the same audio, and in the resident run all five device
    copies are built from what the device rendered."""
    if not (os.path.exists(REF_RENDER) and os.path.exists(UNITS_SO)):
        pytest.skip("oracle/_ref (compiled reference) or liba2amd_units.so not built")
    frames = 2 * 48000
    outs, stats = {}, {}
    for tag, extra in (("reference", None), ("resident", {}), ("uploaded", {"A2AMD_NO_RESIDENT": "1"})):
        out = tmp_path / f"{tag}.pcm"
        env = dict(os.environ, A2REF_REALTIME="1")
        if extra is not None:
            env.update(LD_PRELOAD=UNITS_SO, A2AMD_WAVE_STATS="1", **extra)
        r = subprocess.run([REF_RENDER, f"{A2S}/wavepost.a2s", "Main", str(frames), "64", "48000", "2", str(out), "0.2"],
                           env=env, cwd=A2S, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-800:]
        outs[tag] = np.fromfile(out, dtype="<i4")
        if extra is None:
            continue
        lines = [ln for ln in r.stderr.splitlines() if "waves copied from the host" in ln]
        main = [ln for ln in lines if "state 0:" in ln]
        assert len(main) == 1 and len(lines) == 6, r.stderr[-1200:]        # five substates, one master state
        w = main[0].split()
        stats[tag] = (int(w[w.index("waves") - 1]), int(w[w.index("built") - 1]))
    assert len(outs["reference"]) == 2 * frames and outs["reference"].any()
    assert np.array_equal(outs["reference"], outs["resident"]), "drop-in, waves built on the device"
    assert np.array_equal(outs["reference"], outs["uploaded"]), "drop-in, waves uploaded from the engine's copies"
    assert stats["resident"][1] == 5 and stats["uploaded"][1] == 0, stats
    assert stats["uploaded"][0] == stats["resident"][0] + 5, stats
