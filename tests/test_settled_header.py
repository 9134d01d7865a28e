"""csrc/a2amd_settled.h against the reference's own lines, on a host compiler: no library, no device.

The header is the one statement of what a leaf kernel works out from a voice's state words before it may take a settled
path - the mip level and increment (wtosc.c:250-258), the two panmix gains (panmix.c:84-104), the two "this ramper will
not move" tests (a2_dsp.h:128-149) - and every kernel, the window control pass and the host's phase shadow call it.
tests/settled_probe.cpp prints its results for the inputs below; they are compared with those lines restated in numpy.
The GPU tests (test_gpu_gain_range.py, test_gpu_tap_edges.py, test_osc_bare.py, the noise tests) pin the callers."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from audiality2_amd import synth
from gain_cases import GAINS
from test_switches import CSRC, TESTS, _code, lib_sources

MAXPHINC, MIPS, LOOPED = 512, 10, 0x100          # A2_MAXPHINC (a2_waves.h:57), A2_MIPLEVELS, A2_LOOPED
HEADER = os.path.join(CSRC, "a2amd_settled.h")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("settled") / "settled_probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, os.path.join(TESTS, "settled_probe.cpp")],
                   check=True)

    def run(op, rows):
        text = "".join("%s %d %d %d %d\n" % ((op,) + tuple(int(x) for x in r)) for r in rows)
        out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout
        got = np.array([[int(x) for x in ln.split()] for ln in out.splitlines()], dtype=np.int64)
        assert got.shape == (len(rows), 4 if op == "r" else 3)
        return got
    return run


def i32(x):
    """the low 32 bits as a signed word: what the reference's int arithmetic leaves on the machines it runs on"""
    return (np.asarray(x, dtype=np.int64) & 0xffffffff).astype(np.uint32).astype(np.int32).astype(np.int64)


def ref_gains(vol, pan, clamp):
    """panmix.c:91-101"""
    vp = i32((pan * vol) >> 24)
    v0, v1, lim = i32(vol - vp), i32(vol + vp), i32(vol << 1)
    return np.where(clamp & (v0 > lim), lim, v0), np.where(clamp & (v1 > lim), lim, v1)


def test_pan_gains(probe):
    words = [(i32(vol << 8), i32(pan << 8)) for _, vol, pan in GAINS]
    words += [(i32(vol << 8), pan) for _, vol, _ in GAINS[:4]
              for pan in (0xffff00, -0xffff00, 0xffffff, -0xffffff, 0x1000000, -0x1000000, 0x1000100, -0x1000100)]
    rows = [(int(v), int(p), c, 0) for v, p in words for c in (0, 1)]
    got = probe("g", rows)
    vol, pan, clamp = (np.array([r[k] for r in rows], dtype=np.int64) for k in range(3))
    v0, v1 = ref_gains(vol, pan, clamp != 0)
    assert np.array_equal(got[:, 0], v0) and np.array_equal(got[:, 1], v1)
    # panmix.c:120-124: the clamped variant beyond +-0xffffff
    assert np.array_equal(got[:, 2], ((pan > 0xffffff) | (pan < -0xffffff)).astype(np.int64))
    assert got[:, 2].any() and not got[:, 2].all()
    assert (ref_gains(vol, pan, np.ones(len(rows), bool))[0] != ref_gains(vol, pan, np.zeros(len(rows), bool))[0]).any()


def ref_mip(dphase, period):
    """wtosc.c:251-258, in the reference's unsigned arithmetic"""
    dph = ((((dphase + 255) & 0xffffffff) >> 8) * period) & 0xffffffff
    mm = np.zeros_like(dph)
    for _ in range(MIPS - 1):
        step = (dph > (MAXPHINC << 8)) & (mm < MIPS - 1)
        mm = mm + step
        dph = np.where(step, dph >> 1, dph)
    return mm, ((dphase * period) >> mm) & 0xffffffff


def mip_inputs(period):
    """dphase on both sides of every level's threshold, of the last level's range, and the ends of the word"""
    out = [0, 1, 0xffffffff]
    for k in range(MIPS - 1):
        q = -(-(((MAXPHINC << 8) + 1) << k) // period)         # the smallest (dphase + 255) >> 8 that leaves level k
        out += [(q - 1) << 8, ((q - 1) << 8) + 1]
    top = -(-(((MAXPHINC << 16) + 1) << (MIPS - 1)) // period)   # the smallest dphase out of range at the last level
    out += [top - 1, top]
    return [d for d in out if 0 <= d <= 0xffffffff]


def test_mip_step(probe):
    rows = []
    for period in (1, 3001, synth.WAVEPERIOD):
        ins = mip_inputs(period)
        rows += [(d, period, 1000, LOOPED) for d in ins]
        rows += [(ins[-1], period, size0, flags) for size0, flags in ((0, LOOPED), (1000, 0), (1000, 0xff), (1, 0x1ff))]
    got = probe("m", rows)
    dphase, period, size0, flags = (np.array([r[k] for r in rows], dtype=np.int64) for k in range(4))
    mm, dph = ref_mip(dphase, period)
    assert np.array_equal(got[:, 0], mm) and np.array_equal(got[:, 1], dph)
    # wtosc.c:168-183 (unloaded), :260 (looped), :271 (out of range)
    ok = (size0 != 0) & ((flags & LOOPED) != 0) & (dph <= (MAXPHINC << 16))
    assert np.array_equal(got[:, 2], ok.astype(np.int64))
    # the inputs do straddle what they are named for: each pair sits on two levels, the last pair on the two sides of
    # the range test at the last level
    at = {(int(d), int(p)): (int(m), bool(o)) for d, p, s0, fl, m, o in zip(dphase, period, size0, flags, mm, ok)
          if s0 == 1000 and fl == LOOPED}
    for p in (1, 3001, synth.WAVEPERIOD):
        ins = mip_inputs(p)
        pairs = list(zip(ins[3::2], ins[4::2]))
        if p > 1:       # (period 1: the 32-bit word ends below level 7's threshold)
            assert len(pairs) == MIPS and at[pairs[-1][0], p] == (MIPS - 1, True) and at[pairs[-1][1], p] == (MIPS - 1, False)
            pairs = pairs[:-1]
        assert [(at[a, p][0], at[b, p][0]) for a, b in pairs] == [(k, k + 1) for k in range(len(pairs))]
        assert len(pairs) == (MIPS - 1 if p > 1 else 7)


def prepare(r, frames):
    """a2_PrepareRamper, a2_dsp.h:128-149, on (value, target, delta, timer)"""
    value, target, delta, timer = r
    if not timer:
        return target, target, 0, 0
    if frames <= (timer >> 8):
        return value, target, int((target - value) * 256 / timer), timer - (frames << 8)
    return value, target, int((target - value) / frames), 0


def test_ramper_predicates(probe):
    rows = [(5 if same else 6, 5, delta, timer) for timer, delta, same in itertools.product((0, 255, 256), (0, 1), (True, False))]
    got = probe("r", rows)
    for (value, target, delta, timer), (arrived, arrived_b, at_rest, settled) in zip(rows, got):
        # the wavetable kernels': nothing pending at all (asked of two rampers at once: either place)
        assert arrived == arrived_b == (delta == 0 and timer == 0 and value == target)
        # the noise kernels': the timer at 0, or below one frame with the value there
        assert at_rest == (timer == 0 or (timer < 256 and value == target))
        assert settled == arrived               # (a2s_osc_settled is built from "arrived")
        for frames in (1, 63, 64):
            after = prepare((value, target, delta, timer), frames)
            if arrived:     # a2_PrepareRamper changes nothing, the VALUE word included
                assert after == (value, target, delta, timer)
            if at_rest:     # ... leaves the ramper at its TARGET whatever the window's length
                assert after == (target, target, 0, 0)
    # the two differ exactly here: a ramper that will only snap, a write without a duration that has met no window
    differ = sorted(r[1:] + (r[0] == r[1],) for r, g in zip(rows, got) if g[0] != g[2])
    assert differ == sorted([(5, 0, 0, False), (5, 1, 0, True), (5, 1, 0, False), (5, 0, 255, True), (5, 1, 255, True)])


def test_the_header_is_the_only_statement():
    paths = lib_sources()
    assert HEADER in paths and len(paths) > 30
    mip = {os.path.basename(p) for p in paths if "A2D_MAXPHINC << 8" in _code(p)}
    # (the two per-window paths that step the amplitude ramper between the first product and the level loop keep the
    # lines written out, each marked "restates a2s_mip()": profiles/settled_header_codeobj.txt)
    assert mip == {"a2amd_settled.h", "a2amd_kernels.hip", "a2amd_winctl.h"}
    for name in ("a2amd_kernels.hip", "a2amd_winctl.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert text.count("A2D_MAXPHINC << 8") == 1 and "restates a2s_mip()" in text
    pan = {os.path.basename(p) for p in paths if re.search(r"[<>]=?\s*-?\s*0xffffff\b", _code(p))}
    assert pan == {"a2amd_settled.h"}
