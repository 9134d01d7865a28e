"""Which mip levels are "tame" - no product of a2_Hermite wraps in them - for k_leaf_osc2pan's fused multiply-add steps
(include/a2amd_osc2tame.h; csrc/a2amd_wavetame.h): the host's half, no device.

a2amd_wave_level_tame() through the C ABI against a plain numpy restatement of the three Horner steps as the reference
evaluates them (a2_dsp.h:64-74: x = frac << 7, 32 bit products, >> 15), over every window inside the level and all 256
fractions: the engine's 24 built-in waves (tests/golden/builtin_waves.npz) and synth.test_waves(24), every level tame; a
full-scale white-noise cycle, not tame; and the windows at the edge of the 24 bit product - a = 65 793 (product
2^24 - 1 at frac 255: tame), a = 65 794 (wraps at frac 255 only: not), and their mirror images - each placed in the
payload, in the post-pad beyond the payload (a level whose pads are not periodic) and in the pre-pad window.  The same
function in a program of its own (tests/wavetame_probe.cpp, made to be run under AddressSanitizer and UBSan by the
command line in its header; here it is built without them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from audiality2_amd import synth
from audiality2_amd.replay import WAVEPOST, WAVEPRE
from test_switches import CSRC, TESTS

GOLDEN = os.path.join(TESTS, "golden")
LIM = 1 << 24


@pytest.fixture(scope="module")
def abi(gpu_lib):
    tame = gpu_lib.a2amd_wave_level_tame
    tame.restype, tame.argtypes = C.c_int, [C.POINTER(C.c_int16), C.c_uint]
    rule = gpu_lib.a2amd_osc2_tame_rule
    rule.restype, rule.argtypes = C.c_uint, [C.c_int, C.c_int]

    def level_tame(buf):
        buf = np.ascontiguousarray(buf, dtype=np.int16)
        return tame(buf.ctypes.data_as(C.POINTER(C.c_int16)), len(buf) - WAVEPRE - WAVEPOST)
    return level_tame, rule, tame


def _tame(buf):
    """the rule restated: every window d[i-1 .. i+2] wholly inside the level's buffer, i counted from the first payload
    sample (i in [0, size + post - 3]), every fraction, the three products of a2_Hermite in turn"""
    p = np.asarray(buf, dtype=np.int64)
    size = len(p) - WAVEPRE - WAVEPOST
    n = size + WAVEPOST - 2
    if size <= 0 or n <= 0:
        return 0
    i = np.arange(n) + WAVEPRE
    dm, d0, d1, d2 = p[i - 1], p[i], p[i + 1], p[i + 2]
    c = (d1 - dm) >> 1
    a = (3 * (d0 - d1) + d2 - dm) >> 1
    b = dm - d0 + c - a
    f = np.arange(256, dtype=np.int64)[:, None]
    ok = np.ones((256, n), dtype=bool)
    v = np.broadcast_to(a, (256, n))
    for add in (b, c, None):
        prod = v * f
        ok &= (prod >= -LIM) & (prod < LIM)
        if add is not None:
            v = (prod >> 8) + add       # (what the reference's (v * x) >> 15 gives where the product did not wrap)
    return int(ok.all())


def _levels(flat, sizes):
    out, pos = [], 0
    for s in sizes:
        n = WAVEPRE + int(s) + WAVEPOST
        out.append(flat[pos:pos + n])
        pos += n
    assert pos == len(flat)
    return out


def test_builtin_waves_are_tame(abi):
    level_tame = abi[0]
    z = np.load(os.path.join(GOLDEN, "builtin_waves.npz"))
    n = 0
    for k in range(24):
        hdr, flat = z[f"w{k}_hdr"], z[f"w{k}_data"]
        for lv, buf in enumerate(_levels(flat, hdr[3:])):
            assert level_tame(buf) == _tame(buf) == 1, (k, lv)
            n += 1
    assert n == 240


def test_bench_waves_are_tame(abi):
    level_tame = abi[0]
    n = 0
    for k, cycle in enumerate(synth.test_waves(24)):
        sizes, data = synth.wave_pyramid(cycle)
        for lv, buf in enumerate(data):
            assert level_tame(buf) == _tame(buf) == 1, (k, lv)
            n += 1
    assert n == 240


def test_white_noise_is_not_tame(abi):
    level_tame = abi[0]
    rng = np.random.default_rng(18)
    sizes, data = synth.wave_pyramid(rng.integers(-32768, 32768, size=2048).astype(np.int16))
    assert level_tame(data[0]) == _tame(data[0]) == 0
    for buf in data[1:]:            # (the averaged levels are what they are: the rule and the restatement agree)
        assert level_tame(buf) == _tame(buf)


# (dm, d0, d1, d2), a, tame
EDGE = [
    ((32251, 32767, -32768, -32768), 65793, 1),
    ((32249, 32767, -32768, -32768), 65794, 0),
    ((-32252, -32768, 32767, 32767), -65793, 1),
    ((-32250, -32768, 32767, 32767), -65794, 0),
]
SIZE = 64


@pytest.mark.parametrize("window,a,tame", EDGE)
@pytest.mark.parametrize("where", ["payload", "postpad", "prepad"])
def test_edge_windows(abi, window, a, tame, where):
    level_tame = abi[0]
    dm, d0, d1, d2 = window
    assert (3 * (d0 - d1) + d2 - dm) >> 1 == a
    assert (abs(a) * 255 < LIM) == bool(tame)       # (only frac 255 can tell 65 793 from 65 794)
    buf = np.zeros(WAVEPRE + SIZE + WAVEPOST, dtype=np.int16)
    i = {"payload": 20, "postpad": SIZE + 100, "prepad": 0}[where]      # the window's second sample, payload index
    buf[WAVEPRE + i - 1:WAVEPRE + i + 3] = window
    quiet = np.zeros_like(buf)
    assert level_tame(quiet) == _tame(quiet) == 1
    assert level_tame(buf) == _tame(buf) == tame, (where, window)


def test_degenerate_levels(abi):
    _, _, raw = abi
    one = np.zeros(WAVEPRE + 1 + WAVEPOST, dtype=np.int16)
    assert raw(one.ctypes.data_as(C.POINTER(C.c_int16)), 1) == 1
    assert raw(one.ctypes.data_as(C.POINTER(C.c_int16)), 0) == 0        # an empty level
    assert raw(None, 64) == 0                                           # no data


def test_voice_rule(abi):
    rule = abi[1]
    assert [rule(0, 0), rule(1, 0), rule(0, 1), rule(1, 1)] == [0, 0, 0, 1]
    assert rule(7, -1) == 1         # any non-zero argument is "yes"


def test_probe_program(tmp_path):
    """tests/wavetame_probe.cpp, built plainly here; its header gives the command line that runs it under the sanitizers
    (a program of its own: nothing of it is loaded into this process)"""
    exe = str(tmp_path / "wavetame_probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, os.path.join(TESTS, "wavetame_probe.cpp")],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 30
