"""Which mip levels k_leaf_osc2pan's voice-major walk may read from LDS (include/a2amd_osc2lds.h): the host's half, no device.

The rule - a2d_osc2_stage(), csrc/a2amd_device.h, the kernel's own - through the C ABI, the pad check that sets a
level's "periodic" bit at a2amd_wave_upload() through the C ABI on the levels synth.wave_pyramid() makes, and the same
two functions in a program of their own (tests/wavepads_probe.cpp: exact-size heap blocks, sizes 1, 2, 63, 64 and 2048,
pads wrong at the first and at the last position - made to be run under AddressSanitizer and UBSan, by the command
line in its header; here it is built without them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from audiality2_amd import synth
from audiality2_amd.replay import WAVEPOST, WAVEPRE
from test_switches import CSRC, TESTS

LDS_ENT = 128       # A2D_OSC2_LDS_ENT

# (size0, periodic0, size1, periodic1) -> mask; the first eight are the pairs tests/test_gpu_osc2_lds_taps.py renders
RULE = [
    ((64, 1, 64, 1), 3), ((128, 1, 128, 1), 1), ((128, 1, 64, 1), 1), ((256, 1, 64, 1), 2), ((64, 1, 256, 1), 1),
    ((32, 1, 32, 1), 3), ((96, 1, 64, 1), 2), ((256, 1, 256, 1), 0),
    ((64, 0, 64, 1), 2), ((64, 1, 64, 0), 1), ((64, 0, 64, 0), 0), ((128, 0, 128, 1), 2), ((64, 1, 96, 1), 1),
    ((1, 1, 1, 1), 3), ((0, 1, 64, 1), 2), ((64, 1, 0, 1), 1), ((2048, 1, 1024, 1), 0), ((64, 1, 32, 1), 3),
    ((127, 1, 129, 1), 0), ((1 << 31, 1, 128, 1), 2),
]


@pytest.fixture(scope="module")
def abi(gpu_lib):
    rule = gpu_lib.a2amd_osc2_stage_rule
    rule.restype, rule.argtypes = C.c_uint, [C.c_uint, C.c_int, C.c_uint, C.c_int]
    periodic = gpu_lib.a2amd_wave_level_periodic
    periodic.restype, periodic.argtypes = C.c_int, [C.POINTER(C.c_int16), C.c_uint]

    def level_periodic(buf):
        buf = np.ascontiguousarray(buf, dtype=np.int16)
        return periodic(buf.ctypes.data_as(C.POINTER(C.c_int16)), len(buf) - WAVEPRE - WAVEPOST)
    return rule, level_periodic


def _rule(s0, p0, s1, p1):
    """the rule restated"""
    def cand(s, p):
        return bool(p) and s > 0 and s & (s - 1) == 0 and s <= LDS_ENT
    c0, c1 = cand(s0, p0), cand(s1, p1)
    return (1 if c0 else 0) | (2 if c1 and (s0 if c0 else 0) + s1 <= LDS_ENT else 0)


def test_rule_table(abi):
    rule, _ = abi
    for args, want in RULE:
        assert rule(*args) == want == _rule(*args), args
    assert {want for _, want in RULE} == {0, 1, 2, 3}
    # any non-zero periodic argument is "yes"
    assert rule(64, 7, 64, -1) == 3
    for s0 in list(range(0, 140)) + [255, 256, 257]:
        for s1 in list(range(0, 140)) + [255, 256, 257]:
            for p in range(4):
                assert rule(s0, p & 1, s1, p >> 1) == _rule(s0, p & 1, s1, p >> 1), (s0, s1, p)


def test_pad_check_on_uploaded_levels(abi):
    _, periodic = abi
    rng = np.random.default_rng(5)
    for length in (1, 2, 63, 64, 96, 2048):
        sizes, data = synth.wave_pyramid(rng.integers(-32768, 32768, size=length).astype(np.int16))
        for size, buf in zip(sizes, data):
            assert periodic(buf) == 1, (length, size)       # every level of a looped wave, not only level 0
            for at in (0, WAVEPRE + size, WAVEPRE + size + WAVEPOST - 1):
                bad = buf.copy()
                bad[at] ^= 1
                assert periodic(bad) == 0, (length, size, at)
        # an unlooped wave's pads are silence
        sizes, data = synth.wave_pyramid(rng.integers(1, 32768, size=length).astype(np.int16), looped=False)
        assert periodic(data[0]) == 0


def test_probe_program(tmp_path):
    """tests/wavepads_probe.cpp, built plainly here; its header gives the command line that runs it under the sanitizers
    (a program of its own: nothing of it is loaded into this process)"""
    exe = str(tmp_path / "wavepads_probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, os.path.join(TESTS, "wavepads_probe.cpp")],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 50
