"""Which wavefronts k_leaf_osc2tame takes (include/a2amd_osc2tame_kernel.h; csrc/a2amd_device.h: a2d_osc2tame_voice,
a2d_osc2tame_wave) and when the host launches it (a2d_osc2_all_whole, a2d_osc2_shape): the rule on a host compiler, no
device.

tests/osc2tame_probe.cpp is a program of its own, made to be run under AddressSanitizer and UBSan by the command line in
its header; here it is built without them.  It feeds the rule from state words through the settled tests the kernel
applies (csrc/a2amd_settled.h): level sizes that are and are not powers of two, each tame bit, a record run, each settled
condition, a phase at the limit of the general kernel's mask branch, wavefronts of 1 to 64 voices with each voice
missing in turn, batches with and without a cut fragment."""
import os
import subprocess

from test_switches import CSRC, TESTS


def test_probe_program(tmp_path):
    exe = str(tmp_path / "osc2tame_probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, os.path.join(TESTS, "osc2tame_probe.cpp")],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 2000


def test_the_constant_keeps_small_scenes_on_the_general_kernel():
    """A2D_OSC2TAME_MIN stays above the scenes whose launches tests/test_gpu_launch_plan.py pins (24 such voices)"""
    with open(os.path.join(CSRC, "a2amd_device.h")) as f:
        line = [ln for ln in f if ln.startswith("#define A2D_OSC2TAME_MIN")]
    assert len(line) == 1 and int(line[0].split()[2]) > 24, line
