"""csrc/a2amd_quiet.h on a host compiler: how a filter kernel's workgroup deals its voices to its wavefronts.

The header is the one statement of the skeleton the quiet leaf kernels share (k_leaf_noisepan, k_leaf_noisefiltpan,
k_leaf_oscbare, k_leaf_osc3filtpan).  Its only integer logic that is not a line of the reference - which voices of the
workgroup wavefront wv renders - is written for a host compiler too: tests/quiet_probe.cpp prints it for the inputs below
and it is compared with the same rule restated in numpy.  No library, no device; the GPU tests of the four kernels
(test_noise_quiet.py, test_noise_filt_quiet.py, test_osc_bare.py, test_osc3_filt.py) pin the callers bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_switches import CSRC, TESTS, _code, lib_sources

HEADER = os.path.join(CSRC, "a2amd_quiet.h")
QUIET = ("a2amd_noisepan.hip", "a2amd_noisefiltpan.hip", "a2amd_oscbare.hip", "a2amd_osc3filtpan.hip")
WAVES, FILTER, IDLE = 8, 0, 4
PAIR = r"atomicAdd\s*\(\s*&\s*\w+\s*\[\s*A2D_FRAG\s*\+\s*lane\s*\]"      # the second channel's add of a stereo pair
WORKERS = (1, 2, 3, 5, 6, 7)            # in worker order


def ranges(nv):
    """[(first, end)] of the six workers: the list cut in order, the first nv % 6 ranges one voice longer"""
    per, extra = divmod(nv, len(WORKERS))
    size = np.array([per + (k < extra) for k in range(len(WORKERS))])
    end = np.cumsum(size)
    return list(zip((end - size).tolist(), end.tolist()))


def bits(first, end):
    return ((1 << end) - 1) & ~((1 << first) - 1)


def inputs():
    """(nv, todo): every workgroup size; all its voices, each one alone, every other one, all but one worker's"""
    rows = []
    for nv in range(1, 65):
        full = bits(0, nv)
        rows.append((nv, full))
        rows += [(nv, 1 << v) for v in range(nv)]
        rows += [(nv, full & 0x5555555555555555), (nv, full & 0xaaaaaaaaaaaaaaaa)]
        rows += [(nv, full & ~bits(a, b)) for a, b in ranges(nv) if b > a]
    return rows


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("quiet") / "quiet_probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, os.path.join(TESTS, "quiet_probe.cpp")],
                   check=True)
    rows = inputs()
    text = "".join("%d %x\n" % r for r in rows)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(rows)
    got = []
    for ln in out:
        w = ln.split()
        assert (int(w[-2]), int(w[-1])) == (WAVES, len(WORKERS)) and len(w) == WAVES + 2
        got.append([int(x, 16) for x in w[:WAVES]])
    return rows, got


def test_the_inputs_are_what_they_are_named_for():
    rows = inputs()
    assert {nv for nv, _ in rows} == set(range(1, 65))
    for nv in (1, 5, 6, 7, 63, 64):
        mine = [t for n, t in rows if n == nv]
        assert bits(0, nv) in mine and all(1 << v in mine for v in range(nv))
        assert all(0 < t <= bits(0, nv) for t in mine if nv > 1)
    # (below six voices some workers have no range to leave empty; from six on every worker has one)
    assert sum(1 for n, _ in rows if n == 64) == 1 + 64 + 2 + 6 and sum(1 for n, _ in rows if n == 3) == 1 + 3 + 2 + 3


def test_worker_split(split):
    rows, got = split
    for (nv, todo), masks in zip(rows, got):
        # the filter wavefront renders none, and neither does wavefront 4: it shares the filter's SIMD
        assert masks[FILTER] == 0 and masks[IDLE] == 0, (nv, hex(todo))
        mine = [masks[w] for w in WORKERS]
        # pairwise disjoint, and together exactly the voices to render
        union = 0
        for m in mine:
            assert not union & m, (nv, hex(todo))
            union |= m
        assert union == todo, (nv, hex(todo), hex(union))
        # the rule itself: worker k's share of its range of the list
        assert mine == [todo & bits(a, b) for a, b in ranges(nv)], (nv, hex(todo))


def test_ranges_ascend_in_worker_order_and_are_even(split):
    """With every voice to render a mask IS the worker's range: contiguous, behind the range of the worker before it (the
    bus-run walk relies on list order), the sizes within one of each other."""
    rows, got = split
    seen = set()
    for (nv, todo), masks in zip(rows, got):
        if todo != bits(0, nv):
            continue
        seen.add(nv)
        mine = [masks[w] for w in WORKERS]
        sizes = [bin(m).count("1") for m in mine]
        assert sum(sizes) == nv and max(sizes) - min(sizes) <= 1, (nv, sizes)
        nxt = 0
        for m, n in zip(mine, sizes):
            if m:
                first = (m & -m).bit_length() - 1
                assert first == nxt and m == bits(first, first + n), (nv, hex(m))
                nxt = first + n
        assert nxt == nv
    assert seen == set(range(1, 65))


def test_the_header_is_the_only_statement():
    paths = lib_sources()
    assert HEADER in paths and len(paths) > 30
    names = {os.path.basename(p) for p in paths}
    assert set(QUIET) <= names
    # the tap pair has one name
    assert not [os.path.basename(p) for p in paths if re.search(r"\b(BareTaps|O3Taps)\b", open(p, errors="replace").read())]
    assert {os.path.basename(p) for p in paths if re.search(r"\bstruct\s+OscTaps\b", _code(p))} == {"a2amd_quiet.h"}
    # the worker split's arithmetic stands in the header alone
    assert {os.path.basename(p) for p in paths if re.search(r"%\s*\w*_WORKERS\b", _code(p))} == {"a2amd_quiet.h"}
    assert {os.path.basename(p) for p in paths if re.search(r"#\s*define\s+\w+_WORKERS\b", _code(p))} == {"a2amd_quiet.h"}
    # ... and so does the stereo pair of atomic adds.  Of the four kernels only k_leaf_oscbare adds to a bus itself: its
    # mono run into channel 0, written out (no pair, no second channel)
    for name in QUIET:
        code = _code(os.path.join(CSRC, name))
        assert '#include "a2amd_quiet.h"' in code
        assert not re.search(PAIR, code), name
        assert code.count("atomicAdd") == (2 if name == "a2amd_oscbare.hip" else 0), name
    assert len(re.findall(PAIR, _code(HEADER))) == 1
    # the quiet kernels name no filt_row instantiation: a2amd_filt.h picks it (a2amd_fast.hip's kernels choose for themselves)
    assert {os.path.basename(p) for p in paths if re.search(r"\bfilt_row\s*<", _code(p))} == {"a2amd_filt.h", "a2amd_fast.hip"}
    # the launch shape of the filter kernels - grid, block, the three tiles of dynamic LDS - stands in the header alone
    assert {os.path.basename(p) for p in paths if re.search(r"3\s*\*\s*vpg\s*\*\s*QUIET_PITCH", _code(p))} == {"a2amd_quiet.h"}
    assert {os.path.basename(p) for p in paths if re.search(r"QUIET_MAXV\s*\?", _code(p))} == {"a2amd_quiet.h"}
    # the three-oscillator class: both kernels' rule of which voice is theirs - the mode test of the three oscillators -
    # stands in one function, and so does the panmix head's clamp flag
    o3 = _code(os.path.join(CSRC, "a2amd_osc3filtpan.hip"))
    assert o3.count("__global__") == 2
    modes = [m.start() for m in re.finditer(r"==\s*A2D_OSC_MIPWAVE\b", o3)]
    assert len(modes) == 3 and o3.count("OW_MODE") == 3
    body = o3[o3.rindex("\n{\n", 0, modes[0]):modes[-1]]        # from the function's opening brace to its last mode test
    assert body.count("OW_MODE") == 3 and "\n}\n" not in body
    assert len(re.findall(r"a2s_pan_over\s*\(\s*pan\.target\s*\)", o3)) == 1 and o3.count("a2s_pan_over") == 2
