"""The host copy of the device VM's interpreter (csrc/a2amd_vmcore.h through a2amd_vm_trace_host_env) against a plain
restatement of the reference's VM arithmetic (tests/vm_model.py), over the programs the direct GPU tests hand to the device
(tests/vm_programs.py): edge operands for everything a2amd_vmcore.h leaves to the compiler - 64 bit products and
quotients, truncating / and %, >> of negative values, the tracker's 32 bit mask.  No GPU: an altered expression of any
one opcode in a2amd_vmcore.h fails here; the same source compiled for the device is what test_gpu_vm_direct.py runs."""
import ctypes

import pytest

import audiality2_amd
from audiality2_amd import synth
from conftest import make_oracle
from test_device_vm import MSDUR, R_F1RAMP, R_F1SET, R_SEG, R_WRITE, VmState

import vm_model
import vm_programs as vp

BASEPITCH = synth.basepitch_for(48000)
_ptab = []


def pitch_table(oracle_lib):
    """the pitch table a context reports (a2_pitch_open's, pitch.c:70-96): 64 x {base, coeff}"""
    if not _ptab:
        ora = make_oracle(oracle_lib)
        _ptab.extend(int(x) for x in ora.get_pitch_table())
        ora.close()
    return _ptab


def to_ctypes(st):
    c = VmState()
    c.waketime, c.state, c.pc = st.waketime, st.state, st.pc
    for k, v in enumerate(st.r):
        c.r[k] = v
    return c


def from_ctypes(c):
    return vm_model.State(c.waketime, c.pc, list(c.r), c.state)


def host_trace(words, n, st, chain, layout, base, now, cap=1 << 18):
    """a2amd_vm_trace_host_env over the fragments layout[] (each base[] frames inside the engine's own): (the records as
    (fragment, op, unit, register, value, duration, start), the state at the end)"""
    L = audiality2_amd.load_library()
    L.a2amd_vm_trace_host_env.restype = ctypes.c_int
    kinds = vp.CHAINS[chain][1]
    wu, wr = [-1] * 64, [0] * 64
    for r, (pos, ureg) in vp.wires(chain).items():
        wu[r], wr[r] = pos, ureg
    c = to_ctypes(st)
    recs = (ctypes.c_uint32 * (4 * cap))()
    k = L.a2amd_vm_trace_host_env(words, ctypes.c_uint(n), ctypes.byref(c), (ctypes.c_int32 * 64)(*wu), (ctypes.c_uint8 * 64)(*wr),
                                  (ctypes.c_int32 * len(kinds))(*kinds), len(kinds), ctypes.c_uint32(now), ctypes.c_uint32(MSDUR),
                                  48000, BASEPITCH, (ctypes.c_uint8 * len(layout))(*layout), (ctypes.c_uint8 * len(base))(*base),
                                  len(layout), None, 0, None, recs, cap)
    assert 0 <= k <= cap, k
    out = []
    for i in range(k):
        head, value, dur, start = recs[4 * i], ctypes.c_int32(recs[4 * i + 1]).value, recs[4 * i + 2], recs[4 * i + 3]
        out.append((head & 0xffff, (head >> 16) & 0xff, (head >> 24) & 15, head >> 28, value, dur, start))
    return out, from_ctypes(c)


def unit_value(kind, ureg, value, transpose):
    """what the unit's write callback makes of an a2_VoiceControl before it is a record (as replay_trace() in
    test_device_vm.py builds `want`): pitch + transpose + base pitch, 1 / q; None: no R_WRITE (the filter's cutoff)"""
    if kind in (vp.WTOSC, vp.FM2) and ureg == 1:
        return vm_model.i32(value + transpose + BASEPITCH)
    if kind == vp.FILTER12 and ureg == 0:
        return None
    if kind == vp.FILTER12 and ureg == 1:
        return 32768 if value < 512 else vm_model.cdiv(65536 << 8, value)
    return value


def model_records(chain, ops_per_fragment, layout):
    """the model's control calls and windows of process() in the form of the host's records"""
    kinds, w = vp.CHAINS[chain][1], vp.wires(chain)
    want = []
    for g, ops in enumerate(ops_per_fragment):
        for o in ops:
            if o[0] == "p":
                if (o[1], o[2]) != (0, layout[g]):
                    want.append((g, "p", o[1], o[2]))
                continue
            _w, _at, reg, value, start, dur, transpose = o
            if reg not in w:
                continue
            pos, ureg = w[reg]
            value = unit_value(kinds[pos], ureg, value, transpose)
            if value is not None:
                want.append((g, "w", pos, ureg, value, dur, start))
            elif dur < 256:
                want.append((g, "c", pos))              # (f12_CutOff without a ramp: the coefficient at once, R_F1SET)
    return want


def host_records(recs, layout):
    got = []
    for frag, op, unit, reg, value, dur, start in recs:
        if op == R_SEG:
            if dur != (layout[frag] << 16):         # (a whole-fragment window is the default window, explicit or not)
                got.append((frag, "p", dur & 0xffff, dur >> 16))
        elif op == R_WRITE:
            got.append((frag, "w", unit, reg, value, dur, start))
        elif op == R_F1SET:
            # A cutoff write is no R_WRITE: the ramper stays with the interpreter and what is recorded is a coefficient,
            # f12_pitch2coeff of the ramper's value through a table made with libm.  Where a write without a ramp stands
            # among the records is compared here; the VALUES written to the cutoff register are not - the GPU tests
            # check those: their oracle gets every cutoff write from the model, value, start, duration and transpose.
            got.append((frag, "c", unit))
        else:
            assert op == R_F1RAMP, op               # (a ramping cutoff's coefficient for a window)
    return got


CASES = [(chain, name) for chain in vp.CHAINS for name in vp.programs(chain)]


@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("chain,name", CASES)
def test_host_interpreter_against_the_model(oracle_lib, chain, name, cut):
    """Every program, from the state the GPU tests hand it over in, over enough fragments for 30 VM runs: the final
    A2_vmstate and every write and window record equal the model's.  cut: every third 64-frame fragment arrives as
    two pieces, 17 + 47 frames, the second with its offset."""
    ptab = pitch_table(oracle_lib)
    words, n = vp.assemble(vp.programs(chain)[name])
    k = 11 + len(name)
    st = vp.start_state(chain, name, k, 64)
    states, _calls = vm_model.run_n(list(words), st, MSDUR, ptab, 30)
    nfr = max((states[-1].waketime >> 8) // 64 + 1, 40)
    layout, base = [], []
    for g in range(nfr):
        if cut and g % 3 == 1:
            layout += [17, 47]
            base += [0, 17]
        else:
            layout.append(64)
            base.append(0)
    ops, ends = vm_model.process(list(words), st, MSDUR, ptab, layout, 0)
    assert sum(1 for f in ops for o in f if o[0] == "p") >= 30
    recs, end = host_trace(words, n, st, chain, layout, base, 0)
    assert end.key() == ends[-1].key(), (end.key(), ends[-1].key())
    got, want = host_records(recs, layout), model_records(chain, ops, layout)
    assert len(want) > 30
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"record {i}: host {g}, model {w}"
    assert len(got) == len(want)


def test_the_programs_execute_the_whole_subset(oracle_lib):
    """... and together they reach every opcode of the subset, every conditional jump both ways, LOOP both ways"""
    ptab = pitch_table(oracle_lib)
    for chain in vp.CHAINS:
        seen = set()
        for name, ins in vp.programs(chain).items():
            words, _n = vp.assemble(ins)
            seen |= vp.executed_opcodes(words, vp.start_state(chain, name, 5, 64), 30, ptab)
        assert seen == vp.SUBSET, (chain, sorted(vp.SUBSET - seen), sorted(seen - vp.SUBSET))
    # the operand of the comparisons and jumps takes all three signs
    words, _n = vp.assemble(vp.programs("osc")["cmpflow"])
    states, _c = vm_model.run_n(list(words), vp.start_state("osc", "cmpflow", 5, 64), MSDUR, ptab, 30)
    assert {s.r[vp.T] for s in states} == {-65536, 0, 65536}
    # the arithmetic program's accumulator takes both signs (negative dividends, both divisors' signs are immediates)
    words, _n = vp.assemble(vp.programs("osc")["arith"])
    states, _c = vm_model.run_n(list(words), vp.start_state("osc", "arith", 5, 64), MSDUR, ptab, 30)
    assert min(s.r[vp.C] for s in states) < 0 < max(s.r[vp.C] for s in states)
    assert min(s.r[vp.S] for s in states) < 0 < max(s.r[vp.S] for s in states)


def test_model_known_answers():
    """the model's own C semantics, against values worked out by hand"""
    m = vm_model
    assert m.cdiv(-7, 2) == -3 and m.cdiv(7, -2) == -3 and m.cdiv(-7, -2) == 3
    assert m.crem(-7, 2) == -1 and m.crem(7, -2) == 1 and m.crem(-7, -2) == -1
    assert m.i32(0x80000000) == -0x80000000 and m.i32(-(-0x80000000)) == -0x80000000
    assert m.ms2t(MSDUR, 3 << 16) == 144 << 8                   # 3 ms at 48 kHz
    assert m.ticks2t(MSDUR, 10 << 16, 1 << 16) == 480 << 8      # one tick of 10 ms
    rt = m.Tracker()
    rt.mark(34)
    rt.mark(2)
    assert rt.regs == [34]                                      # (r and r + 32 share a bit)
    rt.unmark(2)
    assert rt.regs == [34] and rt.mask == 0
    rt.mark(34)
    assert rt.regs == [34, 34]
