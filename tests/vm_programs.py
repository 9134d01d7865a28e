"""Hand-assembled VM programs for the direct device-VM tests (test_vm_model.py on the CPU, test_gpu_vm_direct.py on the
GPU): each is `body; DELAY; JUMP 0`.  The bodies compute in unwired scratch registers with edge operands and derive the
wired registers from them through MOD / MUL, so the audio depends on the arithmetic while every wired value stays
in range: pitch within +-2 octaves, gains and pan within +-1.0, cutoff 0 .. 4 octaves, q >= 1.0.

Together they execute every opcode of the subset (include/a2amd_vm.h): test_vm_model.py counts them from the model's runs."""
from test_device_vm import MSDUR, OP, TWO, asm, fx

import vm_model

# a2amd_unitkind, include/a2amd.h
WTOSC, PANMIX, FILTER12, FM2 = 0, 1, 2, 7

# VM registers: the two the engine names, the wired ones (P A VOL PAN in every chain, X1 .. X4 by chain), scratch.
# Scratch stays clear of the twins (r + 32) of everything else - except where a program is about them.
TICK, TR, P, A, VOL, PAN, X1, X2, X3, X4 = range(10)
ACC, C, S, D, T, U, Z, X, L, N = 10, 16, 17, 18, 19, 20, 21, 22, 23, 24
TMP = list(range(25, 32))
P_TWIN = P + 32

# chain -> (synth.Scene's name, unit kinds, [(VM register, chain position, unit register, modulus, base)]): a wired
# register is made as scratch % modulus + base, |value - base| < modulus
CHAINS = {
    "osc": ("osc-pan", [WTOSC, PANMIX],
            [(P, 0, 1, fx(1.75), 0), (A, 0, 2, 3000, 500), (VOL, 1, 0, fx(.45), fx(.5)), (PAN, 1, 1, fx(.95), 0)]),
    "osc2": ("osc2-pan", [WTOSC, WTOSC, PANMIX],
             [(P, 0, 1, fx(1.75), 0), (A, 0, 2, 3000, 500), (VOL, 2, 0, fx(.45), fx(.5)), (PAN, 2, 1, fx(.95), 0),
              (X1, 1, 1, fx(1.75), 0), (X2, 1, 2, 3000, 500)]),
    "filt": ("osc-filter-pan", [WTOSC, FILTER12, PANMIX],
             [(P, 0, 1, fx(1.75), 0), (A, 0, 2, 3000, 500), (VOL, 2, 0, fx(.45), fx(.5)), (PAN, 2, 1, fx(.95), 0),
              (X1, 1, 0, fx(1.9), fx(2)), (X2, 1, 1, fx(1.9), fx(3)), (X3, 1, 2, fx(.45), fx(.5)), (X4, 1, 3, fx(.95), 0)]),
    "fm2": ("fm2-pan", [FM2, PANMIX],
            [(P, 0, 1, fx(1.75), 0), (A, 0, 2, 3000, 500), (VOL, 1, 0, fx(.45), fx(.5)), (PAN, 1, 1, fx(.95), 0),
             (X1, 0, 3, fx(.2), fx(.25)), (X2, 0, 4, fx(.9), fx(1.5)), (X3, 0, 5, fx(.45), fx(.5))]),
}
CLASSES = ("osc", "osc2", "filt")       # the three window classes, in a2amd_vm_batch_info.class_voices' order
CUT = X1                                # (of "filt")


def wires(chain):
    return {r: (pos, ureg) for r, pos, ureg, _m, _b in CHAINS[chain][2]}


def ms_for_ticks(t):
    """the DELAY / RAMP immediate whose a2_ms2t is exactly t ticks (24:8 frames)"""
    d = -((-((t << 24) - 0x7fffff)) // MSDUR)
    assert vm_model.ms2t(MSDUR, d) == t, t
    return d


def assemble(ins):
    """instructions with ("label", name) among them and label names as jump targets -> (words, n) as asm() makes them"""
    at, pos = {}, 0
    for i in ins:
        if i[0] == "label":
            at[i[1]] = pos
        else:
            pos += 2 if i[0] in TWO else 1
    out = []
    for i in ins:
        if i[0] == "label":
            continue
        i = list(i)
        if isinstance(i[2], str):
            i[2] = at[i[2]]
        out.append(tuple(i))
    return asm(*out)


def derive(chain, reg, src, scale=None):
    """reg = src [* scale] % modulus + base"""
    _r, _pos, _ureg, mod, base = next(w for w in CHAINS[chain][2] if w[0] == reg)
    return ([("LOADR", reg, src)] + ([("MUL", reg, 0, scale)] if scale is not None else []) + [("MOD", reg, 0, mod)] +
            ([("ADD", reg, 0, base)] if base else []))


def extras(chain, src):
    """every wired register beyond P A VOL PAN (the second oscillator, the filter, the FM operator) from src"""
    out = []
    for k, w in enumerate(CHAINS[chain][2][4:]):
        out += derive(chain, w[0], src, fx(1.0 + 0.21 * (k + 1)))
    return out


def use(reg):
    return [("ADDR", ACC, reg)]


def p_arith(chain):
    """64 bit products of both signs, truncating / and % with every combination of signs, DIVR with a quotient that wraps,
    NEGR of INT_MIN, ADD / SUBR across the wrap, P2DR where a2_P2I's shift count is negative and where it is >= 32.
    (DIVR / MODR / QUANTR: the voice is taken for a stretch, not for good.)"""
    t = TMP
    return ([("LOAD", ACC, 0, 0),
             ("ADD", C, 0, 0x7fffff00), ("ADD", C, 0, 0x12345),            # C wraps every other run: both signs below
             ("SUBR", S, C)] + use(S) +
            [("LOAD", t[0], 0, 0x7fff0000), ("MUL", t[0], 0, 0x7ffe0001)] + use(t[0]) +         # + * +: 62 bits
            [("LOAD", t[1], 0, -0x7fff0000), ("MULR", t[1], t[0])] + use(t[1]) +
            [("LOAD", t[2], 0, -0x6789abcd), ("MUL", t[2], 0, -0x07654321)] + use(t[2]) +       # - * -: 58 bits
            [("LOADR", t[3], C), ("MULR", t[3], S)] + use(t[3]) +                              # whatever the signs are
            [("LOAD", t[4], 0, -0x80000000), ("NEGR", t[5], t[4])] + use(t[5]) +
            [("NEGR", t[5], C)] + use(t[5]) +
            [("LOADR", t[0], S), ("MOD", t[0], 0, 7777)] + use(t[0]) +
            [("LOADR", t[0], C), ("MOD", t[0], 0, -7777)] + use(t[0]) +
            [("LOADR", t[0], S), ("QUANT", t[0], 0, -30011)] + use(t[0]) +
            [("LOADR", t[0], C), ("QUANT", t[0], 0, 30011)] + use(t[0]) +
            [("LOAD", t[1], 0, 30011), ("LOAD", t[2], 0, -4099),
             ("LOADR", t[0], S), ("MODR", t[0], t[1])] + use(t[0]) +
            [("LOADR", t[0], C), ("MODR", t[0], t[2])] + use(t[0]) +
            [("LOADR", t[0], S), ("QUANTR", t[0], t[2])] + use(t[0]) +
            [("LOADR", t[0], C), ("QUANTR", t[0], t[1])] + use(t[0]) +
            [("LOAD", t[0], 0, 0x7fff0000), ("LOAD", t[3], 0, 3), ("DIVR", t[0], t[3])] + use(t[0]) +     # wraps int32
            [("LOAD", t[0], 0, -0x07654321), ("LOAD", t[3], 0, 0x5000), ("DIVR", t[0], t[3])] + use(t[0]) +
            [("LOADR", t[0], C), ("DIVR", t[0], t[2])] + use(t[0]) +
            [("LOAD", t[3], 0, fx(9.3)), ("P2DR", t[0], t[3])] + use(t[0]) +                   # shift count 7 - 9 = -2 (30 modulo 32)
            [("LOAD", t[3], 0, fx(-26.5)), ("P2DR", t[0], t[3])] + use(t[0]) +                 # shift count 34
            [("LOAD", t[3], 0, fx(-40.25)), ("P2DR", t[0], t[3])] + use(t[0]) +                # shift count 48
            [("LOADR", t[3], C), ("MOD", t[3], 0, fx(3)), ("P2DR", t[0], t[3])] + use(t[0]) +
            derive(chain, P, ACC) + derive(chain, A, ACC, fx(.37)) + derive(chain, VOL, S) + derive(chain, PAN, C) +
            extras(chain, ACC) +
            [("DELAY", 0, 0, fx(7.3)), ("JUMP", 0, 0)])


CMP_OPS = ("GR", "LR", "GER", "LER", "EQR", "NER", "ANDR", "ORR", "XORR")
JUMPS = ("JZ", "JNZ", "JG", "JL", "JGE", "JLE")


def p_cmpflow(chain):
    """T goes -1, 0, 1 from run to run: every comparison and boolean operator against 0 and against -T (smaller, equal,
    larger), every conditional jump taken and not taken, LOOP with a count of 2.5, with one below zero and with a
    whole one, which ends on exactly 0 (a DELAY inside each: the analysis wants a certain yield in every cycle)."""
    body = [("ADD", C, 0, fx(1)), ("LOADR", T, C), ("MOD", T, 0, fx(3)), ("QUANT", T, 0, fx(1)), ("ADD", T, 0, -fx(1)),
            ("NEGR", U, T), ("LOAD", Z, 0, 0), ("LOAD", ACC, 0, 0)]
    for k, op in enumerate(CMP_OPS):
        for other in (Z, U):
            body += [("LOADR", X, T), (op, X, other), ("MUL", X, 0, fx(.013 * (k + 1)))] + use(X)
    body += [("NOTR", X, T), ("MUL", X, 0, fx(.31))] + use(X)
    # (two operands that are both true and share no bit: the boolean operators are not the bitwise ones)
    for k, op in enumerate(("ANDR", "ORR", "XORR")):
        body += [("LOAD", X, 0, 0x10000), ("LOAD", N, 0, 0x20000), (op, X, N), ("MUL", X, 0, fx(.17 * (k + 1)))] + use(X)
    for k, j in enumerate(JUMPS):
        body += [(j, T, f"skip{k}"), ("ADD", ACC, 0, 0x1111 << k), ("label", f"skip{k}")]
    body += ([("LOAD", L, 0, fx(2.5)), ("label", "top"), ("ADD", ACC, 0, 0x333)] + derive(chain, PAN, ACC, fx(3.7)) +
             [("DELAY", 0, 0, fx(1.7)), ("LOOP", L, "top"),
              ("LOAD", L, 0, -fx(1.5)), ("label", "top2"), ("ADD", ACC, 0, 0x77)] + derive(chain, A, ACC, fx(.11)) +
             [("DELAY", 0, 0, fx(.9)), ("LOOP", L, "top2"),
              ("LOAD", L, 0, fx(2.0)), ("label", "top3"), ("ADD", ACC, 0, 0x5)] + derive(chain, VOL, ACC, fx(7.7)) +
             [("DELAY", 0, 0, fx(.6)), ("LOOP", L, "top3")] +            # (a whole count: ends on exactly 0)
             derive(chain, P, ACC, fx(5.3)) + [("SET", P, 0)] +
             derive(chain, VOL, ACC, fx(2.9)) + [("RAMP", VOL, 0, fx(2.0))] +
             [("DELAY", 0, 0, fx(3.1)), ("JUMP", 0, 0)])
    return body


def p_timing(chain):
    """TDELAY / TDELAYR with a tick the program LOADs in the same run, DELAYR / RAMPR / RAMPALLR from registers, a
    DELAY 0 between two writes of one register and behind the only write of another: the tracker is applied twice and
    is not reset in between (core.c:1734-1736) - the second register goes out again with the next delay's duration."""
    return ([("ADD", C, 0, fx(.37)), ("LOADR", D, C), ("MOD", D, 0, fx(2)), ("ADD", D, 0, fx(1.5)),
             # (a tick and a count at which a2_ticks2t's "+ 127" decides the result: 24 590 ticks, 24 589 without it)
             ("LOAD", TICK, 0, fx(2.5) + 5)] + derive(chain, P, C, fx(1.7)) + [("TDELAY", 0, 0, fx(.8) + 27),
             ("LOAD", TICK, 0, fx(1.25))] + derive(chain, PAN, C, fx(2.3)) + [("TDELAYR", D, 0)] +
            derive(chain, VOL, D, fx(3.1)) + [("DELAYR", D, 0)] +
            derive(chain, A, C, fx(.07)) + [("RAMPR", A, D)] +
            derive(chain, VOL, C, fx(1.3)) + derive(chain, PAN, D, fx(.9)) + extras(chain, C) + [("RAMPALLR", D, 0),
             ("LOAD", P, 0, fx(.25))] + derive(chain, PAN, C, fx(.6)) + [("DELAY", 0, 0, 0), ("ADD", P, 0, fx(.125)),
             # (PAN is left alone behind the zero delay: its second write, over the 5 ms, is the tracker's that was not reset)
             ("DELAY", 0, 0, fx(5.0)), ("JUMP", 0, 0)])


def p_many(chain):
    """More records in one run than a lane of k_vm_win holds before it gives way to a drain (VMW_GIVEWAY), and the
    run gives way while the tracker holds wired registers: every wired register is made - and marked - first; eight
    explicit writes of the first two follow (SET / RAMP, each re-marked by an ADD) while the others wait in the tracker;
    SETALL then carries out all of them - what a tracker lost at the re-entry would not - and resets the tracker.  Then
    RAMP on every register but PAN, and the final DELAY's pass through the tracker, which no longer holds PAN."""
    w = CHAINS[chain][2]
    body = [("ADD", C, 0, 0x3c71)]
    for k, (r, _pos, _ureg, _mod, _base) in enumerate(w):
        body += derive(chain, r, C, fx(1.0 + .37 * k))
    for (r, _pos, _ureg, mod, _base), write in zip(w[:2], (lambda r: ("SET", r, 0), lambda r: ("RAMP", r, 0, fx(1.0)))):
        step = mod // 64
        body += [write(r), ("ADD", r, 0, step)] * 4 + [("ADD", r, 0, -4 * step)]
    body += [("SETALL", 0, 0)]
    # (PAN is left alone behind SETALL: a tracker that SETALL had not reset would write it again at the DELAY)
    rest = [x for x in w if x[0] != PAN]
    for r, _pos, _ureg, mod, _base in rest:
        body += [("ADD", r, 0, mod // 64), ("RAMP", r, 0, fx(1.5))]
    body += [("ADD", r, 0, -(mod // 64)) for r, _pos, _ureg, mod, _base in rest]
    return body + [("DELAY", 0, 0, fx(9.0)), ("JUMP", 0, 0)]


def p_fast(chain):
    """wakes every 5.28 frames: a dozen windows per fragment"""
    return [("ADD", C, 0, 0x2f1)] + derive(chain, PAN, C, fx(9.1)) + derive(chain, P, C) + [("DELAY", 0, 0, fx(.11)), ("JUMP", 0, 0)]


def p_long(chain):
    """more than 1 024 words of text, fewer than A2AMD_VM_INSLIMIT instructions between two delays"""
    return ([("ADD", C, 0, 0x1f35)] + derive(chain, P, C, fx(2.1)) + [("DELAY", 0, 0, fx(3.0))] +
            [("ADDR", S, C)] * 700 + derive(chain, A, S) + [("DELAY", 0, 0, fx(2.0))] +
            [("ADDR", S, C)] * 500 + derive(chain, PAN, S) + [("DELAY", 0, 0, fx(2.5)), ("JUMP", 0, 0)])


def p_sleep40(chain):
    """two writes without a ramp, then 40 ms of sleep: idle in most batches"""
    return ([("ADD", C, 0, 0x4567)] + derive(chain, P, C, fx(1.9)) + [("SET", P, 0)] + derive(chain, PAN, C, fx(4.3)) +
            [("SET", PAN, 0), ("DELAY", 0, 0, fx(40.0)), ("JUMP", 0, 0)])


def p_sleep100(chain):
    """a 2 ms ramp, a RAMPALL over 1 ms, then 100 ms of sleep"""
    return ([("ADD", C, 0, 0x89ab)] + derive(chain, VOL, C, fx(1.1)) + [("RAMP", VOL, 0, fx(2.0))] + extras(chain, C) + derive(chain, PAN, C) +
            [("RAMPALL", 0, 0, fx(1.0)), ("DELAY", 0, 0, fx(100.0)), ("JUMP", 0, 0)])


def p_twin(chain, dynamic=True):
    """Registers r and r + 32 share a bit of the tracker's mask (core.c:1076-1099): r34 marked first keeps P off the list
    (P's write is lost); unmarking r34 while P holds the bit leaves P listed with the bit clear, and P is listed twice.
    dynamic: with a DIVR, so that a2amd_vm_adopt takes the voice for a stretch; without, it refuses the program."""
    return ([("ADD", C, 0, 0x999), ("LOADR", X, C)] +
            ([("LOAD", TMP[0], 0, 3), ("DIVR", X, TMP[0])] if dynamic else [("MUL", X, 0, fx(21845.3))]) +
            [("LOADR", P_TWIN, C)] + derive(chain, P, X) + derive(chain, PAN, X) + [("DELAY", 0, 0, fx(4.0))] +
            derive(chain, P, C) + [("LOADR", P_TWIN, X), ("SET", P_TWIN, 0), ("ADD", P, 0, 1), ("DELAY", 0, 0, fx(4.0)), ("JUMP", 0, 0)])


# the voices running p_cutend wake at frame CUTEND_OFF + CUTEND_FRAC / 256 of a fragment, every four fragments
CUTEND_OFF, CUTEND_FRAC = 20, 0x40


def p_cutend(chain):
    """A cutoff ramp that ends exactly at a fragment boundary: started at frame 20.25 of a fragment with a duration that
    brings the ramper's timer to (44 + 64) frames - zero behind the next fragment's window, its delta still set."""
    assert chain == "filt"
    return ([("ADD", C, 0, fx(.21))] + derive(chain, CUT, C) +
            [("RAMP", CUT, 0, ms_for_ticks(((64 - CUTEND_OFF + 64) << 8) - CUTEND_FRAC))] +
            derive(chain, PAN, C) + [("SET", PAN, 0), ("DELAY", 0, 0, ms_for_ticks(256 << 8)), ("JUMP", 0, 0)])


def programs(chain):
    """name -> instructions, in the order the voices of a scene are given them (voice k: program k mod their number)"""
    p = dict(arith=p_arith(chain), cmpflow=p_cmpflow(chain), timing=p_timing(chain), many=p_many(chain), fast=p_fast(chain),
             long=p_long(chain), sleep40=p_sleep40(chain), sleep100=p_sleep100(chain), twin=p_twin(chain))
    if chain == "filt":
        p["cutend"] = p_cutend(chain)
    return p


def start_state(chain, name, k, wake_frame):
    """voice k's A2_vmstate when it is handed over: waiting, its wake time inside the fragment that starts at wake_frame,
    with a fraction that is not zero"""
    st = vm_model.State()
    off, frac = (7 * k + 3) % 64, 1 + (37 * k) % 255
    if name == "cutend":
        off, frac = CUTEND_OFF, CUTEND_FRAC
    st.waketime = ((wake_frame + off) << 8) | frac
    st.r[TICK] = fx(1)
    st.r[TR] = ((k % 5) - 2) * (fx(1) // 24)        # transpose: up to a semitone either way
    st.r[C] = k * 0x1234
    st.r[S] = -k * 0x4321
    for r, _pos, _ureg, _mod, base in CHAINS[chain][2]:
        st.r[r] = base
    return st


def executed_opcodes(words, st, nruns, ptab):
    """the opcodes `nruns` runs of the program execute, by name (the model says which)"""
    seen, s, calls = set(), st.copy(), []
    for _ in range(nruns):
        vm_model.run(list(words), s, MSDUR, ptab, calls, seen)
    return seen


SUBSET = set("JUMP LOOP JZ JNZ JG JL JGE JLE DELAY DELAYR TDELAY TDELAYR SUBR DIVR P2DR NEGR LOAD LOADR ADD ADDR MUL MULR MOD "
             "MODR QUANT QUANTR GR LR GER LER EQR NER ANDR ORR XORR NOTR SET SETALL RAMP RAMPR RAMPALL RAMPALLR".split())
assert SUBSET <= set(OP)
