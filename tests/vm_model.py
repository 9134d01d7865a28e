"""A plain restatement of the reference's VM arithmetic for the instruction subset of include/a2amd_vm.h, from
src/core.c - Python integers, wrapped to 32 bits by hand, nothing of the library imported:

    flow        JUMP LOOP JZ JNZ JG JL JGE JLE                core.c:1279-1320
    timing      DELAY DELAYR TDELAY TDELAYR                   core.c:1323-1336, :1731-1742; a2_ms2t / a2_ticks2t :1120-1131
    arithmetic  SUBR DIVR P2DR NEGR LOAD LOADR ADD ADDR       core.c:1337-1399
                MUL MULR MOD MODR QUANT QUANTR
    compare     GR LR GER LER EQR NER ANDR ORR XORR NOTR      core.c:1413-1456
    control     SET SETALL RAMP RAMPR RAMPALL RAMPALLR        core.c:1458-1489, through the register tracker :1064-1116
    a2_P2I      pitch.c:57-67, over the pitch table handed in (128 words: 64 x {base, coeff})

What C leaves to the target - and gcc on x86-64 settles one way - is written out here: division truncates toward zero,
the remainder takes the dividend's sign, >> of a negative value is arithmetic, a shift count is taken modulo 32 for a
32 bit operand (so `1 << r` gives registers r and r + 32 one tracker bit, and a2_P2I's `>> (7 - oct)` wraps), products
and quotients are 64 bit before the cast to int, the cast keeps the low 32 bits.

run() is one a2_VoiceProcessVM, run_until() the VM runs a2_VoiceProcess makes up to a frame-aligned engine time,
process() a2_VoiceProcess itself over a list of fragments: the VM runs and the windows between them."""

OPS = ("END RETURN CALL JUMP LOOP JZ JNZ JG JL JGE JLE DELAY DELAYR TDELAY TDELAYR SLEEP WAKE FORCE SUBR DIVR P2DR NEGR "
       "LOAD LOADR ADD ADDR MUL MULR MOD MODR QUANT QUANTR RAND RANDR GR LR GER LER EQR NER ANDR ORR XORR NOTR SET SETALL "
       "RAMP RAMPR RAMPALL RAMPALLR").split()     # A2_opcodes, src/internals.h:152-207
NAME = dict(enumerate(OPS))
INSLIMIT = 1000                                   # A2_INSLIMIT, src/config.h:119
R_TICK, R_TRANSPOSE = 0, 1                        # include/a2_vm.h:52
WAITING, RUNNING = 1, 0                           # A2_vstates, include/a2_vm.h:41-48
A2_1K_DIV_MIDDLEC = 4202608409623                 # include/a2_pitch.h:42


def i32(x):
    """the low 32 bits as a signed int: what a cast to int, or int arithmetic that wraps, leaves"""
    return ((x + (1 << 31)) & 0xffffffff) - (1 << 31)


def u32(x):
    return x & 0xffffffff


def i64(x):
    return ((x + (1 << 63)) & 0xffffffffffffffff) - (1 << 63)


def cdiv(a, b):
    """C's a / b: truncated toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def crem(a, b):
    """C's a % b: a - (a / b) * b, the dividend's sign"""
    return a - cdiv(a, b) * b


def ms2t(msdur, d):
    """a2_ms2t, core.c:1128-1131: (int64_t)d * msdur + 0x7fffff >> 24 (arithmetic), returned as unsigned"""
    return u32((d * msdur + 0x7fffff) >> 24)


def ticks2t(msdur, tick, d):
    """a2_ticks2t, core.c:1120-1124: the products are unsigned 64 bit (a negative d or tick is a huge number there)"""
    t = (((d & 0xffffffffffffffff) * (tick & 0xffffffffffffffff) + 127) & 0xffffffffffffffff) >> 8
    return u32(((t * msdur + 0x7fffffff) & 0xffffffffffffffff) >> 32)


def p2i(ptab, pitch):
    """a2_P2I, pitch.c:57-67: unsigned 32 bit arithmetic, the shift count modulo 32"""
    n, octave = pitch & 0xffff, pitch >> 16
    dph = u32(ptab[2 * (n >> 10) + 1] * (n & 0x3ff))
    dph >>= 2
    dph = u32(dph + ptab[2 * (n >> 10)])
    return dph >> ((7 - octave) & 31)


class Tracker:
    """A2_regtracker, core.c:1064-1099"""

    def __init__(self):
        self.mask, self.regs = 0, []

    def mark(self, r):
        b = 1 << (r & 31)
        if b & self.mask:
            return
        self.mask |= b
        self.regs.append(r)

    def unmark(self, r):
        b = 1 << (r & 31)
        if b & self.mask:
            self.mask &= ~b
            if r in self.regs:                  # (regs[i] = regs[--position])
                i = self.regs.index(r)
                last = self.regs.pop()
                if i < len(self.regs):
                    self.regs[i] = last


class State:
    """A2_vmstate, include/a2_vm.h:62-69"""

    def __init__(self, waketime=0, pc=0, r=None, state=WAITING):
        self.waketime, self.pc, self.state = u32(waketime), pc, state
        self.r = list(r) if r is not None else [0] * 64

    def copy(self):
        return State(self.waketime, self.pc, self.r, self.state)

    def key(self):
        return (self.waketime, self.state, self.pc, tuple(self.r))


def run(code, st, msdur, ptab, calls, seen=None):
    """One a2_VoiceProcessVM (core.c:1166-1744) on `st`: instructions up to a timing instruction with dt > 0.
    `code`: 32 bit words.  Every a2_VoiceControl it makes is appended to `calls` as
    (time of the run, register, r[register], start & 255, duration, r[R_TRANSPOSE]); the names of the opcodes it
    executes are added to the set `seen`."""
    r = st.r
    rt = Tracker()
    at = st.waketime
    inscount = INSLIMIT
    if st.state == WAITING:
        st.state = RUNNING

    def control(reg, dur):                      # a2_VoiceControl, core.c:143-149
        calls.append((at, reg, r[reg], at & 255, dur, r[R_TRANSPOSE]))

    def apply(dur):                             # a2_RTApply, core.c:1101-1107
        for reg in list(rt.regs):
            control(reg, dur)

    while True:
        w = code[st.pc]
        op, a1, a2 = NAME.get(w & 0xff), (w >> 8) & 0xff, (w >> 16) & 0xffff
        a3 = i32(code[st.pc + 1]) if st.pc + 1 < len(code) else 0
        if seen is not None:
            seen.add(op)
        inscount -= 1
        if not inscount:
            raise RuntimeError("A2_OVERLOAD")
        dt = None
        if op == "JUMP":
            st.pc = a2
            continue
        if op == "LOOP":
            r[a1] = i32(r[a1] - 65536)
            if r[a1] > 0:
                st.pc = a2
                continue
        elif op in ("JZ", "JNZ", "JG", "JL", "JGE", "JLE"):
            v = r[a1]
            if {"JZ": v == 0, "JNZ": v != 0, "JG": v > 0, "JL": v < 0, "JGE": v >= 0, "JLE": v <= 0}[op]:
                st.pc = a2
                continue
        elif op == "DELAY":
            dt = ms2t(msdur, a3)
            st.pc += 1
        elif op == "DELAYR":
            dt = ms2t(msdur, r[a1])
        elif op == "TDELAY":
            dt = ticks2t(msdur, r[R_TICK], a3)
            st.pc += 1
        elif op == "TDELAYR":
            dt = ticks2t(msdur, r[R_TICK], r[a1])
        elif op == "SUBR":
            r[a1] = i32(r[a1] - r[a2])
            rt.mark(a1)
        elif op == "DIVR":
            if not r[a2]:
                raise ZeroDivisionError("VM:DIVR")
            r[a1] = i32(cdiv(i64(r[a1] << 16), r[a2]))
            rt.mark(a1)
        elif op == "P2DR":
            r[a1] = i32(cdiv(A2_1K_DIV_MIDDLEC, p2i(ptab, r[a2])))
            rt.mark(a1)
        elif op == "NEGR":
            r[a1] = i32(-r[a2])
            rt.mark(a1)
        elif op == "LOAD":
            r[a1] = a3
            rt.mark(a1)
            st.pc += 1
        elif op == "LOADR":
            r[a1] = r[a2]
            rt.mark(a1)
        elif op == "ADD":
            r[a1] = i32(r[a1] + a3)
            rt.mark(a1)
            st.pc += 1
        elif op == "ADDR":
            r[a1] = i32(r[a1] + r[a2])
            rt.mark(a1)
        elif op == "MUL":
            r[a1] = i32((r[a1] * a3) >> 16)
            rt.mark(a1)
            st.pc += 1
        elif op == "MULR":
            r[a1] = i32((r[a1] * r[a2]) >> 16)
            rt.mark(a1)
        elif op == "MOD":
            r[a1] = crem(r[a1], a3)
            rt.mark(a1)
            st.pc += 1
        elif op == "MODR":
            if not r[a2]:
                raise ZeroDivisionError("VM:MODR")
            r[a1] = crem(r[a1], r[a2])
            rt.mark(a1)
        elif op == "QUANT":
            r[a1] = i32(cdiv(r[a1], a3) * a3)
            rt.mark(a1)
            st.pc += 1
        elif op == "QUANTR":
            if not r[a2]:
                raise ZeroDivisionError("VM:QUANTR")
            r[a1] = i32(cdiv(r[a1], r[a2]) * r[a2])
            rt.mark(a1)
        elif op in ("GR", "LR", "GER", "LER", "EQR", "NER", "ANDR", "ORR", "XORR"):
            x, y = r[a1], r[a2]
            t = {"GR": x > y, "LR": x < y, "GER": x >= y, "LER": x <= y, "EQR": x == y, "NER": x != y,
                 "ANDR": bool(x) and bool(y), "ORR": bool(x) or bool(y), "XORR": (not x) != (not y)}[op]
            r[a1] = int(t) << 16
            rt.mark(a1)
        elif op == "NOTR":
            r[a1] = int(not r[a2]) << 16
            rt.mark(a1)
        elif op == "SET":
            control(a1, 0)
            rt.unmark(a1)
        elif op == "SETALL":                    # a2_RTSetAll, core.c:1109-1116
            apply(0)
            rt = Tracker()
        elif op == "RAMP":
            control(a1, ms2t(msdur, a3))
            rt.unmark(a1)
            st.pc += 1
        elif op == "RAMPR":
            control(a1, ms2t(msdur, r[a2]))
            rt.unmark(a1)
        elif op == "RAMPALL":
            apply(ms2t(msdur, a3))
            rt = Tracker()
            st.pc += 1
        elif op == "RAMPALLR":
            apply(ms2t(msdur, r[a1]))
            rt = Tracker()
        else:
            raise ValueError(f"opcode {w & 0xff} at {st.pc} is outside the subset")
        st.pc += 1
        if dt is None:
            continue
        apply(dt)                               # "timing:", core.c:1731-1736 - the tracker is NOT reset
        if not dt:
            continue
        st.state = WAITING
        st.waketime = u32(st.waketime + dt)
        return


def run_n(code, st, msdur, ptab, nruns):
    """`nruns` VM runs from the state `st` (left alone): ([state after each run], [control calls])"""
    st = st.copy()
    states, calls = [], []
    for _ in range(nruns):
        run(code, st, msdur, ptab, calls)
        states.append(st.copy())
    return states, calls


def run_until(code, st, msdur, ptab, end):
    """The VM runs a2_VoiceProcess (core.c:1847-1880, with the "VM only" loop :1818-1834) makes in the windows before
    the frame-aligned engine time `end`: the VM runs at a window start `now` while a2_TSDiff(waketime, now) <= 255,
    and the window then ends at the wake time's frame - so every run whose wake time lies in a frame before `end`."""
    assert end & 255 == 0
    st = st.copy()
    states, calls = [], []
    while i32(st.waketime - end) < 0:
        run(code, st, msdur, ptab, calls)
        states.append(st.copy())
    return states, calls


def process(code, st, msdur, ptab, layout, t0):
    """a2_VoiceProcess (core.c:1847-1880) over fragments of layout[] frames, the first starting at engine time t0: at
    every window start the VM runs while it is due within that frame, then the units get the window up to the frame
    of the next wake time.  Per fragment the list of what the engine does to the voice, in order -
    ("w", time, register, value, start, duration, transpose) for an a2_VoiceControl, ("p", offset, frames) for the
    units' Process - and the state at the end of every fragment.  `st` is left alone."""
    st = st.copy()
    out, ends = [], []
    fs = u32(t0)
    for frames in layout:
        ops, s = [], 0
        while s < frames:
            t = u32(fs + (s << 8))
            while True:
                nextvm = i32(st.waketime - t)           # a2_TSDiff
                if nextvm > 255:
                    res = nextvm >> 8
                    break
                calls = []
                run(code, st, msdur, ptab, calls)
                ops += [("w",) + c for c in calls]
            res = min(res, frames - s)
            ops.append(("p", s, res))
            s += res
        out.append(ops)
        ends.append(st.copy())
        fs = u32(fs + (frames << 8))
    return out, ends
