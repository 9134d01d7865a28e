"""The device VM's kernels - k_vm_count / k_vm_emit / k_vm_pool (a2amd_vm.hip), k_vm_win<NOSC,FILT> / k_vm_commit
(a2amd_vmwin.hip), the speculative pass (vm_speculate, a2amd_vm.cpp) - driven through the C ABI alone: synthetic voices are
handed over with a2amd_vm_adopt, rendered batch by batch, taken back with a2amd_vm_recall.  No engine, no reference
binary, no preload.

What is compared, all of it exactly:
  audio      every batch against the oracle's render of the same scene, in which the adopted voices get their writes and
             windows as calls - made by tests/vm_model.py, the plain restatement of the reference's VM that
             test_vm_model.py pins the host copy of the interpreter to
  state      every A2_vmstate a2amd_vm_recall returns against the model's AND against the host interpreter's
             (a2amd_vm_trace_host_env) after the same fragments
  path       a2amd_last_batch_vm() of every batch against a sequence written out in the test: which kernels ran the VMs

The scenes: 70 voices of one chain under the root (one full block of k_vm_win's 64 lanes and six more), the programs of
tests/vm_programs.py dealt round robin - every block mixes them.  Every voice is adopted in the second fragment of the
second batch, with a wake time inside the next fragment and a fraction that is not zero."""
import pytest

from audiality2_amd import synth
from audiality2_amd.replay import a2amd_vm_state
from conftest import make_gpu, make_oracle
from test_device_vm import MSDUR, fx
from test_gpu_parity import first_diff, last_batch
from test_vm_model import from_ctypes, host_trace

import vm_model
import vm_programs as vp

gpu = pytest.mark.gpu
NV = 70
EUNSUPPORTED = -4           # A2AMD_EUNSUPPORTED, include/a2amd.h
NOT_ASKED = 6               # A2AMD_VM_NOT_ASKED, include/a2amd_vmbatch.h


# ---- the scene and its two players ------------------------------------------------------------
class Voice:
    def __init__(self, chain, k, units, name, words, n):
        self.chain, self.k, self.units, self.name, self.words, self.n = chain, k, units, name, words, n
        self.mode = "plain"         # "vm": the device VM's (GPU); "model": driven by calls made from the model
        self.st0 = self.g0 = None   # the state it was handed over in; the first fragment the VM is in charge of
        self.ops, self.ends = {}, {}


def steps_frag(frames=64, off=0):
    return [("open", frames, off), ("leaves",)]


def steps_batch(layout=8):
    """one batch: `layout` 64-frame fragments, or [(frames, offset inside the engine's fragment)]"""
    if isinstance(layout, int):
        layout = [(64, 0)] * layout
    out = []
    for frames, off in layout:
        out += steps_frag(frames, off)
    return out + [("render",)]


def cut(at):
    """a 64-frame fragment as the engine cuts it where the root's VM wakes: two pieces, the second with its offset"""
    return [(at, 0), (64 - at, at)]


class Rig:
    """One scene on one backend.  run() plays a list of steps:
      ("open", frames, offset) ("leaves",)   a fragment: opened, the voices walked
      ("adopt", [voice])                     in the open fragment, behind its walk
      ("recall", [voice])                    in the open fragment before its walk, or between two batches
      ("write", voice, position, register, value, duration)   a host write to a voice that is not adopted
      ("pre_ramp",)                          a long cutoff ramp on every second filter voice
      ("cuts", [engine time])                a2amd_vm_expect_cuts
      ("render",)
    On the GPU adopted voices are the device VM's (their fragments marked default) until they are recalled; then, and on
    the oracle from the start, they are driven by calls made from the model."""

    def __init__(self, be, on_gpu, chains, settled=0, ptab=None):
        self.be, self.on_gpu = be, on_gpu
        self.ptab = ptab if ptab is not None else [int(x) for x in be.get_pitch_table()]
        self.sc = synth.Scene(be)
        self.sc.root()
        self.voices = []
        for chain in chains:
            first = len(self.sc.leaves)
            self.sc.add_voices(NV, vp.CHAINS[chain][0])
            progs = vp.programs(chain)
            names = list(progs)
            asm = {name: vp.assemble(progs[name]) for name in names}
            for k in range(NV):
                name = names[k % len(names)]
                self.voices.append(Voice(chain, k, self.sc.leaves[first + k], name, *asm[name]))
        self.nplain = settled
        if settled:
            self.sc.add_voices(settled, "osc-pan")
        self.plain = self.sc.leaves[len(self.voices):]
        self.progids = {}
        self.audio, self.infos, self.slabs, self.recalled = [], [], [], 0

    # -- time --
    def lay_out(self, steps):
        self.layout = [(s[1], s[2]) for s in steps if s[0] == "open"]
        self.tstart = [0]
        for frames, _off in self.layout:
            self.tstart.append(self.tstart[-1] + (frames << 8))

    def drive(self, v, st, g0):
        """the voice from fragment g0 on, by the model, from the state st"""
        ops, ends = vm_model.process(list(v.words), st, MSDUR, self.ptab, [f for f, _o in self.layout[g0:]], self.tstart[g0])
        for i, (o, e) in enumerate(zip(ops, ends)):
            v.ops[g0 + i], v.ends[g0 + i] = o, e

    # -- steps --
    def adopt(self, vs, g):
        for v in vs:
            v.st0, v.g0 = vp.start_state(v.chain, v.name, v.k, self.tstart[g + 1] >> 8), g + 1
            self.drive(v, v.st0, g + 1)
            v.mode = "model"
            if not self.on_gpu:
                continue
            key = (v.chain, v.name)
            if key not in self.progids:
                self.progids[key] = self.be.vm_program(0x5000 + len(self.progids), list(v.words))
            c = a2amd_vm_state()
            c.waketime, c.state, c.pc = v.st0.waketime, v.st0.state, v.st0.pc
            for i, x in enumerate(v.st0.r):
                c.r[i] = x
            w = {r: (v.units[pos], ureg) for r, (pos, ureg) in vp.wires(v.chain).items()}
            self.be.vm_adopt(v.units[0], self.progids[key], c, w, self.tstart[g], MSDUR)
            v.mode = "vm"

    def recall(self, vs, g):
        """g: the open fragment, or the next one to be opened.  The states are the ones at the start of it."""
        if not self.on_gpu:
            return
        got = self.be.vm_recall([v.units[0] for v in vs])
        for v, c in zip(vs, got):
            assert v.mode == "vm"
            st = from_ctypes(c)
            want = v.ends[g - 1] if g > v.g0 else v.st0
            assert st.key() == want.key(), f"voice {v.chain} {v.k} ({v.name}) recalled in front of fragment {g}: {diff(st, want)}"
            if g > v.g0:
                _r, host = host_trace(v.words, v.n, v.st0, v.chain, [f for f, _o in self.layout[v.g0:g]],
                                      [o for _f, o in self.layout[v.g0:g]], self.tstart[v.g0])
                assert st.key() == host.key(), f"voice {v.chain} {v.k} ({v.name}): the host interpreter has {diff(st, host)}"
            v.mode = "model"
            self.drive(v, st, g)        # (from what the DEVICE returned)
            self.recalled += 1

    def leaves(self, g, frames):
        be = self.be
        for v in self.voices:
            if v.mode == "vm":
                be.mark_default(v.units)
            elif v.mode == "model":
                w = vp.wires(v.chain)
                for o in v.ops[g]:
                    if o[0] == "p":
                        for u in v.units:
                            be.unit_process(u, o[1], o[2])
                    elif o[2] in w:
                        pos, ureg = w[o[2]]
                        be.unit_write(v.units[pos], ureg, o[3], o[4], o[5], o[6])
            else:
                for u in v.units:
                    be.unit_process(u, 0, frames)
        for units in self.plain:
            for u in units:
                be.unit_process(u, 0, frames)

    def run(self, steps):
        be, root = self.be, self.sc.rootv
        self.lay_out(steps)
        g, is_open, frames, pending = -1, False, 0, 0

        def close():
            nonlocal is_open
            if is_open:
                be.inline_end(root[0])
                be.unit_process(root[1], 0, frames)
                be.unit_process(root[2], 0, frames)
                is_open = False

        for s in steps:
            if s[0] == "open":
                close()
                g, frames, is_open = g + 1, s[1], True
                be.fragment(frames)
                if s[2] and self.on_gpu:
                    be.fragment_offset(s[2])
                be.unit_process(root[0], 0, frames)
                pending += frames
            elif s[0] == "leaves":
                self.leaves(g, frames)
            elif s[0] == "adopt":
                self.adopt(s[1](self) if callable(s[1]) else s[1], g)
            elif s[0] == "recall":
                self.recall(s[1](self) if callable(s[1]) else s[1], g if is_open else g + 1)
            elif s[0] == "write":
                _w, v, pos, ureg, value, dur = s
                v = self.voices[v]
                assert v.mode == "plain"
                be.unit_write(v.units[pos], ureg, value, 0, dur)
            elif s[0] == "pre_ramp":
                for v in self.voices:
                    if v.chain == "filt" and v.k % 2 == 0:
                        be.unit_write(v.units[1], 0, fx(3.5), 0, (40 * 64) << 8)
            elif s[0] == "cuts":
                if self.on_gpu:
                    be.vm_expect_cuts(s[1])
            elif s[0] == "render":
                close()
                a = be.render(pending)
                assert a.shape[1] == pending
                pending = 0
                self.audio.append(a)
                if self.on_gpu:
                    self.infos.append(be.last_batch_vm())
                    self.slabs.append(last_batch(be).win_slabs)
            else:
                raise ValueError(s)
        return self


def diff(a, b):
    out = [f"{n} {getattr(a, n):#x} / {getattr(b, n):#x}" for n in ("waketime", "state", "pc") if getattr(a, n) != getattr(b, n)]
    out += [f"r{i} {x} / {y}" for i, (x, y) in enumerate(zip(a.r, b.r)) if x != y]
    return "; ".join(out) + " (device / expected)"


def all_voices(rig):
    return rig.voices


def still_adopted(rig):
    return [v for v in rig.voices if v.mode == "vm"]


def every(n, first):
    return lambda rig: [v for v in rig.voices if v.k % n == first and v.mode == "vm"]


# the two batches every scene begins with: one by calls; one in whose second fragment every voice is handed over
def prologue(nfr=8, pre_ramp=True, adopt=all_voices):
    return (steps_batch(nfr) + steps_frag() * 1 + ([("pre_ramp",)] if pre_ramp else []) + steps_frag() + [("adopt", adopt)] +
            steps_frag() * (nfr - 2) + [("render",)])


_oracle = {}


def play(oracle_lib, key, chains, steps, settled=0, max_batch=32):
    """the steps on the GPU and - once per key - on the oracle; the audio compared batch by batch; the GPU's rig"""
    be = make_gpu(max_batch=max_batch)
    try:
        rig = Rig(be, True, chains, settled).run(steps)
        ptab = rig.ptab
    finally:
        be.close()
    if key not in _oracle:
        ora = make_oracle(oracle_lib)
        _oracle[key] = Rig(ora, False, chains, settled, ptab).run(steps).audio
        ora.close()
    want = _oracle[key]
    print(f"{key}: last_batch_vm per batch")
    for b, i in enumerate(rig.infos):
        print(f"  {b:2d} {path(i)} quiet {list(i.quiet_launched)} listed {i.listed} {list(i.class_voices)} + {i.other_voices} pending {i.pending} records {i.records} "
              f"idle {list(i.idle) if i.idle_known else None} slabs {rig.slabs[b]}")
    assert len(rig.audio) == len(want)
    loud = 0
    for b, (a, w) in enumerate(zip(rig.audio, want)):
        assert a.shape == w.shape, b
        assert first_diff(a, w) is None, f"batch {b}: (ch, frame, gpu, oracle) = {first_diff(a, w)}"
        loud += int(abs(a).max() > 0)
    assert loud == len(want)
    return rig


def path(i):
    """(fused, not_fused, spec_valid, spec_taken, spec_miss, spec_next, spec_why_not) of a batch"""
    return (i.fused, i.not_fused, i.spec_valid, i.spec_taken, i.spec_miss, i.spec_next, i.spec_why_not)


def counts(rig):
    """(listed, class_voices, other_voices, pending) per batch"""
    return [(i.listed, tuple(i.class_voices), i.other_voices, i.pending) for i in rig.infos]


def of_class(chain, n):
    return tuple(n if c == chain else 0 for c in vp.CLASSES)


def host_records_per_batch(rig, steps, chains=None):
    """records the host interpreter makes for the voices the device VM has, batch by batch (k_vm_count's total)"""
    bounds, g = [], 0
    for s in steps:
        g += s[0] == "open"
        if s[0] == "render":
            bounds.append(g)
    total = [0] * len(bounds)
    for v in rig.voices:
        if v.g0 is None or (chains is not None and v.chain not in chains):
            continue
        recs, _st = host_trace(v.words, v.n, v.st0, v.chain, [f for f, _o in rig.layout[v.g0:]], [o for _f, o in rig.layout[v.g0:]],
                               rig.tstart[v.g0])
        joined = next(b for b, e in enumerate(bounds) if v.g0 < e) + 1     # (the batch of the hand-over is the host's)
        for r in recs:
            gg = v.g0 + r[0]
            b = next(b for b, e in enumerate(bounds) if gg < e)
            if b >= joined:
                total[b] += 1
    return total


def clean_env(monkeypatch, **switches):
    for name in ("A2AMD_NO_FAST", "A2AMD_VPW", "A2AMD_NO_VM", "A2AMD_VMWIN", "A2AMD_VMSPEC", "A2AMD_VMSKIP", "A2AMD_VMSPEC_EARLY",
                 "A2AMD_VMSPEC_GO", "A2AMD_VMSPEC_MIN", "A2AMD_WIN_SLABS", "A2AMD_HOSTTIMING"):
        monkeypatch.delenv(name, raising=False)
    for name, value in switches.items():
        monkeypatch.setenv(name, value)


# the paths, as path() gives them
RECORDS_NO_PREDICTION = (0, 1, 0, 0, 0, 0, 4)   # the first batch on the list: nothing predicted it, the lists are new
RECORDS_NOT_ASKED = (0, NOT_ASKED, 0, 0, 0, 0, 1)
OTHERS_ONLY = (0, 0, 0, 0, 0, 0, 1)             # no class voices: k_vm_count / k_vm_emit, nothing to fuse or to speculate on
FUSED_FIRST = (1, 0, 0, 0, 0, 1, 0)             # k_vm_win (k_vm_pool predicted it), the first pass launched behind it
TAKEN = (1, 0, 1, 1, 0, 1, 0)                   # k_vm_commit, the next pass launched
FUSED_NOSPEC = (1, 0, 0, 0, 0, 0, 1)            # k_vm_win, the speculative pass switched off


# ---- 0. what a2amd_vm_adopt refuses -------------------------------------------------------------
@gpu
def test_registers_r_and_r_plus_32_both_written_are_refused_without_a_look_ahead(monkeypatch):
    """The twin program without its DIVR is one the analysis vouches for as a whole - and a2amd_vm_adopt refuses it: the
    set of registers the tracker may pass on does not cover the twins.  (With the DIVR the voice is taken for a stretch the
    host has run ahead through: every scene below has such voices.)"""
    clean_env(monkeypatch)
    be = make_gpu(max_batch=8)
    sc = synth.Scene(be)
    sc.root()
    sc.add_voices(1, "osc-pan")
    sc.walk(64)
    words, _n = vp.assemble(vp.p_twin("osc", dynamic=False))
    prog = be.vm_program(0x77, list(words))
    st = vp.start_state("osc", "twin", 0, 64)
    c = a2amd_vm_state()
    c.waketime, c.state, c.pc = st.waketime, st.state, st.pc
    w = {r: (sc.leaves[0][pos], ureg) for r, (pos, ureg) in vp.wires("osc").items()}
    rc = be.vm_adopt(sc.leaves[0][0], prog, c, w, 0, MSDUR, check=False)
    msg = be.last_error()
    be.render(64)
    info = be.last_batch_vm()
    be.close()
    assert rc == EUNSUPPORTED and "r + 32" in msg, (rc, msg)
    assert (info.listed, info.pending) == (0, 0)


# ---- 1. records ---------------------------------------------------------------------------------
RECORDS_CASES = [("fm2", {}), ("osc", {"A2AMD_VMWIN": "0"}), ("osc2", {"A2AMD_VMWIN": "0"}), ("filt", {"A2AMD_VMWIN": "0"}),
                 ("osc", {"A2AMD_WIN": "0"}), ("osc2", {"A2AMD_WIN": "0"}), ("filt", {"A2AMD_WIN": "0"})]


@gpu
@pytest.mark.parametrize("chain,switches", RECORDS_CASES, ids=[c + "".join("-" + k[6:] + v for k, v in s.items()) for c, s in RECORDS_CASES])
def test_records_path(oracle_lib, monkeypatch, chain, switches):
    """k_vm_count / k_vm_emit: `fm2; panmix` - the chain outside the window classes - and the three classes with k_vm_win
    or the window kernels switched off.  Six batches; every batch's record count is the host interpreter's; then every
    voice is recalled between two batches and rendered once more from calls.  (No cutoff ramp is left running at the
    hand-over here: a2amd_vm_trace_host_env starts a filter from rest, and its count of coefficient records is compared.)"""
    clean_env(monkeypatch, **switches)
    steps = prologue(pre_ramp=False) + steps_batch() * 6 + [("recall", still_adopted)] + steps_batch()
    rig = play(oracle_lib, ("records", chain), [chain], steps)
    cls, other = (of_class(chain, NV), 0) if chain in vp.CLASSES else ((0, 0, 0), NV)
    assert counts(rig) == [(0, (0, 0, 0), 0, 0), (0, (0, 0, 0), 0, NV)] + [(NV, cls, other, 0)] * 6 + [(0, (0, 0, 0), 0, 0)]
    quiet = (0, 0, 0, 0, 0, 0, 0)
    assert [path(i) for i in rig.infos] == [quiet, quiet] + [OTHERS_ONLY if chain == "fm2" else RECORDS_NOT_ASKED] * 6 + [quiet]
    assert [i.records for i in rig.infos] == host_records_per_batch(rig, steps)[:8] + [0]
    assert min(i.records for i in rig.infos[2:8]) > NV
    assert rig.recalled == NV


# ---- 2. fused -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("chain", vp.CLASSES)
def test_fused(oracle_lib, monkeypatch, chain):
    """k_vm_win<NOSC,FILT> of the batch itself (A2AMD_VMSPEC=0), predicted by k_vm_pool: fused from the first predicted
    batch on.  Voices are recalled between two batches, in fragment 0 of a new batch and in fragment 3 of an open one
    (the host carries them over fragments 0-2) - each time the lists change and that batch goes through records - and
    are driven by calls from the recalled state for the rest of the scene."""
    clean_env(monkeypatch, A2AMD_VMSPEC="0")
    steps = (prologue() + steps_batch() * 3 +
             [("recall", every(7, 1))] +                                                # between batches 4 and 5
             [("open", 64, 0), ("recall", every(7, 3)), ("leaves",)] + steps_frag() * 7 + [("render",)] +      # 5
             steps_frag() * 3 + [("open", 64, 0), ("recall", every(7, 5)), ("leaves",)] + steps_frag() * 4 + [("render",)] +   # 6
             steps_batch() * 2 + [("recall", still_adopted)])
    rig = play(oracle_lib, ("fused", chain), [chain], steps)
    assert [path(i) for i in rig.infos] == [(0, 0, 0, 0, 0, 0, 0)] * 2 + [
        (0, 1, 0, 0, 0, 0, 1),          # 2: on the list, not predicted
        FUSED_NOSPEC, FUSED_NOSPEC,     # 3, 4
        (0, 2, 0, 0, 0, 0, 1),          # 5: other lists than predicted
        (0, 2, 0, 0, 0, 0, 1),          # 6
        FUSED_NOSPEC, FUSED_NOSPEC]     # 7, 8
    assert [i.listed for i in rig.infos] == [0, 0, 70, 70, 70, 50, 40, 40, 40]
    assert rig.infos[2].records > NV and [i.records for i in rig.infos[3:5] + rig.infos[7:]] == [0] * 4
    assert rig.recalled == NV


# ---- 3. speculation taken -------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("switches", [{}, {"A2AMD_VMSKIP": "0"}, {"A2AMD_VMSPEC_EARLY": "0"}, {"A2AMD_VMSPEC_GO": "0"}],
                         ids=["defaults", "VMSKIP0", "EARLY0", "GO0"])
@pytest.mark.parametrize("chain", vp.CLASSES)
def test_speculation_taken(oracle_lib, monkeypatch, chain, switches):
    """The speculative pass (k_vm_win into shadows behind the batch before) and k_vm_commit: eight batches with the
    library's defaults, the pass taken from the second predicted batch on - the first is k_vm_win's, the pass is first
    launched behind it, two batches after the lists were made.  The sleepers are idle in most batches: the pass leaves
    them to the class's quiet kernel (k_leaf_oscpan / k_leaf_osc2pan / k_leaf_oscfiltpan), which is launched."""
    clean_env(monkeypatch, **switches)
    steps = prologue() + steps_batch() * 8 + [("recall", still_adopted)]
    rig = play(oracle_lib, ("spec", chain), [chain], steps)
    assert [path(i) for i in rig.infos] == [(0, 0, 0, 0, 0, 0, 0)] * 2 + [RECORDS_NO_PREDICTION, FUSED_FIRST] + [TAKEN] * 6
    assert counts(rig)[2:] == [(NV, of_class(chain, NV), 0, 0)] * 8
    ci = vp.CLASSES.index(chain)
    assert all(i.idle_known and 0 < i.idle[ci] < NV for i in rig.infos[4:]), [list(i.idle) for i in rig.infos[4:]]
    # ... and the class's quiet kernel, which renders the class voices without a run in the batch, was launched for them
    # (it is not where a taken pass says that it left none: A2AMD_VMSKIP)
    assert [i.quiet_launched[ci] for i in rig.infos[4:]] == [1] * 6
    assert rig.recalled == NV


# ---- 4. announced cuts ----------------------------------------------------------------------------
def when(frame, frac=0x80):
    return (frame << 8) | frac


@gpu
@pytest.mark.parametrize("chain", vp.CLASSES)
def test_announced_cut(oracle_lib, monkeypatch, chain):
    """a2amd_vm_expect_cuts.  One wake time of the root inside the third fragment of batch 5: the pass behind batch 4 is run
    for [64, 64, 23, 41, 64 ...] and batch 5, which comes that way, takes it.  Two wake times inside one fragment of
    batch 7: no plan, no pass behind batch 6; batch 7 - cut twice - is k_vm_win's own."""
    clean_env(monkeypatch)
    b5, b7 = 5 * 512, 7 * 512
    steps = (prologue() + steps_batch() * 2 +
             steps_batch()[:-1] + [("cuts", [when(b5 + 128 + 23)]), ("render",)] +                      # 4
             steps_batch([(64, 0)] * 2 + cut(23) + [(64, 0)] * 5) +                                     # 5
             steps_batch()[:-1] + [("cuts", [when(b7 + 64 + 10), when(b7 + 64 + 40, 0x10)]), ("render",)] +   # 6
             steps_batch([(64, 0), (10, 0), (30, 10), (24, 40)] + [(64, 0)] * 6) +                      # 7
             steps_batch() * 2 + [("recall", still_adopted)])
    rig = play(oracle_lib, ("cuts", chain), [chain], steps)
    assert [path(i) for i in rig.infos] == [(0, 0, 0, 0, 0, 0, 0)] * 2 + [
        RECORDS_NO_PREDICTION, FUSED_FIRST, TAKEN,
        TAKEN,                          # 5: cut where it was announced
        (1, 0, 1, 1, 0, 0, 2),          # 6: taken; two cuts announced inside one fragment of the next: no plan
        FUSED_FIRST,                    # 7: k_vm_win of its own
        TAKEN, TAKEN]
    assert rig.recalled == NV


# ---- 5. mispredictions ----------------------------------------------------------------------------
OTHER_FRAGMENTS = (1, 0, 1, 0, 2, 1, 0)     # fused by the batch's own k_vm_win; the pass: "other fragments"


@gpu
@pytest.mark.parametrize("chain", vp.CLASSES)
def test_mispredicted_lengths(oracle_lib, monkeypatch, chain):
    """Batches that are not the one the pass was run for, by their length - each behind a taken pass, each followed by two
    batches that take passes again (after the batch k_vm_pool's prediction of the odd length costs); the shadows the
    pass wrote leave no trace in the audio or in the states recalled at the end."""
    clean_env(monkeypatch)
    steps = (prologue() + steps_batch() * 3 +
             steps_batch(4) +                                               # 5: four fragments - another length
             steps_batch() * 3 +                                            # 6 (k_vm_pool predicted four), 7, 8
             steps_batch([(64, 0)] * 7 + [(40, 0)]) +                       # 9: 488 frames
             steps_batch() * 3 + [("recall", still_adopted)])               # 10 (predicted: 488), 11, 12
    rig = play(oracle_lib, ("mislen", chain), [chain], steps)
    assert [path(i) for i in rig.infos] == [(0, 0, 0, 0, 0, 0, 0)] * 2 + [
        RECORDS_NO_PREDICTION, FUSED_FIRST, TAKEN,
        (0, 4, 1, 0, 1, 0, 1),          # 5: another length - records; too short for a pass of its own
        (0, 4, 0, 0, 0, 1, 0),          # 6: k_vm_pool predicted 256 frames
        TAKEN, TAKEN,
        (0, 4, 1, 0, 1, 0, 2),          # 9: 488 frames; no plan for what follows
        (0, 4, 0, 0, 0, 1, 0),          # 10
        TAKEN, TAKEN]
    assert rig.recalled == NV


@gpu
@pytest.mark.parametrize("chain", vp.CLASSES)
def test_mispredicted_cuts(oracle_lib, monkeypatch, chain):
    """... and by where its fragments are cut: a cut nobody announced, an announced cut that does not come, a fragment
    that comes as 48 + 16 frames.  The batch's span is the predicted one, so its own k_vm_win runs the VMs; each is
    followed by two batches that take passes again."""
    clean_env(monkeypatch)
    steps = (prologue() + steps_batch() * 3 +
             steps_batch([(64, 0)] * 3 + cut(37) + [(64, 0)] * 4) +         # 5: a cut nobody announced
             steps_batch() +                                                # 6
             steps_batch()[:-1] + [("cuts", [when(8 * 512 + 64 + 17)]), ("render",)] +      # 7: announces a cut in 8
             steps_batch() * 3 +                                            # 8: comes uncut; 9, 10
             steps_batch([(48, 0), (16, 48)] + [(64, 0)] * 7) +             # 11: 48 + 16, pieces of one fragment
             steps_batch() * 2 + [("recall", still_adopted)])               # 12, 13
    rig = play(oracle_lib, ("miscut", chain), [chain], steps)
    assert [path(i) for i in rig.infos] == [(0, 0, 0, 0, 0, 0, 0)] * 2 + [
        RECORDS_NO_PREDICTION, FUSED_FIRST, TAKEN,
        OTHER_FRAGMENTS, TAKEN, TAKEN,  # 5 - 7
        OTHER_FRAGMENTS, TAKEN, TAKEN,  # 8: announced, not cut
        OTHER_FRAGMENTS, TAKEN, TAKEN]  # 11
    assert rig.recalled == NV


@gpu
@pytest.mark.parametrize("chain", vp.CLASSES)
def test_mispredicted_lists(oracle_lib, monkeypatch, chain):
    """... and by what happens to the voices between the pass and the batch: a voice recalled, a host write to a voice of
    the scene that is not adopted (the last one: handed over late), that voice adopted in a batch that has a pass."""
    clean_env(monkeypatch)
    late = lambda rig: [rig.voices[NV - 1]]
    steps = (prologue(adopt=lambda rig: rig.voices[:NV - 1]) + steps_batch() * 3 +
             [("recall", lambda rig: [rig.voices[12]])] + steps_batch() * 4 +             # 5: the lists changed; 6, 7, 8
             [("write", NV - 1, len(vp.CHAINS[chain][1]) - 1, 1, fx(-.7), 300 << 8)] + steps_batch() * 3 +      # 9, 10, 11
             steps_frag() * 2 + [("adopt", late)] + steps_frag() * 6 + [("render",)] +      # 12: one more voice
             steps_batch() * 4 + [("recall", still_adopted)])                               # 13 (new lists), 14, 15, 16
    rig = play(oracle_lib, ("mislist", chain), [chain], steps)
    other_lists = (0, 2, 1, 0, 1, 0, 4)         # records; the lists are new: no pass behind it either
    assert [path(i) for i in rig.infos] == [(0, 0, 0, 0, 0, 0, 0)] * 2 + [
        RECORDS_NO_PREDICTION, FUSED_FIRST, TAKEN,
        other_lists, FUSED_FIRST, TAKEN, TAKEN,             # 5 - 8
        TAKEN, TAKEN, TAKEN,                                # 9 - 11: the write touches no list of the VM's
        TAKEN,                                              # 12: the new voice is the host's for this batch
        other_lists, FUSED_FIRST, TAKEN, TAKEN]             # 13 - 16
    assert [i.listed for i in rig.infos] == [0, 0] + [69] * 3 + [68] * 8 + [69] * 4
    assert [i.pending for i in rig.infos] == [0, 69] + [0] * 10 + [1] + [0] * 4
    assert rig.recalled == NV


# ---- 6. slabs -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("spec", ["1", "0"])
@pytest.mark.parametrize("chain", vp.CLASSES)
def test_slabs(oracle_lib, monkeypatch, chain, spec):
    """Batches of 16 fragments in four slabs (A2AMD_WIN_SLABS=4): k_vm_win entered once per slab, from the second on with
    the state the slab before left (fa > 0).  With the speculative pass a taken batch is one piece."""
    clean_env(monkeypatch, A2AMD_WIN_SLABS="4", A2AMD_VMSPEC=spec)
    steps = prologue(16) + steps_batch(16) * 5 + [("recall", still_adopted)]
    rig = play(oracle_lib, ("slabs", chain), [chain], steps)
    if spec == "1":
        assert [path(i) for i in rig.infos] == [(0, 0, 0, 0, 0, 0, 0)] * 2 + [RECORDS_NO_PREDICTION, FUSED_FIRST] + [TAKEN] * 3
        assert rig.slabs[2:] == [4, 4, 1, 1, 1]
    else:
        assert [path(i) for i in rig.infos] == [(0, 0, 0, 0, 0, 0, 0)] * 2 + [(0, 1, 0, 0, 0, 0, 1)] + [FUSED_NOSPEC] * 4
        assert rig.slabs[2:] == [4] * 5
    assert rig.recalled == NV


# ---- 7. mixed -------------------------------------------------------------------------------------
@gpu
def test_mixed(oracle_lib, monkeypatch):
    """All four chains in one context beside 200 settled `wtosc; panmix` voices that are not adopted: the quiet kernels,
    k_vm_win / k_vm_commit of every class, k_vm_count / k_vm_emit and the general kernel share the batches.  (As in
    test_records_path no cutoff ramp is left running at the hand-over: the record counts are compared.)"""
    clean_env(monkeypatch)
    chains = ["osc", "osc2", "filt", "fm2"]
    steps = prologue(pre_ramp=False) + steps_batch() * 6 + [("recall", still_adopted)]
    rig = play(oracle_lib, ("mixed",), chains, steps, settled=200)
    assert counts(rig) == [(0, (0, 0, 0), 0, 0), (0, (0, 0, 0), 0, 4 * NV)] + [(4 * NV, (NV, NV, NV), NV, 0)] * 6
    assert [path(i) for i in rig.infos] == [(0, 0, 0, 0, 0, 0, 0)] * 2 + [RECORDS_NO_PREDICTION, FUSED_FIRST] + [TAKEN] * 4
    want = host_records_per_batch(rig, steps)
    fm2 = host_records_per_batch(rig, steps, ["fm2"])
    assert [i.records for i in rig.infos] == want[:3] + fm2[3:]
    assert rig.recalled == 4 * NV
