"""The state commit behind the time-sliced quiet leaf kernels (k_leaf_oscpan, k_leaf_osc2pan; a2amd_fast.hip).

A time-sliced launch cannot write a voice's end state where the other slices still read its start state: it stages
it, says per list entry WHAT it staged (A2DCommit::staged - nothing for a voice that carried records, the oscillators'
phases for a settled voice, every word for a voice with something still moving), and a commit that rides in
k_bus_driver's launch (or k_commit_oscpan on its own) copies exactly that.  A phase, or a ramper, that does not make
it from one batch into the next shows in the next batch: every case renders several batches and is compared with the
oracle batch by batch, bit for bit.

Every scene: 70 osc2-pan and 70 osc-pan voices - no multiple of any voices-per-wavefront count, the last wavefront
of each launch is part-filled - under the root and under one delay group (two buses per launch list), with 4 and 32
voices per wavefront and 1 (no staging at all), 2 and 16 time slices asked for (a batch of 16 fragments has 2 chunks
for k_leaf_oscpan and 4 for k_leaf_osc2pan: that many slices at the most)."""
import numpy as np
import pytest

from audiality2_amd import synth
from conftest import make_gpu, make_oracle
from test_gpu_parity import _async_steps, _oracle_fragments

pytestmark = pytest.mark.gpu

SHAPES = [(vpw, ysplit) for vpw in (4, 32) for ysplit in (1, 2, 16)]
B = 16              # fragments per batch on the graph path (a graph needs 8 at least: a2amd_render.cpp)
_REF = {}           # the oracle's render of a scene, made once and shared by the scene's shape cases (read only)


def _shape(monkeypatch, vpw, ysplit):
    monkeypatch.setenv("A2AMD_VPW", str(vpw))
    monkeypatch.setenv("A2AMD_YSPLIT", str(ysplit))


def _ref(key, make):
    if key not in _REF:
        _REF[key] = make()
        _REF[key].setflags(write=False)
    return _REF[key]


def _scene(be, group=None, private=None):
    """70 + 70 voices, both classes on both buses"""
    sc = synth.Scene(be)
    sc.root()
    if private:
        sc.private_waves(5, length=private, period=256)
    g = sc.add_group(**(group or dict(preset="fmtest4")))
    sc.add_voices(40, chain="osc2-pan", group=g, total=256, private=bool(private))
    sc.add_voices(30, chain="osc-pan", group=g, total=256, private=bool(private))
    sc.add_voices(30, chain="osc2-pan", total=256, private=bool(private))
    sc.add_voices(40, chain="osc-pan", total=256, private=bool(private))
    return sc


def _all_leaves(sc):
    return [u for g in sc.groups for u in g["leaves"]] + list(sc.leaves)


def _assert_batches_equal(got, want, starts):
    """starts: the first frame of every batch, and the end"""
    assert got.shape == want.shape
    for b in range(len(starts) - 1):
        a, w = got[:, starts[b]:starts[b + 1]], want[:, starts[b]:starts[b + 1]]
        if not np.array_equal(a, w):
            ch, fr = [int(x[0]) for x in np.nonzero(a != w)]
            pytest.fail(f"batch {b} differs from the oracle: first at channel {ch}, frame {fr} of the batch "
                        f"(gpu {int(a[ch, fr])}, oracle {int(w[ch, fr])}); "
                        f"{int((a != w).any(axis=0).sum())} of its {a.shape[1]} frames differ")


def _walked(be, build, plan, between=None):
    """plan: per batch the list of its fragments' lengths; every fragment walked, a render per batch.
    between(sc, batch, fragment) runs in front of every fragment's walk."""
    sc = build(be)
    outs = []
    for b, frags in enumerate(plan):
        for f, n in enumerate(frags):
            if between:
                between(sc, b, f)
            sc.walk(n)
        outs.append(be.render(sum(frags)).copy())
    be.close()
    return np.concatenate(outs, axis=1)


def _starts(plan):
    return [0] + list(np.cumsum([sum(frags) for frags in plan]))


@pytest.mark.parametrize("vpw,ysplit", SHAPES)
def test_settled_batches_on_the_graph_path(oracle_lib, monkeypatch, vpw, ysplit):
    """Four identical quiet batches of 16 fragments through fragment_repeat / render(ASYNC) / collect: the second one
    builds the graph, the third and fourth replay it.  Every voice is settled in every batch: phases only."""
    _shape(monkeypatch, vpw, ysplit)
    gpu = make_gpu(max_batch=B)
    got = _async_steps(gpu, _scene(gpu), 4, B)
    gpu.close()
    want = _ref("settled", lambda: _oracle_fragments(oracle_lib, _scene, 4 * B))
    _assert_batches_equal(got, want, [k * B * 64 for k in range(5)])


@pytest.mark.parametrize("frames", ["64", "64-and-37"])
@pytest.mark.parametrize("vpw,ysplit", SHAPES)
def test_settled_batches_of_direct_launches(oracle_lib, monkeypatch, vpw, ysplit, frames):
    """The same in batches of 4 fragments - too short for a graph: direct launches - of 64 frames, and with fragments
    of 37 frames among them."""
    _shape(monkeypatch, vpw, ysplit)
    plan = [[64] * 4] * 4 if frames == "64" else [[64, 37, 64, 64], [37, 64, 64, 37], [64, 64, 37, 64], [37, 37, 64, 64]]
    got = _walked(make_gpu(max_batch=4), _scene, plan)
    want = _ref(("direct", frames), lambda: _walked(make_oracle(oracle_lib), _scene, plan))
    _assert_batches_equal(got, want, _starts(plan))


@pytest.mark.parametrize("vpw,ysplit", SHAPES)
def test_settled_time_sliced_batches_of_direct_launches(oracle_lib, monkeypatch, vpw, ysplit):
    """... and direct launches that ARE time-sliced (a batch of 4 fragments is one chunk, one slice): batches of 16
    fragments, 37-frame ones among them, with the graphs switched off - the commit rides in k_bus_driver's direct
    launch."""
    _shape(monkeypatch, vpw, ysplit)
    monkeypatch.setenv("A2AMD_NO_GRAPH", "1")
    plan = [[37 if (3 * b + f) % 5 == 2 else 64 for f in range(B)] for b in range(3)]
    got = _walked(make_gpu(max_batch=B), _scene, plan)
    want = _ref("direct-sliced", lambda: _walked(make_oracle(oracle_lib), _scene, plan))
    _assert_batches_equal(got, want, _starts(plan))


def _mixed_build(be):
    """Of every five voices in a row - a wavefront of 4 or 32 voices holds every kind - two stay settled, one fades
    and one sweeps its pan (ramps of 1500 frames end inside the second batch of 1024, those of 2500 inside the third:
    staged whole while they last, phases only after), and one is written to in the third batch."""
    sc = _scene(be)
    for k, units in enumerate(_all_leaves(sc)):
        frames = 1500 if k % 2 else 2500
        if k % 5 == 2:
            be.unit_write(units[k % (len(units) - 1)], 2, synth.fix(0.0007 * (1 + k % 3)), 0, frames << 8)    # fade
        if k % 5 == 3:
            be.unit_write(units[-1], 1, synth.fix(((k % 9) - 4) / 5.0), 0, frames << 8)                       # pan sweep
    return sc


def _mixed_writes(sc, b, f):
    """the third batch's writes, in front of its sixth fragment: those voices carry records in that batch - neither the
    quiet kernel nor the commit touches them - and are the quiet kernel's again after (a jump: settled at once; a
    glide of 2000 frames: staged whole for two more batches)"""
    if (b, f) != (2, 5):
        return
    for k, units in enumerate(_all_leaves(sc)):
        if k % 10 == 4:
            sc.be.unit_write(units[-1], 1, synth.fix(((k % 7) - 3) / 4.0))                                    # pan jumps
        if k % 10 == 9:
            sc.be.unit_write(units[0], 2, synth.fix(0.0009), 0, 2000 << 8)                                    # amplitude glides


@pytest.mark.parametrize("vpw,ysplit", SHAPES)
def test_settled_moving_and_written_voices_in_one_wavefront(oracle_lib, monkeypatch, vpw, ysplit):
    """Six batches of 16 fragments in which a wavefront's voices are of every kind the commit tells apart."""
    _shape(monkeypatch, vpw, ysplit)
    plan = [[64] * B] * 6
    got = _walked(make_gpu(max_batch=B), _mixed_build, plan, _mixed_writes)
    want = _ref("mixed", lambda: _walked(make_oracle(oracle_lib), _mixed_build, plan, _mixed_writes))
    _assert_batches_equal(got, want, _starts(plan))


@pytest.mark.parametrize("vpw,ysplit", SHAPES)
def test_settled_voices_on_waves_of_odd_sizes(oracle_lib, monkeypatch, vpw, ysplit):
    """Private waves of 3001 samples: no mip level's size (3001, 1501, 751 ...) is a power of two, the base phase of a
    chunk takes wrap_phase's branch and the phase that is committed is what that branch left."""
    _shape(monkeypatch, vpw, ysplit)

    def build(be):
        return _scene(be, private=3001)
    gpu = make_gpu(max_batch=B)
    got = _async_steps(gpu, build(gpu), 4, B)
    gpu.close()
    want = _ref("odd", lambda: _oracle_fragments(oracle_lib, build, 4 * B))
    _assert_batches_equal(got, want, [k * B * 64 for k in range(5)])


# delay taps in ms at 48 kHz: 2.0 ms = 96 frames - rounds of one fragment; 4.5 ms = 216 frames - rounds of three, the
# batch's last round a single fragment; 63.1 ms = 3028 frames - the batch of 16 fragments is one round
ROUNDS = {1: (2.0, 2.2, 2.5), 3: (4.5, 5.0, 5.2), "batch": (63.1, 75.6, 100.4)}


@pytest.mark.parametrize("delays", [2, 4])
@pytest.mark.parametrize("rounds", [1, 3, "batch"])
@pytest.mark.parametrize("vpw,ysplit", SHAPES)
def test_delay_chain_rounds_behind_the_leaves(oracle_lib, monkeypatch, vpw, ysplit, rounds, delays):
    """k_bus_fbdchain between the leaf kernels and the launch the commit rides in: a chain of two and of four delays
    (the ones in the middle adding) whose shortest tap allows rounds of 1 and of 3 fragments and the whole batch."""
    _shape(monkeypatch, vpw, ysplit)
    # (the later delays of the chain have longer taps: the first one's shortest tap sets the round)
    group = dict(fb=[tuple(t * (1 + 0.37 * i) for t in ROUNDS[rounds]) for i in range(delays)],
                 gains=(0.3, 0.25, 0.25), delays=delays, mid_add=True)

    def build(be):
        return _scene(be, group=group)
    gpu = make_gpu(max_batch=B)
    got = _async_steps(gpu, build(gpu), 4, B)
    bi = gpu.last_batch_buses()
    gpu.close()
    assert (bi.fbd_voices, bi.driver_voices, bi.generic_voices) == (1, 1, 0), "the chain did not reach k_bus_fbdchain"
    want = _ref(("rounds", rounds, delays), lambda: _oracle_fragments(oracle_lib, build, 4 * B))
    _assert_batches_equal(got, want, [k * B * 64 for k in range(5)])
