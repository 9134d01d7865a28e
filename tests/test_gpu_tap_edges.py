"""The wavetable taps at the edges of their arithmetic (audiality2_amd/csrc/a2amd_taps.h: hermite_step, inter_coefs,
tap_phase), bit for bit against the CPU oracle: waves whose Hermite coefficients reach their extremes, the largest and
the smallest phase increment the settled paths take, an increment whose lane multiples cross the 16 bit carry inside
a fragment, phases whose fraction byte is 0 and 255 at the start of the first fragment the settled kernels render (the
birth fragment goes through the records kernels; the start phases allow for its 64 frames).  The largest-increment
and the carry voices sweep every fraction byte along the lanes besides.

70 voices (two wavefronts' worth at the smallest voices per wavefront, the second partly filled), a birth fragment,
then two batches of 5 fragments (a chunk of 4 and a remainder) rendered by the settled leaf kernels; one voice glides
in pitch through both, so the window kernels (forced by conftest) and the still-moving path run too."""
import ctypes

import numpy as np
import pytest

from audiality2_amd import synth
from audiality2_amd.replay import MIPLEVELS
from conftest import fnv1a_fragments, make_gpu, make_oracle

pytestmark = pytest.mark.gpu

NVOICES, BFRAGS = 70, 5
MAXPHINC = 512                      # A2_MAXPHINC (a2amd_device.h: A2D_MAXPHINC)


def edge_waves():
    """(samples, period): a full-scale square at the sample rate, a full-scale impulse in silence"""
    square = np.where(np.arange(2048) & 1, -32768, 32767).astype(np.int16)
    impulse = np.zeros(1500, dtype=np.int16)
    impulse[700] = 32767
    # (an odd period: phase = ph * period << 8 then reaches every fraction byte; 2048 reaches multiples of 8 only)
    return [(square, 2047), (impulse, 1500)]


class Pitches:
    """Total pitches (16:16 octaves, basepitch included) by what they make of the phase increment, found with the
    oracle's own pitch table and a2_P2I (oracle/a2o.c: a2o_build_pitch_table, a2o_p2i)."""

    def __init__(self, oracle_lib):
        self.tab = (ctypes.c_uint32 * 128)()
        oracle_lib.a2o_build_pitch_table(self.tab)
        oracle_lib.a2o_p2i.restype = ctypes.c_uint
        self.p2i = lambda pitch: int(oracle_lib.a2o_p2i(self.tab, ctypes.c_int(pitch)))

    def dph(self, pitch, period):
        """(dph, mip level) of wtosc_wavetable (wtosc.c:239-258)"""
        dphase = self.p2i(pitch)
        d8, mm = ((dphase + 255) >> 8) * period, 0
        while d8 > (MAXPHINC << 8) and mm < MIPLEVELS - 1:
            d8 >>= 1
            mm += 1
        return (dphase * period) >> mm, mm

    def largest(self, period):
        """the highest pitch that stays on mip level 0: the largest dph the settled paths take for this period"""
        lo, hi = -24 << 16, 0                                   # (dphase rises with the pitch in this range)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if ((self.p2i(mid) + 255) >> 8) * period <= (MAXPHINC << 8):
                lo = mid
            else:
                hi = mid
        return lo

    smallest = -24 << 16                                        # dphase = 1: dph = the wave's period
    carry = (-23 << 16) + int(0.6 * 65536)                      # dphase = 3: lane * dph crosses 2^16 every ~11 lanes


def phase_for_byte(period, byte, dph):
    """a 16:16 start phase ph (wtosc_set_phase: phase = ph * period << 8) that, 64 frames of dph on, has fraction byte
    `byte` in the 24:8 tap phase - or the nearest byte that this period reaches (2048: steps of 8)"""
    ph = np.arange(65536, dtype=np.int64)
    got = ((((ph * period) << 8) + 64 * dph) >> 16) & 0xFF
    for b in sorted(range(256), key=lambda b: abs(b - byte)):
        hit = np.nonzero(got == b)[0]
        if len(hit):
            return int(hit[0])
    raise AssertionError((period, byte))


def build_and_run(be, chain, pit, basepitch):
    sc = synth.Scene(be, nwaves=1)
    sc.root()
    waves = []
    for i, (w, period) in enumerate(edge_waves()):
        sizes, data = synth.wave_pyramid(w)
        waves.append((be.wave_upload(0x700 + i, synth.WMIPWAVE, synth.LOOPED, period,
                                     sizes + [0] * (MIPLEVELS - len(sizes)), data), period))
    waves.append((sc.wave_ids[0], synth.WAVEPERIOD))            # one built-in wave (period 2048: dph = 2^25 exactly)
    sc.add_voices(NVOICES, chain=chain, total=NVOICES)
    for k, units in enumerate(sc.leaves):
        for j, o in enumerate(units[:-1]):
            wid, period = waves[(k + j) % 3]
            kind = (k // 3 + j) % 3
            total = (pit.largest(period), pit.smallest, pit.carry)[kind]
            byte = (0, 255)[(k // 9 + j) % 2]
            be.unit_write(o, 0, wid)
            be.unit_write(o, 1, total - basepitch)
            be.unit_write(o, 2, synth.fix(0.25))
            be.unit_write(o, 3, phase_for_byte(period, byte, pit.dph(total, period)[0]))
    glider = sc.leaves[5]
    for o in glider[:-1]:
        be.unit_write(o, 1, synth.fix(-0.5))
    parts = [sc.run(1, batch=1)]                                # births: the records kernels
    be.unit_write(glider[0], 1, synth.fix(0.75), 0, 500 << 8)   # a glide over fragments 1 .. 8
    parts.append(sc.run(BFRAGS, batch=BFRAGS))
    parts.append(sc.run(BFRAGS, batch=BFRAGS))
    return np.concatenate(parts, axis=1)


@pytest.fixture(scope="module")
def pitches(oracle_lib):
    pit = Pitches(oracle_lib)
    # what the scene is built for, checked on the oracle's own table
    assert pit.dph(pit.largest(synth.WAVEPERIOD), synth.WAVEPERIOD) == (MAXPHINC << 16, 0)
    for _, period in edge_waves():
        d, mm = pit.dph(pit.largest(period), period)
        assert mm == 0 and (MAXPHINC << 16) - 2 * period * 256 < d <= (MAXPHINC << 16)
        assert pit.dph(pit.largest(period) + 1, period)[1] == 1     # one step up the next mip level takes over
    assert pit.p2i(pit.smallest) == 1
    assert pit.p2i(pit.carry) == 3
    # ... and that writing `total - basepitch` to an oscillator's pitch register makes p2i(total) of it: the impulse
    # (sample 700) comes out where a phase advancing by dph(total) per frame reaches it, at two pitches an octave apart
    impulse, period = edge_waves()[1]
    for total, frags in ((pit.largest(period), 8), (pit.largest(period) - 65536, 12)):
        ora = make_oracle(oracle_lib)
        sc = synth.Scene(ora, nwaves=1)
        sc.root()
        sizes, data = synth.wave_pyramid(impulse)
        wid = ora.wave_upload(0x700, synth.WMIPWAVE, synth.LOOPED, period, sizes + [0] * (MIPLEVELS - len(sizes)), data)
        sc.add_voices(1, chain="osc-pan", total=1)
        osc = sc.leaves[0][0]
        ora.unit_write(osc, 0, wid)
        ora.unit_write(osc, 1, total - synth.basepitch_for(48000))
        ora.unit_write(osc, 2, synth.fix(0.25))
        ora.unit_write(osc, 3, 0)
        out = sc.run(frags, batch=frags)
        ora.close()
        peak = int(np.argmax(np.abs(out[0])))
        assert abs(peak - 700.0 * (1 << 24) / pit.dph(total, period)[0]) <= 3, (total, peak)
    return pit


@pytest.fixture(scope="module")
def oracle_audio(oracle_lib, pitches):
    out = {}
    for chain in ("osc-pan", "osc2-pan"):
        ora = make_oracle(oracle_lib)
        out[chain] = build_and_run(ora, chain, pitches, synth.basepitch_for(48000))
        ora.close()
    return out


@pytest.mark.parametrize("chain", ["osc-pan", "osc2-pan"])
def test_tap_edges_match_oracle(oracle_audio, pitches, chain):
    want = oracle_audio[chain]
    assert want.shape[1] == (1 + 2 * BFRAGS) * 64 and want.any()
    gpu = make_gpu(max_batch=8)
    got = build_and_run(gpu, chain, pitches, synth.basepitch_for(48000))
    gpu.close()
    bad = np.nonzero(fnv1a_fragments(got) != fnv1a_fragments(want))[0]
    assert not len(bad), f"fragments differing from the oracle: {bad.tolist()}"
