#!/usr/bin/env python3
"""Writes tests/golden/wavepost_cases.npz: what the compiled reference (oracle/_ref/libaudiality2.so) makes of
waves that are written the way a2_RenderWave writes them - a2_NewWave(type, period, flags), a2_OpenStream, one
a2_Write(A2_I24) per chunk, a2_Release of the stream - with "normalize" and / or "xfade" set.  Run once, where
the reference is built; tests/test_wavepost.py compares a2amd_wavepost_host() and synth.wave_postprocess()
with the file.

The file holds four arrays: `names`; `meta` (one row per case: samples, chunk, flags, wave type); `pcm` (int32,
the cases' samples one after the other) and `expect` (int16, the cases' level 0 WITH its pads, A2_WAVEPRE before
and A2_WAVEPOST after, one after the other).  All samples stay inside 24 bits.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiality2_amd.synth import LOOPED, NORMALIZE, XFADE, WWAVE, WMIPWAVE  # noqa: E402
from audiality2_amd.replay import WAVEPRE, WAVEPOST, MIPLEVELS              # noqa: E402

A2_AUDIODRIVER, A2_AUTOCLOSE, A2_REALTIME, A2_I24 = 2, 0x20000000, 0x800, 2
N, X, L = NORMALIZE, XFADE, LOOPED


class A2_wave(C.Structure):     # include/a2_waves.h:95-103
    _fields_ = [("type", C.c_int), ("flags", C.c_uint), ("period", C.c_uint),
                ("data", C.POINTER(C.c_int16) * MIPLEVELS), ("size", C.c_uint * MIPLEVELS)]


def signal(rng, n, peak):
    """a few partials and some noise, scaled so that the largest magnitude is exactly `peak`"""
    t = np.arange(n)
    s = sum(rng.uniform(.2, 1) * np.sin(t * rng.uniform(.01, .4) + rng.uniform(0, 6.28)) for _ in range(4))
    s = s + rng.uniform(-.3, .3, n)
    if not n or not np.abs(s).max():
        return np.zeros(n, dtype=np.int32)
    x = np.trunc(s / np.abs(s).max() * peak).astype(np.int32)
    return x


def cases():
    rng = np.random.default_rng(20240607)
    out = []

    def add(name, x, chunk, flags, wtype=WWAVE):
        x = np.asarray(x, dtype=np.int32)
        assert len(x) <= 3000 and (not len(x) or np.abs(x.astype(np.int64)).max() < 1 << 23)
        out.append((name, x, chunk, flags, wtype))

    # normalize: the peak in the middle chunk (the other chunks stay below it)
    x = signal(rng, 700, 1500000)
    x[256:512] = signal(rng, 256, 3000017)
    add("normalize_peak_in_the_middle_chunk", x, 256, N)
    # ... in the last, short chunk (600 = 2 * 256 + 88)
    x = signal(rng, 600, 900000)
    x[512:] = signal(rng, 88, 2222221)
    add("normalize_peak_in_the_last_short_chunk", x, 256, N)
    # a quiet signal with one silent chunk: that chunk's gain of 1 is the smallest, nothing is amplified
    x = signal(rng, 768, 40000)
    x[256:512] = 0
    add("normalize_quiet_with_a_silent_chunk", x, 256, N)
    # peak below 8389: 8388352 / peak is above 1000, the cap
    add("normalize_gain_capped_at_1000", signal(rng, 300, 5000), 100, N)
    # one negative sample beyond every positive one
    x = signal(rng, 500, 1000000)
    x[x < -900000] = -900000
    x[301] = -4194301
    add("normalize_negative_peak", x, 256, N)
    add("normalize_all_silent", np.zeros(300, dtype=np.int32), 256, N | X)
    # loud: a gain below 1
    add("normalize_attenuates", signal(rng, 400, 8388607), 256, N)
    add("xfade_even", signal(rng, 512, 6000000), 256, X)
    add("xfade_odd", signal(rng, 733, 7000000), 256, X | L)
    add("xfade_two_samples", [5000000, -3000000], 256, X)
    add("xfade_three_samples", [5000000, -3000000, 7654321], 256, X | L)
    add("normalize_xfade_looped_mipwave", signal(rng, 733, 2500000), 256, N | X | L, WMIPWAVE)
    add("normalize_xfade_looped_long", signal(rng, 1500, 123457), 256, N | X | L)
    add("normalize_chunk_100", signal(rng, 450, 3100000), 100, N)
    add("normalize_xfade_chunk_1", signal(rng, 130, 4000000), 1, N | X)
    add("normalize_chunk_larger_than_the_wave", signal(rng, 200, 777777), 256, N | X)
    return out


def main():
    ref = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libaudiality2.so"))
    vp = C.c_void_p
    for name, res, args in (("a2_NewDriver", vp, [C.c_int, C.c_char_p]), ("a2_OpenConfig", vp, [C.c_int] * 4),
                            ("a2_AddDriver", C.c_int, [vp, vp]), ("a2_OpenVersion", vp, [vp, C.c_uint]), ("a2_LinkedVersion", C.c_uint, []),
                            ("a2_Close", None, [vp]),
                            ("a2_NewWave", C.c_int, [vp, C.c_int, C.c_uint, C.c_int]),
                            ("a2_OpenStream", C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_uint]),
                            ("a2_Write", C.c_int, [vp, C.c_int, C.c_int, vp, C.c_uint]),
                            ("a2_GetWave", C.POINTER(A2_wave), [vp, C.c_int])):
        f = getattr(ref, name)
        f.restype, f.argtypes = res, args
    drv = ref.a2_NewDriver(A2_AUDIODRIVER, b"buffer")
    # (A2_REALTIME: the interface of any other state has no Release, src/interface.c:496-505, 932-935)
    cfg = ref.a2_OpenConfig(48000, 64, 2, A2_AUTOCLOSE | A2_REALTIME)
    assert drv and cfg and ref.a2_AddDriver(cfg, drv) == 0
    iface = ref.a2_OpenVersion(cfg, ref.a2_LinkedVersion())     # (a2_Open() is an inline of the header)
    assert iface
    # a2_Release() is an inline of the header too: the first member of A2_interface (include/a2_interface.h:39-42)
    release = C.CFUNCTYPE(C.c_int, vp, C.c_int)(C.cast(iface, C.POINTER(vp))[0])
    names, meta, pcm, expect = [], [], [], []
    for name, x, chunk, flags, wtype in cases():
        wh = ref.a2_NewWave(iface, wtype, 64, flags)
        assert wh >= 0
        sh = ref.a2_OpenStream(iface, wh, 0, 0, 0)
        assert sh >= 0
        for lo in range(0, len(x), chunk):
            part = np.ascontiguousarray(x[lo:lo + chunk])
            assert ref.a2_Write(iface, sh, A2_I24, part.ctypes.data, part.nbytes) == 0
        assert release(iface, sh) == 0
        w = ref.a2_GetWave(iface, wh).contents
        assert w.size[0] == len(x) and w.flags == flags, (name, w.size[0], hex(w.flags))
        lvl0 = np.ctypeslib.as_array(w.data[0], shape=(WAVEPRE + len(x) + WAVEPOST,)).copy()
        release(iface, wh)
        names.append(name)
        meta.append((len(x), chunk, flags, wtype))
        pcm.append(x)
        expect.append(lvl0)
        print(f"{name}: {len(x)} samples, chunk {chunk}, flags {flags:#x}, peak in {int(np.abs(x).max()) if len(x) else 0}, "
              f"out {int(np.abs(lvl0.astype(np.int32)).max())}")
    ref.a2_Close(iface)
    path = os.path.join(ROOT, "tests", "golden", "wavepost_cases.npz")
    np.savez_compressed(path, names=np.array(names), meta=np.array(meta, dtype=np.int64),
                        pcm=np.concatenate(pcm).astype(np.int32), expect=np.concatenate(expect).astype(np.int16))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
