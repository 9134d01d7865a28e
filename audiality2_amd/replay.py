"""Call-trace reader and replayer.

A trace is the ordered list of calls the Audiality 2 engine made through its
unit plugin surface (Initialize / write / Process / Deinitialize, see
include/a2amd.h) while rendering a script, captured from the unmodified
reference (see tests/golden/).  Replaying it against a library that exports the
call protocol of include/a2amd.h under some symbol prefix ("a2amd_" = the GPU
library) must reproduce the audio the reference rendered.

Format (little endian): int32 records of 8 words {op,a,b,c,d,e,f,g}; a WAVE
record is followed by uint32 size[10] and the int16 payload of every level
(pads included), each level padded to a multiple of 4 bytes.
"""
import ctypes as C
import gzip
import lzma

import numpy as np

T_FRAGMENT, T_INIT, T_DEINIT, T_WRITE, T_PROCESS, T_INLINE_END, T_WAVE, T_CONFIG, T_WAVEDROP = range(1, 10)
MIPLEVELS = 10
WAVEPRE = 1
WAVEPOST = 131


class Trace:
    """Parsed trace: .config dict, .records (list of tuples), .waves."""

    def __init__(self, path):
        opener = gzip.open if str(path).endswith(".gz") else lzma.open if str(path).endswith(".xz") else open
        with opener(path, "rb") as f:
            raw = f.read()
        words = np.frombuffer(raw[: len(raw) // 4 * 4], dtype="<i4")
        self.records = []
        self.waves = {}
        self.config = None
        i = 0
        n = len(words)
        while i + 8 <= n:
            r = tuple(int(x) for x in words[i : i + 8])
            i += 8
            op = r[0]
            if op == T_WAVE:
                wid, wtype, flags, period, levels = r[1:6]
                sizes = words[i : i + MIPLEVELS].astype(np.uint32)
                i += MIPLEVELS
                data = []
                for lv in range(levels):
                    cnt = WAVEPRE + int(sizes[lv]) + WAVEPOST
                    nw = (cnt + 1) // 2
                    d = words[i : i + nw].view("<i2")[:cnt].copy()
                    i += nw
                    data.append(d)
                self.waves[wid] = dict(type=wtype, flags=flags & 0xFFFFFFFF, period=period,
                                       sizes=[int(s) for s in sizes], data=data)
                self.records.append((T_WAVE, wid, 0, 0, 0, 0, 0, 0))
            elif op == T_CONFIG:
                self.config = dict(samplerate=r[1], basepitch=r[2], channels=r[3],
                                   buffer=r[4], noiseseed=r[5] & 0xFFFFFFFF)
            else:
                self.records.append(r)
        if self.config is None:
            raise ValueError("trace without CONFIG record")
        self.kinds = {r[1]: r[3] for r in self.records if r[0] == T_INIT}

    @property
    def total_frames(self):
        return sum(r[1] for r in self.records if r[0] == T_FRAGMENT)


class a2amd_config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("samplerate", C.c_int32),
                ("basepitch", C.c_int32), ("channels", C.c_int32),
                ("device", C.c_int32), ("max_batch", C.c_uint32),
                ("stream", C.c_void_p)]


class a2amd_wavedesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("flags", C.c_uint32), ("period", C.c_uint32),
                ("size", C.c_uint32 * MIPLEVELS),
                ("data", C.POINTER(C.c_int16) * MIPLEVELS)]


class a2amd_noise_batch_info(C.Structure):
    """include/a2amd_noisepan.h: who rendered the noise voices of the most recent batch"""
    _fields_ = [("quiet_launched", C.c_uint32), ("quiet_voices", C.c_uint32),
                ("class_voices", C.c_uint32), ("standin_voices", C.c_uint32)]

    def __repr__(self):
        return "noise_batch_info(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_) + ")"


class a2amd_noise_filter_batch_info(C.Structure):
    """include/a2amd_noisefilt.h: who rendered the noise-filter voices of the most recent batch"""
    _fields_ = [("quiet_launched", C.c_uint32), ("quiet_voices", C.c_uint32),
                ("class_voices", C.c_uint32), ("min_voices", C.c_uint32)]

    def __repr__(self):
        return "noise_filter_batch_info(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_) + ")"


class a2amd_sweep_batch_info(C.Structure):
    """include/a2amd_sweep.h: the cutoff sweeps of the most recent batch's repeated fragments"""
    _fields_ = [("pass_launched", C.c_uint32), ("filters", C.c_uint32),
                ("ramp_windows", C.c_uint32), ("standin_voices", C.c_uint32)]

    def __repr__(self):
        return "sweep_batch_info(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_) + ")"


class a2amd_bus_info(C.Structure):
    """include/a2amd_bus.h: who rendered the bus owners - the root and the group voices - of the most recent batch"""
    _fields_ = [(n, C.c_uint32) for n in ("driver_voices", "driver_ramping", "driver_windows_dropped", "fbd_voices",
                                          "generic_voices", "consume", "master_direct")]

    def __repr__(self):
        return "bus_info(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_) + ")"


class a2amd_bare_batch_info(C.Structure):
    """include/a2amd_oscbare.h: who rendered the bare wtosc voices of the most recent batch, and the mono group drivers"""
    _fields_ = [(n, C.c_uint32) for n in ("launched", "class_voices", "quiet_voices", "gliding_voices", "record_voices",
                                          "vpw", "mono_drivers", "reserved")]

    def __repr__(self):
        return "bare_batch_info(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_) + ")"


class a2amd_osc3filt_batch_info(C.Structure):
    """include/a2amd_osc3filt.h: who rendered the 3 x wtosc-filter12-panmix voices of the most recent batch"""
    _fields_ = [(n, C.c_uint32) for n in ("launched", "class_voices", "quiet_voices", "gliding_voices", "record_voices",
                                          "vpg", "workgroups", "reserved")]

    def __repr__(self):
        return "osc3filt_batch_info(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_) + ")"


class a2amd_osc3filt_windows_info(C.Structure):
    """include/a2amd_osc3win.h: the 3 x wtosc-filter12-panmix voices whose only records of the most recent batch were cut
    windows - those the class's windows launch rendered, and those refused"""
    _fields_ = [(n, C.c_uint32) for n in ("launched", "window_voices", "gliding_voices", "windows", "refused_tiling",
                                          "vpg", "workgroups", "reserved")]

    def __repr__(self):
        return "osc3filt_windows_info(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_) + ")"


class a2amd_osc2_batch_info(C.Structure):
    """include/a2amd_osc2.h: how k_leaf_osc2pan walked the settled voices of the most recent batch"""
    _fields_ = [(n, C.c_uint32) for n in ("launched", "voices", "vpw", "ysplit", "voice_major", "superchunks_voice_major",
                                          "superchunks_chunk_major", "reserved")] + [("chunk_major_mask", C.c_uint64)]

    def __repr__(self):
        return "osc2_batch_info(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_) + ")"


class a2amd_osc2quiet_batch_info(C.Structure):
    """include/a2amd_osc2tame_kernel.h: k_leaf_osc2tame's launch in front of k_leaf_osc2pan in the most recent batch"""
    _fields_ = [("launched", C.c_uint32), ("wavefronts", C.c_uint32), ("taken_total", C.c_uint64)]

    def __repr__(self):
        return "osc2quiet_batch_info(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_) + ")"


class a2amd_fbdpan_batch_info(C.Structure):
    """include/a2amd_fbdpan.h: who rendered the pan-tailed delay chains (inline; fbdelay x 1..4; panmix >) of the most recent batch"""
    _fields_ = [(n, C.c_uint32) for n in ("launched", "class_voices", "quiet_voices", "gliding_voices", "record_voices",
                                          "max_delays")] + [("reserved", C.c_uint32 * 2)]

    def __repr__(self):
        return "fbdpan_batch_info(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_[:-1]) + ")"


class a2amd_bus_windows_info(C.Structure):
    """include/a2amd_buswin.h: the delay-chain bus owners of the most recent batch whose only records were cut windows"""
    _fields_ = [(n, C.c_uint32) for n in ("fbd_dropped", "fbdpan_voices", "fbdpan_gliding", "fbdpan_windows", "refused_tiling",
                                          "refused_cap", "window_cap", "launched")]

    def __repr__(self):
        return "bus_windows_info(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_) + ")"


class a2amd_vm_batch_info(C.Structure):
    """include/a2amd_vmbatch.h: who ran the device VM's voices of the most recent batch"""
    _fields_ = [("listed", C.c_uint32), ("class_voices", C.c_uint32 * 3), ("other_voices", C.c_uint32),
                ("pending", C.c_uint32), ("fused", C.c_uint32), ("not_fused", C.c_uint32),
                ("spec_valid", C.c_uint32), ("spec_taken", C.c_uint32), ("spec_miss", C.c_uint32),
                ("spec_next", C.c_uint32), ("spec_why_not", C.c_uint32), ("records", C.c_uint32),
                ("idle_known", C.c_uint32), ("idle", C.c_uint32 * 3), ("quiet_launched", C.c_uint32 * 3)]

    def __repr__(self):
        return ("vm_batch_info(" + ", ".join(f"{n}={list(getattr(self, n)) if n in ('class_voices', 'idle', 'quiet_launched') else getattr(self, n)}"
                                             for n, _ in self._fields_) + ")")


class a2amd_wave_pool_info(C.Structure):
    """include/a2amd_wavepool.h: what the host has done with the wave pool and the tables that follow it"""
    _fields_ = [(n, C.c_uint64) for n in ("used", "capacity", "free_samples")] + \
               [(n, C.c_uint32) for n in ("coef4", "raw_waves", "reallocations", "regions_reused")]

    def __repr__(self):
        return "wave_pool_info(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_) + ")"


class a2amd_vm_state(C.Structure):
    """include/a2amd_vm.h: A2_vmstate, field for field"""
    _fields_ = [("waketime", C.c_uint32), ("state", C.c_uint8), ("func", C.c_uint8), ("pc", C.c_uint16),
                ("r", C.c_int32 * 64)]


class Backend:
    """Thin ctypes veneer over one implementation of the call protocol."""

    def __init__(self, lib, prefix, samplerate, basepitch, channels=2, device=0,
                 max_batch=64, stream=None):
        self.lib, self.prefix, self.channels = lib, prefix, channels

        def fn(name, restype, *argtypes):
            f = getattr(lib, prefix + name)
            f.restype, f.argtypes = restype, list(argtypes)
            return f

        vp, i32, u32, u64 = C.c_void_p, C.c_int, C.c_uint, C.c_uint64
        self._open = fn("open", i32, C.POINTER(a2amd_config), C.POINTER(vp))
        self._close = fn("close", None, vp)
        self._err = fn("last_error", C.c_char_p, vp)
        self._wave_upload = fn("wave_upload", i32, vp, u64, C.POINTER(a2amd_wavedesc))
        self._wave_drop = fn("wave_drop", i32, vp, u64)
        self._fragment = fn("fragment", i32, vp, u32)
        self._unit_init = fn("unit_init", i32, vp, u64, i32, u32, i32, i32, i32, i32, u32)
        self._unit_deinit = fn("unit_deinit", i32, vp, i32)
        self._unit_write = fn("unit_write", i32, vp, i32, i32, i32, u32, u32, i32)
        self._unit_process = fn("unit_process", i32, vp, i32, u32, u32, C.POINTER(C.c_uint32))
        self._inline_end = fn("inline_end", i32, vp, i32)
        self._unit_clients = fn("unit_clients", i32, vp, i32, u32)
        self._unit_inject = fn("unit_inject", i32, vp, i32, u32, u32, C.POINTER(C.POINTER(C.c_int32)))
        self._unit_tapped = fn("unit_tapped", i32, vp, i32, u32, C.POINTER(C.POINTER(C.c_int32)))
        self._render = fn("render", i32, vp, u32, C.POINTER(C.POINTER(C.c_int32)), u32)
        self._set_pt = fn("set_pitch_table", i32, vp, C.POINTER(C.c_uint32))
        self._get_pt = fn("get_pitch_table", i32, vp, C.POINTER(C.c_uint32))
        # the host walk's short cuts (the product library only; the checker has none)
        self.has_walk = hasattr(lib, prefix + "voice_process")
        if self.has_walk:
            self._voice_process = fn("voice_process", i32, vp, i32, u32, u32, C.POINTER(C.c_uint32))
            self._voice_slot = fn("voice_slot", i32, vp, i32)
            self._default_map = fn("default_map", C.POINTER(C.c_uint8), vp, C.POINTER(u32))
        # stretches of default windows (the product library only)
        self._fragment_repeat_noise = None
        if hasattr(lib, prefix + "fragment_repeat_noise"):
            self._fragment_repeat_noise = fn("fragment_repeat_noise", i32, vp, u32, u32, C.POINTER(C.c_uint32))
        self._last_batch_noise = None
        if hasattr(lib, prefix + "last_batch_noise"):
            self._last_batch_noise = fn("last_batch_noise", i32, vp, C.POINTER(a2amd_noise_batch_info))
        self._last_batch_noise_filter = None
        if hasattr(lib, prefix + "last_batch_noise_filter"):
            self._last_batch_noise_filter = fn("last_batch_noise_filter", i32, vp, C.POINTER(a2amd_noise_filter_batch_info))
        self._fragment_repeat = None
        if hasattr(lib, prefix + "fragment_repeat"):
            self._fragment_repeat = fn("fragment_repeat", i32, vp, u32, u32)
        self._last_batch_sweeps = None
        if hasattr(lib, prefix + "last_batch_sweeps"):
            self._last_batch_sweeps = fn("last_batch_sweeps", i32, vp, C.POINTER(a2amd_sweep_batch_info))
        self._last_batch_buses = None
        if hasattr(lib, prefix + "last_batch_buses"):
            self._last_batch_buses = fn("last_batch_buses", i32, vp, C.POINTER(a2amd_bus_info))
        self._last_batch_bare = None
        if hasattr(lib, prefix + "last_batch_bare"):
            self._last_batch_bare = fn("last_batch_bare", i32, vp, C.POINTER(a2amd_bare_batch_info))
        self._last_batch_osc3filt = None
        if hasattr(lib, prefix + "last_batch_osc3filt"):
            self._last_batch_osc3filt = fn("last_batch_osc3filt", i32, vp, C.POINTER(a2amd_osc3filt_batch_info))
        self._last_batch_osc3filt_windows = None
        if hasattr(lib, prefix + "last_batch_osc3filt_windows"):
            self._last_batch_osc3filt_windows = fn("last_batch_osc3filt_windows", i32, vp, C.POINTER(a2amd_osc3filt_windows_info))
        self._last_batch_osc2 = None
        if hasattr(lib, prefix + "last_batch_osc2"):
            self._last_batch_osc2 = fn("last_batch_osc2", i32, vp, C.POINTER(a2amd_osc2_batch_info))
        self._last_batch_osc2quiet = None
        if hasattr(lib, prefix + "last_batch_osc2quiet"):
            self._last_batch_osc2quiet = fn("last_batch_osc2quiet", i32, vp, C.POINTER(a2amd_osc2quiet_batch_info))
            self._osc2quiet_hold = fn("osc2quiet_hold", i32, vp, i32)
        # include/a2amd_osc2lds.h: pure functions, no context (the product library only)
        self._osc2_stage_rule = self._wave_level_periodic = None
        if hasattr(lib, prefix + "osc2_stage_rule"):
            self._osc2_stage_rule = fn("osc2_stage_rule", u32, u32, i32, u32, i32)
            self._wave_level_periodic = fn("wave_level_periodic", i32, C.POINTER(C.c_int16), u32)
        # include/a2amd_osc2tame.h: likewise
        self._osc2_tame_rule = self._wave_level_tame = None
        if hasattr(lib, prefix + "osc2_tame_rule"):
            self._osc2_tame_rule = fn("osc2_tame_rule", u32, i32, i32)
            self._wave_level_tame = fn("wave_level_tame", i32, C.POINTER(C.c_int16), u32)
            self._osc2_tame_voices = fn("osc2_tame_voices", i32, vp, C.POINTER(C.c_uint64))
        # include/a2amd_wavepool.h: the wave pool's bookkeeping (the product library only)
        if hasattr(lib, prefix + "wave_pool_info"):
            self._wave_pool_info = fn("wave_pool_info", i32, vp, C.POINTER(a2amd_wave_pool_info))

            def wave_pool_info():
                """a2amd_wave_pool_info: pool samples used, capacity, samples on the free list, whether the 16 byte
                table exists, live waves flagged raw, pool reallocations and regions reused since open"""
                pi = a2amd_wave_pool_info()
                self._chk(self._wave_pool_info(self.ctx, C.byref(pi)), "wave_pool_info")
                return pi
            self.wave_pool_info = wave_pool_info
        self._last_batch_fbdpan = None
        if hasattr(lib, prefix + "last_batch_fbdpan"):
            self._last_batch_fbdpan = fn("last_batch_fbdpan", i32, vp, C.POINTER(a2amd_fbdpan_batch_info))
        self._last_batch_bus_windows = None
        if hasattr(lib, prefix + "last_batch_bus_windows"):
            self._last_batch_bus_windows = fn("last_batch_bus_windows", i32, vp, C.POINTER(a2amd_bus_windows_info))
        # the device VM (the product library only; include/a2amd_vm.h)
        self.has_vm = hasattr(lib, prefix + "vm_adopt")
        if self.has_vm:
            self._fragment_offset = fn("fragment_offset", i32, vp, u32)
            self._vm_program = fn("vm_program", i32, vp, u64, C.POINTER(C.c_uint32), u32)
            self._vm_adopt = fn("vm_adopt", i32, vp, i32, i32, C.POINTER(a2amd_vm_state), C.POINTER(C.c_int32),
                                C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, vp, i32)
            self._vm_expect_cuts = fn("vm_expect_cuts", i32, vp, C.POINTER(C.c_uint32), i32)
            self._vm_recall = fn("vm_recall", i32, vp, C.POINTER(C.c_int32), u32, C.POINTER(a2amd_vm_state), vp)
        self._last_batch_vm = None
        if hasattr(lib, prefix + "last_batch_vm"):
            self._last_batch_vm = fn("last_batch_vm", i32, vp, C.POINTER(a2amd_vm_batch_info))
        # waves built on the device from what it rendered (the product library only)
        self.has_capture = hasattr(lib, prefix + "wave_upload_captured_post")
        if self.has_capture:
            self._capture_begin = fn("capture_begin", i32, vp)
            self._capture_end = fn("capture_end", i32, vp, C.POINTER(vp))
            self._capture_frames = fn("capture_frames", u32, vp)
            self._capture_free = fn("capture_free", None, vp)
            self._wave_upload_captured = fn("wave_upload_captured", i32, vp, u64, C.POINTER(a2amd_wavedesc), vp)
            self._wave_upload_captured_post = fn("wave_upload_captured_post", i32, vp, u64, C.POINTER(a2amd_wavedesc), vp, u32)
            self._wave_stats = fn("wave_stats", i32, vp, C.POINTER(u64), C.POINTER(u32), C.POINTER(u32))
        cfg = a2amd_config(C.sizeof(a2amd_config), samplerate, basepitch, channels,
                           device, max_batch, stream)
        self.ctx = vp()
        rc = self._open(C.byref(cfg), C.byref(self.ctx))
        if rc != 0:
            raise RuntimeError(f"{prefix}open failed: {rc} "
                               f"{self._err(None).decode(errors='replace')}")
        self.noise = C.c_uint32(0)
        self._keep = []

    def close(self):
        if self.ctx:
            self._close(self.ctx)
            self.ctx = None

    def _chk(self, rc, what):
        if rc < 0:
            msg = self._err(self.ctx)
            raise RuntimeError(f"{self.prefix}{what}: {rc} {msg.decode(errors='replace') if msg else ''}")
        return rc

    def wave_upload(self, key, wtype, flags, period, sizes, data):
        d = a2amd_wavedesc()
        d.type, d.flags, d.period = wtype, flags, period
        for lv, arr in enumerate(data):
            arr = np.ascontiguousarray(arr, dtype=np.int16)
            self._keep.append(arr)
            d.size[lv] = sizes[lv]
            d.data[lv] = arr.ctypes.data_as(C.POINTER(C.c_int16))
        return self._chk(self._wave_upload(self.ctx, key, C.byref(d)), "wave_upload")

    def capture_begin(self):
        """From here on channel 0 of everything this context renders is also kept in device memory."""
        return self._chk(self._capture_begin(self.ctx), "capture_begin")

    def capture_end(self):
        """Detaches what was kept: an opaque capture (it outlives the context; release it with capture_free()),
        or None when nothing was rendered."""
        cap = C.c_void_p()
        self._chk(self._capture_end(self.ctx, C.byref(cap)), "capture_end")
        return cap if cap.value else None

    def capture_frames(self, cap):
        return self._capture_frames(cap)

    def capture_free(self, cap):
        self._capture_free(cap)

    def wave_upload_captured(self, key, wtype, flags, period, sizes, cap, chunk=None, check=True):
        """A wave built on the device from a capture (a2amd_wave_upload_captured).  With `chunk` - the frames per
        write of the render, A2_config.buffer of the rendering substate - the entry point that also applies
        A2_NORMALIZE / A2_XFADE there (a2amd_wave_upload_captured_post).  check=False: the return code as it is."""
        d = a2amd_wavedesc()
        d.type, d.flags, d.period = wtype, flags, period
        for lv, n in enumerate(sizes):
            d.size[lv] = n
        if chunk is None:
            rc = self._wave_upload_captured(self.ctx, key, C.byref(d), cap)
        else:
            rc = self._wave_upload_captured_post(self.ctx, key, C.byref(d), cap, chunk)
        return self._chk(rc, "wave_upload_captured") if check else rc

    def wave_stats(self):
        """(bytes of wave data copied from the host, waves copied from the host, waves built from captures)"""
        h2d, up, res = C.c_uint64(), C.c_uint32(), C.c_uint32()
        self._chk(self._wave_stats(self.ctx, C.byref(h2d), C.byref(up), C.byref(res)), "wave_stats")
        return h2d.value, up.value, res.value

    def wave_drop(self, key):
        return self._chk(self._wave_drop(self.ctx, key), "wave_drop")

    def fragment(self, frames):
        return self._chk(self._fragment(self.ctx, frames), "fragment")

    def fragment_repeat(self, frames, count):
        """`count` further fragments of default windows (a2amd_fragment_repeat): no noise oscillators; the
        coefficients of filters whose cutoff is sweeping are made on the device."""
        if self._fragment_repeat is None:
            raise RuntimeError(f"this library has no {self.prefix}fragment_repeat")
        return self._chk(self._fragment_repeat(self.ctx, frames, count), "fragment_repeat")

    def last_batch_sweeps(self):
        """a2amd_last_batch_sweeps: whether the sweep pass ran for the most recent batch, the filters it listed,
        the windows in which a cutoff moved, the voices given the stand-in record for it"""
        if self._last_batch_sweeps is None:
            raise RuntimeError(f"this library has no {self.prefix}last_batch_sweeps")
        bi = a2amd_sweep_batch_info()
        self._chk(self._last_batch_sweeps(self.ctx, C.byref(bi)), "last_batch_sweeps")
        return bi

    def fragment_repeat_noise(self, frames, count):
        """`count` further fragments of default windows, settled noise oscillators seeded on the device
        (a2amd_fragment_repeat_noise): self.noise goes in and comes back as `count` walks by calls would
        have left it."""
        if self._fragment_repeat_noise is None:
            raise RuntimeError(f"this library has no {self.prefix}fragment_repeat_noise")
        return self._chk(self._fragment_repeat_noise(self.ctx, frames, count, C.byref(self.noise)),
                         "fragment_repeat_noise")

    def last_batch_noise(self):
        """a2amd_last_batch_noise: whether k_leaf_noisepan was launched for the most recent batch, the voices it
        rendered, the voices of its launch class, the noise voices given the stand-in record instead"""
        if self._last_batch_noise is None:
            raise RuntimeError(f"this library has no {self.prefix}last_batch_noise")
        bi = a2amd_noise_batch_info()
        self._chk(self._last_batch_noise(self.ctx, C.byref(bi)), "last_batch_noise")
        return bi

    def last_batch_noise_filter(self):
        """a2amd_last_batch_noise_filter: whether k_leaf_noisefiltpan was launched for the most recent batch, the voices
        left to it, the voices of its launch class, the threshold in force (A2AMD_NZF_MIN)"""
        if self._last_batch_noise_filter is None:
            raise RuntimeError(f"this library has no {self.prefix}last_batch_noise_filter")
        bi = a2amd_noise_filter_batch_info()
        self._chk(self._last_batch_noise_filter(self.ctx, C.byref(bi)), "last_batch_noise_filter")
        return bi

    def last_batch_buses(self):
        """a2amd_last_batch_buses: the bus owners of the most recent batch by the kernel that rendered them - k_bus_driver
        (and how many of those ramping, how many with their cut windows dropped), k_bus_fbdchain, the general kernel -
        what the bus launches were told to consume, whether the root stored into the host's buffer"""
        if self._last_batch_buses is None:
            raise RuntimeError(f"this library has no {self.prefix}last_batch_buses")
        bi = a2amd_bus_info()
        self._chk(self._last_batch_buses(self.ctx, C.byref(bi)), "last_batch_buses")
        return bi

    def last_batch_bare(self):
        """a2amd_last_batch_bare: whether k_leaf_oscbare was launched for the most recent batch, the voices of its launch
        class (bare wtosc: one unit, wired, adding) by who rendered them - the kernel (of which still gliding), the
        general kernel (those with records) - its voices per wavefront, and the mono owners on k_bus_driver's lists"""
        if self._last_batch_bare is None:
            raise RuntimeError(f"this library has no {self.prefix}last_batch_bare")
        bi = a2amd_bare_batch_info()
        self._chk(self._last_batch_bare(self.ctx, C.byref(bi)), "last_batch_bare")
        return bi

    def last_batch_osc3filt(self):
        """a2amd_last_batch_osc3filt: whether k_leaf_osc3filtpan was launched for the most recent batch, the voices of its
        launch class (3 x wtosc; filter12; panmix) by who rendered them - the kernel (of which still gliding), the general
        kernel (those with a run) - its voices per workgroup and its workgroups"""
        if self._last_batch_osc3filt is None:
            raise RuntimeError(f"this library has no {self.prefix}last_batch_osc3filt")
        bi = a2amd_osc3filt_batch_info()
        self._chk(self._last_batch_osc3filt(self.ctx, C.byref(bi)), "last_batch_osc3filt")
        return bi

    def last_batch_osc3filt_windows(self):
        """a2amd_last_batch_osc3filt_windows: whether k_leaf_osc3filtpan_win, the windows launch, ran for the most recent
        batch, the voices of the class whose windows-only run it rendered (of which still gliding), their windows, the
        windows-only runs refused for not tiling, its voices per workgroup and its workgroups"""
        if self._last_batch_osc3filt_windows is None:
            raise RuntimeError(f"this library has no {self.prefix}last_batch_osc3filt_windows")
        wi = a2amd_osc3filt_windows_info()
        self._chk(self._last_batch_osc3filt_windows(self.ctx, C.byref(wi)), "last_batch_osc3filt_windows")
        return wi

    def last_batch_osc2(self):
        """a2amd_last_batch_osc2: whether k_leaf_osc2pan was launched for the most recent batch, the voices on its list,
        its launch shape, and the super-chunks of the batch by the walk their settled voices took - voice by voice
        (whole fragments only) or chunk by chunk (a short fragment among them, or A2AMD_DEBUG bit 16)"""
        if self._last_batch_osc2 is None:
            raise RuntimeError(f"this library has no {self.prefix}last_batch_osc2")
        bi = a2amd_osc2_batch_info()
        self._chk(self._last_batch_osc2(self.ctx, C.byref(bi)), "last_batch_osc2")
        return bi

    def last_batch_osc2quiet(self):
        """a2amd_last_batch_osc2quiet: whether k_leaf_osc2tame was launched in front of k_leaf_osc2pan for the most recent
        batch, the wavefronts of that launch list, and the wavefronts it took, summed over its launches so far (read
        from the device: waits for the stream)"""
        if self._last_batch_osc2quiet is None:
            raise RuntimeError(f"this library has no {self.prefix}last_batch_osc2quiet")
        bi = a2amd_osc2quiet_batch_info()
        self._chk(self._last_batch_osc2quiet(self.ctx, C.byref(bi)), "last_batch_osc2quiet")
        return bi

    def osc2quiet_hold(self, hold):
        """a2amd_osc2quiet_hold: from the next batch on k_leaf_osc2pan alone (hold), or the pair by its rule again"""
        if self._last_batch_osc2quiet is None:
            raise RuntimeError(f"this library has no {self.prefix}osc2quiet_hold")
        self._chk(self._osc2quiet_hold(self.ctx, int(bool(hold))), "osc2quiet_hold")

    def osc2_stage_rule(self, size0, periodic0, size1, periodic1):
        """a2amd_osc2_stage_rule: the mask of a settled `wtosc; wtosc; panmix` voice's oscillators whose taps
        k_leaf_osc2pan's voice-major walk reads from a copy of the mip level in LDS, from the sizes of the levels they
        play and whether those levels' pads are periodic (bit 0: the first oscillator, bit 1: the second)"""
        if self._osc2_stage_rule is None:
            raise RuntimeError(f"this library has no {self.prefix}osc2_stage_rule")
        return int(self._osc2_stage_rule(size0, int(bool(periodic0)), size1, int(bool(periodic1))))

    def osc2_tame_rule(self, tame0, tame1):
        """a2amd_osc2_tame_rule: does a settled `wtosc; wtosc; panmix` voice whose oscillators play levels that are
        tame or not take the fused multiply-add steps on the voice-major walk"""
        if self._osc2_tame_rule is None:
            raise RuntimeError(f"this library has no {self.prefix}osc2_tame_rule")
        return int(self._osc2_tame_rule(int(bool(tame0)), int(bool(tame1))))

    def osc2_tame_voices(self):
        """a2amd_osc2_tame_voices: the voices k_leaf_osc2pan gave the tame bit, summed over its launches so far"""
        if self._osc2_tame_rule is None:
            raise RuntimeError(f"this library has no {self.prefix}osc2_tame_voices")
        n = C.c_uint64(0)
        self._chk(self._osc2_tame_voices(self.ctx, C.byref(n)), "osc2_tame_voices")
        return int(n.value)

    def wave_level_tame(self, level, size=None):
        """a2amd_wave_level_tame: does no product of the Hermite interpolation wrap anywhere in this level - int16,
        WAVEPRE + size + WAVEPOST samples, as wave_upload() takes it"""
        if self._wave_level_tame is None:
            raise RuntimeError(f"this library has no {self.prefix}wave_level_tame")
        arr = np.ascontiguousarray(level, dtype=np.int16)
        n = len(arr) - WAVEPRE - WAVEPOST if size is None else size
        return bool(self._wave_level_tame(arr.ctypes.data_as(C.POINTER(C.c_int16)), n))

    def wave_level_periodic(self, level):
        """a2amd_wave_level_periodic: are the pads of this level - int16, WAVEPRE + size + WAVEPOST samples, as
        wave_upload() takes it - the periodic continuation of its payload"""
        if self._wave_level_periodic is None:
            raise RuntimeError(f"this library has no {self.prefix}wave_level_periodic")
        arr = np.ascontiguousarray(level, dtype=np.int16)
        return bool(self._wave_level_periodic(arr.ctypes.data_as(C.POINTER(C.c_int16)), len(arr) - WAVEPRE - WAVEPOST))

    def last_batch_fbdpan(self):
        """a2amd_last_batch_fbdpan: whether k_bus_fbdpan was launched for the most recent batch, the bus owners of its
        class (inline; fbdelay x 1..4; panmix wired and adding) by who rendered them - the kernel (of which within the
        host's bound for a moving volume or pan), the general kernel (those with records) - and the longest chain"""
        if self._last_batch_fbdpan is None:
            raise RuntimeError(f"this library has no {self.prefix}last_batch_fbdpan")
        bi = a2amd_fbdpan_batch_info()
        self._chk(self._last_batch_fbdpan(self.ctx, C.byref(bi)), "last_batch_fbdpan")
        return bi

    def last_batch_bus_windows(self):
        """a2amd_last_batch_bus_windows: the delay-chain bus owners whose only records this batch were cut windows - wired
        chains whose records were dropped (k_bus_fbdchain's), pan-tailed chains on k_bus_fbdpan's windows launch (of which
        within the host's bound for a moving volume or pan, and the table rows their runs need), the runs left to the
        general kernel because they do not tile their fragments or need more rows than window_cap, and whether the
        windows launch ran"""
        if self._last_batch_bus_windows is None:
            raise RuntimeError(f"this library has no {self.prefix}last_batch_bus_windows")
        bi = a2amd_bus_windows_info()
        self._chk(self._last_batch_bus_windows(self.ctx, C.byref(bi)), "last_batch_bus_windows")
        return bi

    def last_batch_vm(self):
        """a2amd_last_batch_vm: the device VM's voices of the most recent batch by class, whether their VMs ran fused
        (k_vm_win, or a speculative pass taken: k_vm_commit) or through records (k_vm_count / k_vm_emit) and why, and
        whether a pass for the next batch was launched behind it"""
        if self._last_batch_vm is None:
            raise RuntimeError(f"this library has no {self.prefix}last_batch_vm")
        bi = a2amd_vm_batch_info()
        self._chk(self._last_batch_vm(self.ctx, C.byref(bi)), "last_batch_vm")
        return bi

    def fragment_offset(self, offset):
        """the open fragment begins `offset` frames inside the engine's own 64-frame fragment (a2amd_fragment_offset)"""
        return self._chk(self._fragment_offset(self.ctx, offset), "fragment_offset")

    def vm_program(self, key, words):
        """a2amd_vm_program: the text of one function (32 bit words); the program id"""
        code = (C.c_uint32 * len(words))(*[w & 0xffffffff for w in words])
        return self._chk(self._vm_program(self.ctx, key, code, len(words)), "vm_program")

    def vm_adopt(self, head_unit, prog, state, wires, now, msdur, check=True):
        """a2amd_vm_adopt without env units.  state: a2amd_vm_state; wires: {VM register: (backend unit, its register)}.
        check=False: the return code as it is (a refusal is an answer)."""
        wu = (C.c_int32 * 64)(*([-1] * 64))
        wr = (C.c_uint8 * 64)()
        for r, (u, ureg) in wires.items():
            wu[r], wr[r] = u, ureg
        rc = self._vm_adopt(self.ctx, head_unit, prog, C.byref(state), wu, wr, now & 0xffffffff, msdur, None, 0)
        return self._chk(rc, "vm_adopt") if check else rc

    def vm_expect_cuts(self, when):
        """a2amd_vm_expect_cuts: engine times (24:8) at which the root's VM wakes next; [] forgets them"""
        arr = (C.c_uint32 * max(len(when), 1))(*[w & 0xffffffff for w in when])
        return self._chk(self._vm_expect_cuts(self.ctx, arr, len(when)), "vm_expect_cuts")

    def vm_recall(self, head_units):
        """a2amd_vm_recall: the voices go back to the host; their a2amd_vm_state as of the start of the open fragment"""
        n = len(head_units)
        out = (a2amd_vm_state * n)()
        self._chk(self._vm_recall(self.ctx, (C.c_int32 * n)(*head_units), n, out, None), "vm_recall")
        return list(out)

    def last_error(self):
        msg = self._err(self.ctx)
        return msg.decode(errors="replace") if msg else ""

    def unit_init(self, voice_key, kind, flags, nin, nout, wired, transpose=0, wakefrac=0):
        return self._chk(self._unit_init(self.ctx, voice_key, kind, flags, nin, nout, wired,
                                         transpose, wakefrac), "unit_init")

    def unit_deinit(self, unit):
        return self._chk(self._unit_deinit(self.ctx, unit), "unit_deinit")

    def unit_write(self, unit, reg, value, start=0, dur=0, transpose=0):
        return self._chk(self._unit_write(self.ctx, unit, reg, value, start, dur, transpose),
                         "unit_write")

    def unit_process(self, unit, offset, frames, use_noise=True):
        return self._chk(self._unit_process(self.ctx, unit, offset, frames,
                                            C.byref(self.noise) if use_noise else None),
                         "unit_process")

    def voice_process(self, units, offset, frames):
        """One window of a whole voice (units = its chain): a2amd_voice_process where the
        library has it, else unit by unit.  Returns 1 when the voice's default windows may
        be reported through mark_default() from the next fragment on."""
        if self.has_walk:
            return self._chk(self._voice_process(self.ctx, units[0], offset, frames, C.byref(self.noise)),
                             "voice_process")
        for u in units:
            self.unit_process(u, offset, frames)
        return 0

    def mark_default(self, units):
        """The voice got exactly the default window in the open fragment: one byte store
        into the default map (a2amd_default_map)."""
        n = C.c_uint(0)
        m = self._default_map(self.ctx, C.byref(n))
        slot = self._chk(self._voice_slot(self.ctx, units[0]), "voice_slot")
        assert m and slot < n.value
        m[slot] = 1

    def inline_end(self, unit):
        return self._chk(self._inline_end(self.ctx, unit), "inline_end")

    def unit_clients(self, unit, mode):
        """mode: 1 = tap the unit's input for READ clients, 2 = take WRITE clients' output."""
        return self._chk(self._unit_clients(self.ctx, unit, mode), "unit_clients")

    def unit_inject(self, unit, offset, audio):
        """audio: int32 [channels, frames] produced by the WRITE clients for this window."""
        audio = np.ascontiguousarray(audio, dtype=np.int32)
        ptrs = (C.POINTER(C.c_int32) * audio.shape[0])()
        for c in range(audio.shape[0]):
            ptrs[c] = audio[c].ctypes.data_as(C.POINTER(C.c_int32))
        return self._chk(self._unit_inject(self.ctx, unit, offset, audio.shape[1], ptrs), "unit_inject")

    def unit_tapped(self, unit, fragment):
        """int32 [channels, 64]: what the unit's inputs carried in `fragment` of the last batch."""
        ptrs = (C.POINTER(C.c_int32) * 8)()
        n = self._chk(self._unit_tapped(self.ctx, unit, fragment, ptrs), "unit_tapped")
        return np.stack([np.ctypeslib.as_array(ptrs[c], shape=(64,)).copy() for c in range(n)])

    def render(self, capacity_frames, phases=15):
        out = np.zeros((self.channels, max(capacity_frames, 1)), dtype=np.int32)
        ptrs = (C.POINTER(C.c_int32) * self.channels)()
        for c in range(self.channels):
            ptrs[c] = out[c].ctypes.data_as(C.POINTER(C.c_int32))
        n = self._chk(self._render(self.ctx, phases, ptrs, capacity_frames), "render")
        return out[:, :n]

    def render_kept(self, capacity_frames):
        """render() with A2AMD_RENDER_KEEP: the batch stays recorded and uploaded, for replay() or another render()"""
        return self.render(capacity_frames, phases=15 | 16)

    def replay(self, steps):
        """a2amd_replay: the kept batch `steps` times more, unheard (eight steps to a graph, the rest one by one)"""
        f = getattr(self.lib, self.prefix + "replay")
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_uint]
        return self._chk(f(self.ctx, steps), "replay")

    def set_pitch_table(self, tab):
        tab = np.ascontiguousarray(tab, dtype=np.uint32)
        return self._chk(self._set_pt(self.ctx, tab.ctypes.data_as(C.POINTER(C.c_uint32))), "set_pt")

    def get_pitch_table(self):
        tab = np.zeros(128, dtype=np.uint32)
        self._chk(self._get_pt(self.ctx, tab.ctypes.data_as(C.POINTER(C.c_uint32))), "get_pt")
        return tab


def replay(trace, backend, batch=64, check_noise=True, max_fragments=None):
    """Feed `trace` to `backend`; returns int32 [channels, frames].

    `batch` fragments are recorded between renders.  When `check_noise` is set
    the engine-global noise state after every wtosc Process call is compared
    with what the reference had at that point.
    """
    umap, wmap = {}, {}
    outs = []
    nfrag = 0
    pending = 0
    backend.noise.value = trace.config["noiseseed"]
    for r in trace.records:
        op = r[0]
        if op == T_FRAGMENT:
            if max_fragments is not None and nfrag >= max_fragments:
                break
            if pending and nfrag % batch == 0:
                outs.append(backend.render(pending))
                pending = 0
            backend.fragment(r[1])
            pending += r[1]
            nfrag += 1
        elif op == T_WAVE:
            w = trace.waves[r[1]]
            wmap[r[1]] = backend.wave_upload(0x1000 + r[1], w["type"], w["flags"], w["period"],
                                             w["sizes"], w["data"])
        elif op == T_WAVEDROP:
            # the wave was released between two a2_Run() calls: what was
            # recorded so far plays it to the end
            if pending:
                outs.append(backend.render(pending))
                pending = 0
            backend.wave_drop(0x1000 + r[1])
            wmap.pop(r[1], None)
        elif op == T_INIT:
            _, uid, voice, kind, flags, io, transpose, wakefrac = r
            umap[uid] = backend.unit_init(voice, kind, flags & 0xFFFFFFFF, io & 0xFF,
                                          (io >> 8) & 0xFF, (io >> 16) & 1, transpose, wakefrac)
        elif op == T_DEINIT:
            backend.unit_deinit(umap.pop(r[1]))
        elif op == T_WRITE:
            _, uid, reg, value, start, dur, transpose, _g = r
            if trace.kinds.get(uid) == 0 and reg == 0:      # wtosc 'w'
                value = wmap.get(value, -1)
            backend.unit_write(umap[uid], reg, value, start & 0xFFFFFFFF, dur & 0xFFFFFFFF, transpose)
        elif op == T_PROCESS:
            _, uid, offset, frames, is_osc, before, after, _g = r
            if is_osc:
                backend.noise.value = before & 0xFFFFFFFF
            backend.unit_process(umap[uid], offset, frames)
            if is_osc and check_noise and backend.noise.value != (after & 0xFFFFFFFF):
                raise AssertionError(f"noise state diverged at unit {uid}: "
                                     f"{backend.noise.value:#x} != {after & 0xFFFFFFFF:#x}")
        elif op == T_INLINE_END:
            backend.inline_end(umap[r[1]])
    if pending:
        outs.append(backend.render(pending))
    return np.concatenate(outs, axis=1) if outs else np.zeros((backend.channels, 0), np.int32)


def read_pcm(path, channels, buffer):
    """PCM written by ref_tools: per a2_Run() call, `channels` planar blocks."""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rb") as f:
        raw = np.frombuffer(f.read(), dtype="<i4")
    nfull = len(raw) // (channels * buffer)
    body = raw[: nfull * channels * buffer].reshape(nfull, channels, buffer)
    out = body.transpose(1, 0, 2).reshape(channels, nfull * buffer)
    rest = raw[nfull * channels * buffer:]
    if len(rest):
        out = np.concatenate([out, rest.reshape(channels, -1)], axis=1)
    return out
