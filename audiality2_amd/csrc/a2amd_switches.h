// Everything the environment can tell liba2amd.so: one table, read once per context by a2amd_open() into a2amd_ctx::sw
// (and once more, without a context, by the timing dump at process exit).  A switch is fixed when its context is opened.
// No other source of the library calls getenv("A2AMD_...") (tests/test_switches.py).  Plain C++, no HIP.
// (a2amd_units.c and a2amd_walk.c are libraries of their own with their own init-time reads.)
#pragma once
#include <stdlib.h>

namespace a2sw {
// the ways a switch is parsed.  atoi: "" and "abc" are 0.
static inline bool set(const char *name) { return getenv(name) != nullptr; }					// present at all ("" counts)
static inline bool on(const char *name) { const char *e = getenv(name); return !(e && !atoi(e)); }		// on unless it reads 0 ("" is off)
static inline int num(const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; }
static inline int num1(const char *name, int unset) { const char *e = getenv(name); return e ? (atoi(e) > 1 ? atoi(e) : 1) : unset; }	// ... at least 1
static inline int full(const char *name, int unset) { const char *e = getenv(name); return (e && *e) ? atoi(e) : unset; }	// "" counts as unset
static inline int within(const char *name, int lo, int hi) { const int v = num(name, 0); return v >= lo && v <= hi ? v : 0; }	// 0: not forced
}

// X(type, member, read)	// name, default: meaning.  "x_set": whether the switch was there at all, where the code asks.
#define A2AMD_SWITCHES(X) \
	X(bool, bus_windows, a2sw::set("A2AMD_BUS_WINDOWS"))	/* unset: driver chains at rest and wired delay chains drop windows-only records, pan-tailed delay chains take theirs to k_bus_fbdpan's windows launch (include/a2amd_buswin.h). Set: they go to the general kernel (A/B: round 4's routing) */ \
	X(bool, cls_check, a2sw::set("A2AMD_CLS_CHECK"))	/* unset. Set: every rebuild of the launch lists classifies every voice anew and fails on a remembered class that no longer holds */ \
	X(int, coef_cache_mb, a2sw::full("A2AMD_COEF_CACHE_MB", 192))	/* 192 ("" too): MB of Hermite entries beyond which waves of 4 096 samples or more play from their samples */ \
	X(int, dbg_walk, a2sw::num("A2AMD_DBG_WALK", 0))	/* 0. Bits: 1 a2amd_voice_process() never takes its short path, 2 ... never reports the default window (debugging the walk) */ \
	X(int, debug, a2sw::num("A2AMD_DEBUG", 0))		/* 0. A2DParams::debug, ablations: 1 no bus atomics (breaks the audio on purpose), 4 no shadow lanes in the FM kernel, 8 k_leaf_oscfiltpan's wavefronts add to the bus themselves, not through the workgroup's LDS sums, 16 k_leaf_osc2pan walks no super-chunk voice by voice (a launch argument; include/a2amd_osc2.h), 1 << 17 that walk stages no mip level in LDS (a launch argument; include/a2amd_osc2lds.h), 1 << 18 that walk takes the fused multiply-add steps for no voice (a launch argument; include/a2amd_osc2tame.h), 1 << 19 k_leaf_osc2tame is never launched in front of k_leaf_osc2pan, 1 << 20 it is whatever the class's size (the host's launch rule; include/a2amd_osc2tame_kernel.h) */ \
	X(bool, debug_noise, a2sw::set("A2AMD_DEBUG_NOISE"))	/* unset. Set: trace the noise oscillators' seeds (debugging aid) */ \
	X(int, f2vpw, a2sw::num("A2AMD_F2VPW", 0))		/* 0 = the launcher's own choice: voices per workgroup of k_leaf_osc2filtpan; and, clamped to 1..64, of k_leaf_osc3filtpan and its windows launch (0: by count) */ \
	X(bool, fmvpw_set, a2sw::set("A2AMD_FMVPW")) X(int, fmvpw, a2sw::num("A2AMD_FMVPW", 0))	/* unset = by count: voices per wavefront of k_leaf_fmpan. Set: no one-launch FM path */ \
	X(bool, fvpw_set, a2sw::set("A2AMD_FVPW")) X(int, fvpw, a2sw::num("A2AMD_FVPW", 0))	/* unset = by count: voices per wavefront of k_leaf_oscfiltpan */ \
	X(bool, hosttiming, a2sw::set("A2AMD_HOSTTIMING")) X(int, hosttiming_level, a2sw::num("A2AMD_HOSTTIMING", 0))	/* unset: host timing counters and their dump at exit; the level (2, 3) adds per-batch traces */ \
	X(bool, noise_quiet, a2sw::on("A2AMD_NOISE_QUIET"))	/* on. 0: no launch classes for wtosc (noise)-[filter12-]panmix voices - they are wtosc-[filter12-]panmix voices, and every noise voice of a device-seeded batch gets the stand-in record (A/B) */ \
	X(bool, no_direct, a2sw::set("A2AMD_NO_DIRECT"))	/* unset. Set: the root never stores the master bus straight into the host's buffer */ \
	X(int, no_fast, a2sw::num("A2AMD_NO_FAST", 0))		/* 0. Bit mask of classes sent to the general kernel: 1 wtosc-panmix, 2 wtosc-filter12-panmix, 4 driver chains, 8 2 x wtosc-panmix, 16 fm-panmix, 32 fbdelay chains, 64 no records kernel, 128 2 x wtosc-filter12-panmix, 256 bare wtosc, 512 pan-tailed fbdelay chains, 1024 3 x wtosc-filter12-panmix, 2048 no windows launch for that class - a voice of it whose run is windows only goes to the general kernel, as any other run of it does (include/a2amd_osc3win.h) (debugging / A-B tests) */ \
	X(bool, no_graph, a2sw::set("A2AMD_NO_GRAPH"))		/* unset. Set: no batch is captured into or replayed from a graph */ \
	X(bool, no_moving, a2sw::set("A2AMD_NO_MOVING"))	/* unset. Set: gliding voices get no stand-in record (they stay the quiet kernels') */ \
	X(bool, no_selfclean, a2sw::set("A2AMD_NO_SELFCLEAN"))	/* unset. Set: bus owners never count as clearing their own buses */ \
	X(bool, no_vm, a2sw::set("A2AMD_NO_VM"))		/* unset. Set: the device VM's cutoff -> coefficient table is not made (a2amd_units.c and a2amd_walk.c read the switch too: no voice is adopted) */ \
	X(bool, nzfvpg_set, a2sw::set("A2AMD_NZFVPG")) X(int, nzfvpg, a2sw::num("A2AMD_NZFVPG", 0))	/* unset = by count: voices per workgroup of k_leaf_noisefiltpan */ \
	X(int, nzf_min, a2sw::num1("A2AMD_NZF_MIN", 64))	/* 64, at least 1: such voices IN A BATCH from which wtosc (noise)-filter12-panmix has its quiet kernel (a2amd_host.h) */ \
	X(bool, nzvpw_set, a2sw::set("A2AMD_NZVPW")) X(int, nzvpw, a2sw::num("A2AMD_NZVPW", 0))	/* unset = by count: voices per wavefront of k_leaf_noisepan */ \
	X(int, o2f_min, a2sw::num("A2AMD_O2F_MIN", 512))	/* 512: voices of 2 x wtosc-filter12-panmix from which the class has its quiet kernel */ \
	X(int, raw, a2sw::full("A2AMD_RAW", -1))		/* -1 ("" too) = by footprint; 0 / 1: every wave plays from Hermite entries / from its samples */ \
	X(int, recs_wpb, a2sw::within("A2AMD_RECS_WPB", 1, 8))	/* 0 = by launch size; 1..8 (RECS_WPB, a2amd_fast.hip) forces the records kernels' wavefronts per workgroup, anything else is ignored */ \
	X(bool, rvpw_set, a2sw::set("A2AMD_RVPW")) X(int, rvpw, a2sw::num("A2AMD_RVPW", 0))	/* unset = by count: voices per wavefront of k_leaf_recs. Set: no one-launch records path, and the lane = voice filter keeps this value */ \
	X(int, vfilt, a2sw::num("A2AMD_VFILT", -1))		/* -1 = from 16 384 voices on; 0 / 1: k_leaf_recs' lane = voice filter off / on */ \
	X(int, vmskip, a2sw::num("A2AMD_VMSKIP", 1))		/* 1. Bits: a quiet kernel whose voices are all the device VM's and none idle is not launched - 1 the classes without filter12, 2 the one with */ \
	X(bool, vmspec, a2sw::on("A2AMD_VMSPEC"))		/* on. 0: no speculative device-VM pass */ \
	X(bool, vmspec_early, a2sw::on("A2AMD_VMSPEC_EARLY"))	/* on. 0: the old order - the batch's other leaf kernels and the speculative pass behind the window render passes, not between the two window passes */ \
	X(bool, vmspec_go, a2sw::on("A2AMD_VMSPEC_GO"))		/* on. 0: no event that lets the speculative pass onto the CUs ahead of the next window render pass (classes without filter12) */ \
	X(int, vmspec_min, a2sw::num("A2AMD_VMSPEC_MIN", 8))	/* 8: fragments of a batch from which the speculative pass runs */ \
	X(bool, vmwin, a2sw::on("A2AMD_VMWIN"))			/* on. 0: the device VM's voices never go through the fused window pass */ \
	X(bool, vm_dump, a2sw::set("A2AMD_VM_DUMP"))		/* unset. Set: print the records of every batch, host-made and device-made (debugging aid) */ \
	X(bool, vpw_set, a2sw::set("A2AMD_VPW")) X(int, vpw, a2sw::num("A2AMD_VPW", 0))	/* unset = pick_fast_shape(): voices per wavefront of the time-sliced leaf kernels; and, clamped to 1..64, of k_leaf_oscbare (unset: by count) */ \
	X(int, wfvpg, a2sw::within("A2AMD_WFVPG", 1, 0x7fffffff))	/* 0 = by count; > 0 forces k_win_render_f's voices per workgroup */ \
	X(int, wfwaves, a2sw::within("A2AMD_WFWAVES", 2, 0x7fffffff))	/* 0 = by voices per workgroup; > 1 forces k_win_render_f's wavefronts per workgroup */ \
	X(int, win, a2sw::set("A2AMD_WIN") ? a2sw::num("A2AMD_WIN", 0) != 0 : -1)	/* -1 = from win_min voices on; 0 ("" too) / not 0: the window kernels never / always take the voices with records */ \
	X(bool, win_check, a2sw::set("A2AMD_WIN_CHECK"))	/* unset. Set: wait for every window batch and fail at once if its pool overflowed */ \
	X(bool, win_fork, a2sw::on("A2AMD_WIN_FORK"))		/* on. 0: the lists of a one-slab window batch share one stream */ \
	X(int, win_mb, a2sw::num("A2AMD_WIN_MB", 1024))		/* 1024: MB the window slots of a batch (and of the speculative pass) may take before the batch is cut into slabs */ \
	X(int, win_min, a2sw::num("A2AMD_WIN_MIN", 2048))	/* 2048: record-carrying voices from which the window kernels take over from k_leaf_recs */ \
	X(int, win_slabs, a2sw::num1("A2AMD_WIN_SLABS", 1))	/* 1, at least 1: slabs a batch of 16 fragments or more is cut into for the window kernels */ \
	X(bool, win_sync, a2sw::set("A2AMD_WIN_SYNC"))		/* unset. Set: wait for every window launch and name it (debugging: the last line names the kernel that faulted) */ \
	X(bool, win_timing, a2sw::set("A2AMD_WIN_TIMING"))	/* unset. Set: the two window passes' times per slab on stderr (a measurement aid that waits for the GPU; one stream) */ \
	X(int, wvpw, a2sw::within("A2AMD_WVPW", 1, 0x7fffffff))	/* 0 = by count; > 0 forces k_win_render's voices per wavefront */ \
	X(bool, ysplit_set, a2sw::set("A2AMD_YSPLIT")) X(int, ysplit, a2sw::num("A2AMD_YSPLIT", 0))	/* unset = the kernel's maximum: time slices of the time-sliced leaf kernels */

struct A2Switches {
#define X(type, member, read) type member;
	A2AMD_SWITCHES(X)
#undef X
};

static inline void a2amd_read_switches(A2Switches *sw)
{
#define X(type, member, read) sw->member = read;
	A2AMD_SWITCHES(X)
#undef X
}
