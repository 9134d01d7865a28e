// a2amd_quiet.h - the skeleton the quiet leaf kernels share: k_leaf_noisepan (a2amd_noisepan.hip), k_leaf_noisefiltpan
// (a2amd_noisefiltpan.hip), k_leaf_oscbare (a2amd_oscbare.hip) and k_leaf_osc3filtpan / k_leaf_osc3filtpan_win
// (a2amd_osc3filtpan.hip).  The one statement of: how the filter kernels' workgroup deals its voices to its worker
// wavefronts (for a host compiler too: tests/test_quiet_header.py pins it), the shape their launchers launch
// (quiet_launch), the facts every wavefront of such a workgroup derives from the same words, how the pan stage reads a
// filtered row (quiet_row), where a worker's bus sums go and how a walk over the bus-sorted list cuts them into runs, and
// one oscillator's pair of window taps.  The stages themselves differ from kernel to kernel and stay in the kernels;
// the stages the two three-oscillator kernels share with each other alone stand once in a2amd_osc3filtpan.hip.
#pragma once
#include <stdint.h>
#include "a2amd_settled.h"	// (A2S: for the host and the device alike)

// ---- The filter kernels' workgroup: one filter wavefront (lane = voice), six workers, one wavefront that only adds the
// workgroup's sums to the bus ----
#define QUIET_MAXV  64	// voices per workgroup: the lanes of the filter wavefront
#define QUIET_PITCH 65	// words per tile row (+1: row and column accesses both bank-conflict free)
// Wavefronts per workgroup: 8 = the filter wavefront, six workers, one idle.
// The step: a pipeline step is as long as the filter wavefront's chain of dependent instructions - 64 frames x 12 (pure
// low pass) to 15 instructions, 770 - 960 issues one behind the other, about 4 600 cycles (a2amd_fast.hip) - whatever the
// number of busy lanes.  In k_leaf_noisefiltpan, A + C cost a worker about 50 vector instructions per voice and fragment
// (A: five lane reads, the map's multiply-add, the value, the draw count, ds_bpermute, three selects, the amplitude, the
// tile store, ~35; C: the tile load, two 64-bit products, two adds, ~15), 200 cycles of its SIMD.  64 voices over six
// workers are 11 each, two workers per SIMD: 22 x 200 = 4 400 cycles - below the filter's chain; with three workers (4
// wavefronts) a SIMD would carry 21 - 22 voices alone, the same, but nothing would overlap the workers' own LDS and
// lane-read latencies.  Where a wavefront runs is the hardware's choice; wavefronts w and w + 4 of a workgroup were
// observed to share a SIMD (a2amd_fast.hip), so wavefront 4 takes no voices and leaves the filter's SIMD to the filter.
// LDS: three tiles of 64 x 65 words are 49 920 bytes, the bus sums 1 536 more - three workgroups fit the 160 KB of a CU,
// which is what k_leaf_noisefiltpan's launcher relies on once there are more than 256 workgroups; 16 wavefronts per
// workgroup would not buy more (one filter wavefront per 64 voices either way) and would leave a CU two workgroups at most.
#define QUIET_WAVES 8
#define QUIET_WORKERS 6

// The voices wavefront wv of a workgroup of nv voices renders, as a mask over the workgroup's voices, among the ones to
// render (todo).  The workers are wavefronts 1, 2, 3, 5, 6, 7 in this order; worker k has the k-th of six ranges of the
// list, in list order (the bus-run walk relies on it), the first nv % 6 of them one voice longer.  The filter wavefront
// (0) renders none, and neither does wavefront 4: it shares the filter's SIMD.
A2S uint64_t a2q_worker_voices(int wv, int nv, uint64_t todo)
{
	if(wv <= 0 || wv == 4 || wv >= QUIET_WAVES)
		return 0;
	const int widx = wv < 4 ? wv - 1 : wv - 2;
	const int per = nv / QUIET_WORKERS, extra = nv % QUIET_WORKERS;
	const int vb = widx * per + (widx < extra ? widx : extra);
	const int ve = vb + per + (widx < extra ? 1 : 0);
	if(ve <= vb)
		return 0;
	return todo & ((ve >= 64 ? ~0ull : ((1ull << ve) - 1ull)) & ~((1ull << vb) - 1ull));
}

#ifdef __HIPCC__
#include "a2amd_dsp.h"
#include "a2amd_taps.h"
#include "a2amd_winctl.h"

// ... wave-uniform, and known to the compiler as such
DEV unsigned long long quiet_worker_voices(int wv, int nv, unsigned long long todo)
{
	const unsigned long long mine = a2q_worker_voices(wv, nv, todo);
	return (unsigned long long)(unsigned)rfl((int)(unsigned)mine) | ((unsigned long long)(unsigned)rfl((int)(unsigned)(mine >> 32)) << 32);
}

// The filter kernels' launch over a list of nlist voices: vpg voices per workgroup, at most QUIET_MAXV (one per lane of
// the filter wavefront); the ring of three [vpg][QUIET_PITCH] tiles is the dynamic LDS.  Every such kernel's arguments
// begin (params, list, nlist, vpg); rest: the ones behind them.  Returns nonzero where the launch failed.
template<typename Kernel, typename... Rest>
static inline int quiet_launch(Kernel kernel, const A2DParams *dparams, const int *dlist, int nlist, int vpg, void *stream, Rest... rest)
{
	if(nlist <= 0)
		return 0;
	vpg = vpg < 1 ? 1 : vpg > QUIET_MAXV ? QUIET_MAXV : vpg;
	hipLaunchKernelGGL(kernel, dim3((nlist + vpg - 1) / vpg), dim3(64 * QUIET_WAVES), (size_t)3 * vpg * QUIET_PITCH * sizeof(int),
			(hipStream_t)stream, dparams, dlist, nlist, vpg, rest...);
	return hipGetLastError() != hipSuccess;
}

// What every wavefront of the workgroup derives from the same words, lane = voice (ok: the voice is this kernel's; bp, hp:
// its filter's band and high pass gains; off, nch: its output bus): the voices to render; the row format of the batch
// (filt_step) - pure low pass filters in the whole workgroup leave l in the rows and the pan stage applies lp, 12
// dependent instructions per frame instead of 15; whether all the voices mix into ONE stereo bus, at wg_off (stage D).
// Nothing but todo is set where there is no voice to render: the whole workgroup returns.
struct QuietWg { unsigned long long todo; bool lpraw, wgbus; int wg_off; };

DEV QuietWg quiet_wg(bool ok, int bp, int hp, int off, int nch)
{
	QuietWg g = { __ballot(ok), false, false, -1 };
	if(g.todo) {
		g.lpraw = __all(!ok || (bp == 0 && hp == 0));
		g.wg_off = rdl(off, (int)__builtin_ctzll(g.todo));
		g.wgbus = __all(!ok || (off == g.wg_off && nch == 2));
	}
	return g;
}

// The pan stage's read of voice v's filtered row, lane = frame (lp: lane v's low pass gain): where the row holds l (lpraw,
// filt_step) the scaling the filter wavefront left out
DEV int quiet_row(const int *tile, int v, int lane, bool lpraw, int lp)
{
	const int y = tile[v * QUIET_PITCH + lane];
	return lpraw ? wmul(y, rdl(lp, v)) >> 3 : y;
}

// ---- Bus sums, lane = frame ----
// one fragment's two channels into a stereo pair of rows
DEV void quiet_pair_add(int *dst, int lane, int acc0, int acc1)
{
	if(acc0) atomicAdd(&dst[lane], acc0);
	if(acc1) atomicAdd(&dst[A2D_FRAG + lane], acc1);
}

// the workgroup's share of its bus, fragment by fragment, where it has one bus: a ring of three like the tiles
typedef int QuietBus[3][2][A2D_FRAG];

DEV void quiet_bus_clear(QuietBus &ring, int k0, int stride)
{
	for(int k = k0; k < 3 * 2 * A2D_FRAG; k += stride)
		(&ring[0][0][0])[k] = 0;
}

// stage D: the workgroup's sum of fragment f, complete since the last barrier, to the bus in device memory
DEV void quiet_bus_flush(QuietBus &ring, int *busmem, int wg_off, int f, int lane)
{
	const int a0 = ring[f % 3][0][lane], a1 = ring[f % 3][1][lane];
	ring[f % 3][0][lane] = 0;
	ring[f % 3][1][lane] = 0;
	quiet_pair_add(busmem + wg_off + (size_t)f * 2 * A2D_FRAG, lane, a0, a1);
}

// atomicAdd() on a word of the ring, its address space stated: the ring reaches the workers through a pointer, and with a
// generic one the compiler merges this add and the one to device memory into one flat atomic
DEV void quiet_lds_add(int *p, int x)
{
	__hip_atomic_fetch_add((__attribute__((address_space(3))) int *)p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// where a wavefront's sums go: the workgroup's ring (wgbus) or straight to the buses in device memory
struct QuietOut { int *busmem; QuietBus *ring; bool wgbus; int lane; };

// one fragment's sums of a run of voices on the bus at off
DEV void quiet_out_add(const QuietOut &o, int off, int nch, int f, int acc0, int acc1)
{
	if(o.wgbus) {
		if(acc0) quiet_lds_add(&(*o.ring)[f % 3][0][o.lane], acc0);
		if(acc1) quiet_lds_add(&(*o.ring)[f % 3][1][o.lane], acc1);
	} else
		quiet_pair_add(o.busmem + off + (size_t)f * nch * A2D_FRAG, o.lane, acc0, acc1);
}

// The walk over the voices of a wavefront in list order (sorted by bus; neighbouring buses may have different channel
// counts): the sums of the current run of voices on one bus.
struct BusRun { int off, nch, acc0, acc1; };

DEV BusRun busrun_begin() { return BusRun{ -1, 2, 0, 0 }; }

// in front of voice v's share (lane v of off / nch: its bus): the bus differs from the current run's - flush, restart
DEV void busrun_voice(BusRun &r, const QuietOut &o, int f, int off, int nch, int v)
{
	const int voff = rdl(off, v);
	if(voff != r.off) {
		if(r.off >= 0)
			quiet_out_add(o, r.off, r.nch, f, r.acc0, r.acc1);
		r.acc0 = r.acc1 = 0;
		r.off = voff;
		r.nch = rdl(nch, v);
	}
}

DEV void busrun_end(const BusRun &r, const QuietOut &o, int f)
{
	if(r.off >= 0)
		quiet_out_add(o, r.off, r.nch, f, r.acc0, r.acc1);
}

// ---- One oscillator's two taps of a frame, issued (win_taps_issue's words for one oscillator); all zero for an
// oscillator that is silent in the window: it then comes out as 0 ----
struct OscTaps { Coef4 k1, k2; unsigned t1, t2; int ak, da; };

DEV void osctaps_clear(OscTaps &T)
{
	T.k1 = T.k2 = Coef4{ 0, 0, 0 };
	T.t1 = T.t2 = 0;
	T.ak = T.da = 0;
}

// voice v's window words (osc_window_v) out of the lanes; where this lane's frame fl reads the wave; the loads
DEV void osctaps_issue(const int (&w)[6], int v, const CoefRsrc rs, unsigned fl, OscTaps &T)
{
	const unsigned phlo = (unsigned)rdl(w[WO_B], v), phhi = (unsigned)rdl(w[WO_C], v), dph = (unsigned)rdl(w[WO_DPH], v);
	const int cb = coef_base((unsigned)rdl(w[WO_A], v));
	T.ak = rdl(w[WO_AK], v);
	T.da = rdl(w[WO_DA], v);
	T.t1 = tap_phase((uint64_t)phlo | ((uint64_t)phhi << 32), fl * dph);
	T.t2 = T.t1 + ((dph >> 16) >> 1);
	T.k1 = coef_at(rs, cb, T.t1);
	T.k2 = coef_at(rs, cb, T.t2);
}

// wtosc_do_fragment's sample of frame fl, wtosc.c:227-229 (the amplitude ramper run frame by frame)
DEV int osctaps_finish(const OscTaps &T, unsigned fl)
{
	const int h = inter_coefs(T.k1, T.t1, T.k2, T.t2);
	return mul64s(h, wadd(T.ak, wmul(T.da, (int)fl)), 17);
}
#endif /* __HIPCC__ */
