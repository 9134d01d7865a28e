// a2amd_noisefiltpan.hip - k_leaf_noisefiltpan: the quiet kernel of settled "wtosc (noise) -> filter12 (1 ch) -> panmix
// 1->2, wired, adding" leaf voices - the hat, snare and cymbal shape - in a batch whose noise windows are seeded on the
// device (a2amd_fragment_repeat_noise, a2amd_noise.hip).
//
// The oscillator is k_leaf_noisepan's (a2amd_noisepan.hip): no wave memory, the draw a frame holds a difference of two
// quotients of the phase, the generator word after k draws one affine map of the window's seed (a2amd_noisemap.h),
// lane = frame and no loop over the draws.  Only the filter is a recurrence in time, and it runs as in k_leaf_oscfiltpan
// (a2amd_fast.hip, "wtosc -> filter12 (1 ch) -> panmix 1->2"): lane = voice on ONE wavefront, filt_row (a2amd_filt.h).
//
// A workgroup owns up to 64 voices for the WHOLE batch and walks its fragments in order - the held sample, the generator
// word and the filter's d1 / d2 travel from fragment to fragment, so the batch is not cut into time slices.  Per
// fragment three stages meet over a ring of three [voices][64 + 1] LDS tiles, a barrier per step:
//   A(f)      workers, lane = frame: per voice the window's draws from its column of the seed table -> a2nm_out at the
//             oscillator's amplitude -> the row, already shifted (x5 = out >> 5, filter12.c:105); phase, held sample and
//             word carried in the voice's lane
//   B(f - 1)  wavefront 0, lane = voice: filt_row in place, f0 = FW_F1, df = 0, q at rest (f12_process, filter12.c:74-119)
//   C(f - 2)  workers, lane = frame: the rows x the two panmix gains, summed over the voices of one output bus (the list
//             is sorted by bus).  Where all the workgroup's voices mix into ONE stereo bus - the usual case - the workers'
//             sums meet in LDS (a ring of three like the tiles) and
//   D(f - 3)  the idle wavefront adds the workgroup's total to the bus in device memory: one atomic add per (fragment,
//             channel, frame) and workgroup, as k_leaf_oscfiltpan does it.  A workgroup that spans several buses adds
//             per worker and bus run instead.
// Steps 0 and 1 are the pipeline's prologue (A only, A + B), the three steps behind the last fragment its epilogue.
// At the end the voice's words are stored as k_win_ctl's ctl_store would have left them for the same windows, with plain
// vector stores - the oscillator's and the panmix's by the worker that carried them, the filter's by wavefront 0.
//
// A voice with records this batch (runs[v].count != 0) is the window / records kernels' and is skipped untouched.  The
// host (upload(), a2amd_sched.cpp) leaves a voice without the stand-in run only while amplitude, q, volume and pan are at
// rest and no filter of it has a column of the batch's sweep table (a cutoff sweeping in a stretch: a2d_cut_coeff); a
// stretch of device-seeded fragments only exists while every noise oscillator's pitch is at rest.  A
// voice that is not at rest all the same is left alone here, as one with records is: every wavefront of the workgroup
// reads the same words and comes to the same answer.
#include <hip/hip_runtime.h>
#include "a2amd_device.h"
#include "a2amd_noisevoice.h"
#include "a2amd_filt.h"

#define NFP_MAXV  64	// voices per workgroup: the lanes of the filter wavefront
#define NFP_PITCH 65	// (+1: row and column accesses both bank-conflict free)
// Wavefronts per workgroup: 8 = the filter wavefront, six workers, one idle.
// The step: a pipeline step is as long as the filter wavefront's chain of dependent instructions - 64 frames x 12 (pure
// low pass) to 15 instructions, 770 - 960 issues one behind the other, about 4 600 cycles (a2amd_fast.hip) - whatever the
// number of busy lanes.  A + C cost a worker about 50 vector instructions per voice and fragment (A: five lane reads, the
// map's multiply-add, the value, the draw count, ds_bpermute, three selects, the amplitude, the tile store, ~35; C: the
// tile load, two 64-bit products, two adds, ~15), 200 cycles of its SIMD.  64 voices over six workers are 11 each, two
// workers per SIMD: 22 x 200 = 4 400 cycles - below the filter's chain; with three workers (4 wavefronts) a SIMD would
// carry 21 - 22 voices alone, the same, but nothing would overlap the workers' own LDS and lane-read latencies.  Where a
// wavefront runs is the hardware's choice; wavefronts w and w + 4 of a workgroup were observed to share a SIMD
// (a2amd_fast.hip), so wavefront 4 takes no voices and leaves the filter's SIMD to the filter.
// LDS: three tiles of 64 x 65 words are 49 920 bytes, the bus sums 1 536 more - three workgroups fit the 160 KB of a CU, which is what the launcher
// relies on once there are more than 256 workgroups; 16 wavefronts per workgroup would not buy more (one filter wavefront
// per 64 voices either way) and would leave a CU two workgroups at most.
#define NFP_WAVES 8
#define NFP_WORKERS 6

__global__ __launch_bounds__(64 * NFP_WAVES)
void k_leaf_noisefiltpan(const A2DParams *__restrict__ pp, const int *__restrict__ list, int nlist, int vpg,
		const A2DVoice *__restrict__ voices, const A2DRun *__restrict__ runs, int *ustate,
		const uint32_t *__restrict__ nseed, const int32_t *__restrict__ nslot, int nnoise, int nfrags,
		int *__restrict__ busmem)
{
	extern __shared__ __attribute__((aligned(16))) int nf_tiles[];	// 3 x [vpg][NFP_PITCH]
	const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const int lane = threadIdx.x & 63;
	const int first = (int)blockIdx.x * vpg;
	const int nv = min(vpg, nlist - first);
	if(nv <= 0)
		return;		// (the whole workgroup: the grid has none such)
	const int tsize = vpg * NFP_PITCH;

	// lane v: voice v of this workgroup, in every wavefront
	int u0 = 0, u1 = 0, u2 = 0, my_off = -1, my_nch = 2;
	NoiseV nz = { 0, 0, 0, 0, 0, 0, 0 };
	int v0_l = 0, v1_l = 0, v0r_l = 0, v1r_l = 0;
	int qt_l = 0, ff_l = 0, lp_l = 0, bp_l = 0, hp_l = 0, d1_l = 0, d2_l = 0;
	bool ok = false;
	if(lane < nv) {
		const int slot = list[first + lane];
		if(runs[slot].count == 0) {
			const A2DVoice &vc = voices[slot];
			u0 = vc.unit[0];
			u1 = vc.unit[1];
			u2 = vc.unit[2];
			my_off = vc.out_off;
			my_nch = vc.out_nch;
			const int *w0 = ustate + (size_t)u0 * A2D_USTATE;
			const int *w1 = ustate + (size_t)u1 * A2D_USTATE;
			const int *w2 = ustate + (size_t)u2 * A2D_USTATE;
			nz.d = (unsigned)w0[OW_DPHASE];
			// at rest: wtosc_run_pitch returns early, a2_PrepareRamper finds every ramper arrived, no R_F1RAMP is pending
			ok = vc.nunits == 3 && my_off >= 0 && w0[OW_MODE] == A2D_OSC_NOISE && nz.d && !w0[OW_PRAMPING] &&
					a2s_at_rest(w0 + OW_P) && a2s_at_rest(w0 + OW_A) && a2s_at_rest(w1 + FW_Q) && !w1[FW_RAMP] &&
					a2s_at_rest(w2 + PW_VOL) && a2s_at_rest(w2 + PW_PAN);
			if(ok) {
				noisev_load(nz, w0, u0, nseed, nslot, nnoise);
				// f12_process's loop constants (filter12.c:99-100) with the q ramper at its target
				qt_l = w1[FW_Q + 1];
				ff_l = w1[FW_F1] >> 12;
				lp_l = w1[FW_LP]; bp_l = w1[FW_BP]; hp_l = w1[FW_HP];
				d1_l = w1[FW_D1A];
				d2_l = w1[FW_D2A];
				// panmix_process12's two gains as k_leaf_noisepan derives them.  Whether they are clamped is decided in front of
				// a2_PrepareRamper (panmix.c:120-124): the first window still sees the value a finished ramp stopped at, the
				// others the target
				const int vol = w2[PW_VOL + 1], pan = w2[PW_PAN + 1];
				const bool cr = a2s_pan_over(pan), c0 = cr || a2s_pan_over(w2[PW_PAN]);
				a2s_pan_gains(vol, pan, c0, &v0_l, &v1_l);
				a2s_pan_gains(vol, pan, cr, &v0r_l, &v1r_l);
			}
		}
	}
	const unsigned long long todo = __ballot(ok);
	if(!todo)
		return;		// (the whole workgroup)
	// The row format of the batch (filt_step): pure low pass filters in the whole workgroup leave l in the rows and the pan
	// stage applies lp - 12 dependent instructions per frame instead of 15.
	const bool lpraw = __all(!ok || (bp_l == 0 && hp_l == 0));
	// the workgroup's share of its bus, fragment by fragment, where it has one bus (stage D)
	__shared__ int nf_acc[3][2][A2D_FRAG];
	const int wg_off = rdl(my_off, (int)__builtin_ctzll(todo));
	const bool wgbus = __all(!ok || (my_off == wg_off && my_nch == 2));
	const int nsteps = nfrags + 3;

	if(wv == 0) {
		// ================= the filter wavefront: lane = voice =================
		__builtin_amdgcn_s_setprio(3);
		for(int st = 0; st < nsteps; ++st) {
			const int f = st - 1;
			if(f >= 0 && f < nfrags) {
				const int n = min((int)pp->fragframes[f], A2D_FRAG);
				if(n > 0 && ok) {
					int *row = nf_tiles + (f % 3) * tsize + lane * NFP_PITCH;
					int qv = qt_l;
					if(lpraw)
						filt_row<true, true>(row, n, ff_l, lp_l, bp_l, hp_l, d1_l, d2_l, qv, 0);
					else
						filt_row<false, true>(row, n, ff_l, lp_l, bp_l, hp_l, d1_l, d2_l, qv, 0);
				}
			}
			filt_barrier();
		}
		// state out: the filter's words as ctl_store / k_win_render_f leave them
		if(ok) {
			int *w1 = ustate + (size_t)u1 * A2D_USTATE;
			ramp_settle(w1 + FW_Q);
			w1[FW_D1A] = d1_l;
			w1[FW_D2A] = d2_l;
		}
		return;
	}

	// ================= workers: lane = frame, voices [vb, ve) of the workgroup =================
	const int widx = wv < 4 ? wv - 1 : wv - 2;	// (wavefront 4 shares the filter's SIMD: no voices)
	int vb = 0, ve = 0;
	if(wv != 4) {
		const int per = nv / NFP_WORKERS, extra = nv % NFP_WORKERS;
		vb = widx * per + min(widx, extra);
		ve = vb + per + (widx < extra ? 1 : 0);
	}
	// my voices among the ones to render
	unsigned long long mine = 0;
	if(ve > vb)
		mine = todo & ((ve >= 64 ? ~0ull : ((1ull << ve) - 1ull)) & ~((1ull << vb) - 1ull));
	// (wave-uniform, and known to the compiler as such)
	mine = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)mine) |
			((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(mine >> 32)) << 32);
	const bool mylane = (mine >> lane) & 1ull;

	// lane j: the map of j + 1 draws
	uint32_t mapA, mapC;
	a2nm_map((unsigned)lane + 1u, &mapA, &mapC);

	if(wv == 4 && wgbus) {	// (first used in step 2: two barriers away)
		for(int k = lane; k < 3 * 2 * A2D_FRAG; k += 64)
			(&nf_acc[0][0][0])[k] = 0;
	}
	// one fragment's sums of this wavefront's bus run
	auto bus_add = [&](int off, int nch, int f, int acc0, int acc1) __attribute__((always_inline)) {
		if(wgbus) {
			if(acc0) atomicAdd(&nf_acc[f % 3][0][lane], acc0);
			if(acc1) atomicAdd(&nf_acc[f % 3][1][lane], acc1);
		} else {
			int *dst = busmem + off + (size_t)f * nch * A2D_FRAG;
			if(acc0) atomicAdd(&dst[lane], acc0);
			if(acc1) atomicAdd(&dst[A2D_FRAG + lane], acc1);
		}
	};

	unsigned total_frames = 0;
	bool cfirst = true;	// stage C has not met a window yet: the first one's gains
	for(int st = 0; st < nsteps; ++st) {
		// ---- D(st - 3): the workgroup's sum of a fragment, complete since the last barrier ----
		if(wv == 4 && wgbus && st >= 3) {
			const int f = st - 3;
			if((int)pp->fragframes[f] > 0) {
				const int a0 = nf_acc[f % 3][0][lane], a1 = nf_acc[f % 3][1][lane];
				nf_acc[f % 3][0][lane] = 0;
				nf_acc[f % 3][1][lane] = 0;
				int *dst = busmem + wg_off + (size_t)f * 2 * A2D_FRAG;
				if(a0) atomicAdd(&dst[lane], a0);
				if(a1) atomicAdd(&dst[A2D_FRAG + lane], a1);
			}
		}
		// ---- A(st) ----
		if(st < nfrags && mine) {
			const int f = st;
			const int n = min((int)pp->fragframes[f], A2D_FRAG);
			if(n > 0) {
				// the generator word in front of each voice's window: the seed pass's, or - no column in this batch - the
				// word its last window left
				if(nz.col && mylane)
					nz.seed = noisev_seed(nz, nseed, f, nnoise);
				int *tile = nf_tiles + (f % 3) * tsize;
				const unsigned fl = (unsigned)min(lane, n - 1);	// (lanes beyond the fragment's frames: the last frame's, stored as 0)
				for(unsigned long long m = mine; m; m &= m - 1) {
					const int v = (int)__builtin_ctzll(m);
					const int x = noisev_window(nz, v, lane, fl, n, mapA, mapC);
					// wtosc.c:148 at the amplitude, filter12.c:105's shift
					const int y = a2nm_out(x, rdl(nz.g, v));
					tile[v * NFP_PITCH + lane] = lane < n ? y >> 5 : 0;
				}
				// every voice moves on by n frames (all lanes at once)
				nz.phlo += (unsigned)n * nz.d;
				total_frames += (unsigned)n;
			}
		}
		// ---- C(st - 2) ----
		if(st >= 2 && st - 2 < nfrags && mine) {
			const int f = st - 2;
			const int n = min((int)pp->fragframes[f], A2D_FRAG);
			if(n > 0) {
				const int *tile = nf_tiles + (f % 3) * tsize;
				int acc0 = 0, acc1 = 0;
				int cur_off = -1, cur_nch = 2;
				for(unsigned long long m = mine; m; m &= m - 1) {
					const int v = (int)__builtin_ctzll(m);
					const int voff = rdl(my_off, v);
					if(voff != cur_off) {
						if(cur_off >= 0)
							bus_add(cur_off, cur_nch, f, acc0, acc1);
						acc0 = acc1 = 0;
						cur_off = voff;
						cur_nch = rdl(my_nch, v);
					}
					int y = tile[v * NFP_PITCH + lane];
					if(lpraw)
						y = wmul(y, rdl(lp_l, v)) >> 3;	// (filt_step: the row holds l)
					if(lane < n) {
						acc0 = wadd(acc0, mul64s(y, rdl(cfirst ? v0_l : v0r_l, v), 24));
						acc1 = wadd(acc1, mul64s(y, rdl(cfirst ? v1_l : v1r_l, v), 24));
					}
				}
				if(cur_off >= 0)
					bus_add(cur_off, cur_nch, f, acc0, acc1);
				cfirst = false;
			}
		}
		filt_barrier();
	}

	// state out: ctl_store's words for the same windows
	if(mylane)
		noisev_store(nz, total_frames, ustate + (size_t)u0 * A2D_USTATE, ustate + (size_t)u2 * A2D_USTATE);
}

// voices per workgroup: at most NFP_MAXV (one per lane of the filter wavefront)
int a2d_launch_leaf_noisefiltpan(const A2DParams *dparams, const A2DParams &hp, const int *dlist, int nlist, int vpg, void *stream)
{
	if(nlist <= 0)
		return 0;
	vpg = vpg < 1 ? 1 : vpg > NFP_MAXV ? NFP_MAXV : vpg;
	const dim3 grid((nlist + vpg - 1) / vpg), block(64 * NFP_WAVES);
	const size_t dyn = (size_t)3 * vpg * NFP_PITCH * sizeof(int);
	hipLaunchKernelGGL(k_leaf_noisefiltpan, grid, block, dyn, (hipStream_t)stream, dparams, dlist, nlist, vpg, hp.voices, hp.runs,
			hp.ustate, hp.nseed, hp.nslot, hp.nnoise, hp.nfrags, hp.busmem);
	return hipGetLastError() != hipSuccess;
}
