// a2amd_noisefiltpan.hip - k_leaf_noisefiltpan: the quiet kernel of settled "wtosc (noise) -> filter12 (1 ch) -> panmix
// 1->2, wired, adding" leaf voices - the hat, snare and cymbal shape - in a batch whose noise windows are seeded on the
// device (a2amd_fragment_repeat_noise, a2amd_noise.hip).
//
// The oscillator is k_leaf_noisepan's (a2amd_noisepan.hip): no wave memory, the draw a frame holds a difference of two
// quotients of the phase, the generator word after k draws one affine map of the window's seed (a2amd_noisemap.h),
// lane = frame and no loop over the draws.  Only the filter is a recurrence in time, and it runs as in k_leaf_oscfiltpan
// (a2amd_fast.hip, "wtosc -> filter12 (1 ch) -> panmix 1->2"): lane = voice on ONE wavefront, filt_row (a2amd_filt.h).
//
// The workgroup - its constants, the split of its voices over the workers, the facts every wavefront derives alike, the
// bus sums and the bus-run walk - is a2amd_quiet.h's, shared with k_leaf_osc3filtpan.  It owns up to 64 voices for the
// WHOLE batch and walks its fragments in order - the held sample, the generator word and the filter's d1 / d2 travel from
// fragment to fragment, so the batch is not cut into time slices.  Per
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
#include "a2amd_quiet.h"

__global__ __launch_bounds__(64 * QUIET_WAVES)
void k_leaf_noisefiltpan(const A2DParams *__restrict__ pp, const int *__restrict__ list, int nlist, int vpg,
		const A2DVoice *__restrict__ voices, const A2DRun *__restrict__ runs, int *ustate,
		const uint32_t *__restrict__ nseed, const int32_t *__restrict__ nslot, int nnoise, int nfrags,
		int *__restrict__ busmem)
{
	extern __shared__ __attribute__((aligned(16))) int nf_tiles[];	// 3 x [vpg][QUIET_PITCH]
	const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const int lane = threadIdx.x & 63;
	const int first = (int)blockIdx.x * vpg;
	const int nv = min(vpg, nlist - first);
	if(nv <= 0)
		return;		// (the whole workgroup: the grid has none such)
	const int tsize = vpg * QUIET_PITCH;

	// lane v: voice v of this workgroup, in every wavefront
	int u0 = 0, u1 = 0, u2 = 0, my_off = -1, my_nch = 2;
	NoiseV nz = { 0, 0, 0, 0, 0, 0, 0 };
	PanRest pg = { 0, 0, 0, 0 };
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
				panrest_load(pg, w2);
			}
		}
	}
	const QuietWg wg = quiet_wg(ok, bp_l, hp_l, my_off, my_nch);
	if(!wg.todo)
		return;		// (the whole workgroup)
	const bool lpraw = wg.lpraw, wgbus = wg.wgbus;
	__shared__ QuietBus nf_acc;
	const int nsteps = nfrags + 3;

	if(wv == 0) {
		// ================= the filter wavefront: lane = voice =================
		__builtin_amdgcn_s_setprio(3);
		for(int st = 0; st < nsteps; ++st) {
			const int f = st - 1;
			if(f >= 0 && f < nfrags) {
				const int n = min((int)pp->fragframes[f], A2D_FRAG);
				if(n > 0 && ok) {
					int *row = nf_tiles + (f % 3) * tsize + lane * QUIET_PITCH;
					int qv = qt_l;
					filt_row_pick(lpraw, true, row, n, ff_l, lp_l, bp_l, hp_l, d1_l, d2_l, qv, 0);
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

	// ================= workers: lane = frame, a range of the workgroup's voices each =================
	const unsigned long long mine = quiet_worker_voices(wv, nv, wg.todo);	// (wavefront 4: none)
	const bool mylane = (mine >> lane) & 1ull;

	// lane j: the map of j + 1 draws
	uint32_t mapA, mapC;
	a2nm_map((unsigned)lane + 1u, &mapA, &mapC);

	if(wv == 4 && wgbus)	// (first used in step 2: two barriers away)
		quiet_bus_clear(nf_acc, lane, 64);
	const QuietOut out = { busmem, &nf_acc, wgbus, lane };

	unsigned total_frames = 0;
	bool cfirst = true;	// stage C has not met a window yet: the first one's gains
	for(int st = 0; st < nsteps; ++st) {
		// ---- D(st - 3): the workgroup's sum of a fragment, complete since the last barrier ----
		if(wv == 4 && wgbus && st >= 3) {
			const int f = st - 3;
			if((int)pp->fragframes[f] > 0)
				quiet_bus_flush(nf_acc, busmem, wg.wg_off, f, lane);
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
					tile[v * QUIET_PITCH + lane] = lane < n ? y >> 5 : 0;
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
				BusRun run = busrun_begin();
				for(unsigned long long m = mine; m; m &= m - 1) {
					const int v = (int)__builtin_ctzll(m);
					busrun_voice(run, out, f, my_off, my_nch, v);
					const int y = quiet_row(tile, v, lane, lpraw, lp_l);
					if(lane < n) {
						run.acc0 = wadd(run.acc0, mul64s(y, rdl(cfirst ? pg.v0 : pg.v0r, v), 24));
						run.acc1 = wadd(run.acc1, mul64s(y, rdl(cfirst ? pg.v1 : pg.v1r, v), 24));
					}
				}
				busrun_end(run, out, f);
				cfirst = false;
			}
		}
		filt_barrier();
	}

	// state out: ctl_store's words for the same windows
	if(mylane)
		noisev_store(nz, total_frames, ustate + (size_t)u0 * A2D_USTATE, ustate + (size_t)u2 * A2D_USTATE);
}

int a2d_launch_leaf_noisefiltpan(const A2DParams *dparams, const A2DParams &hp, const int *dlist, int nlist, int vpg, void *stream)
{
	return quiet_launch(k_leaf_noisefiltpan, dparams, dlist, nlist, vpg, stream, hp.voices, hp.runs, hp.ustate, hp.nseed, hp.nslot,
			hp.nnoise, hp.nfrags, hp.busmem);
}
