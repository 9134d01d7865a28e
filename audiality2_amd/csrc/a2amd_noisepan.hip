// a2amd_noisepan.hip - k_leaf_noisepan: the quiet kernel of settled "wtosc (noise) -> panmix 1->2, wired, adding" leaf
// voices in a batch whose noise windows are seeded on the device (a2amd_fragment_repeat_noise, a2amd_noise.hip).
//
// Such a voice has no wave memory and no recurrence the lanes cannot resolve: which draw of the engine's generator a
// frame holds is a difference of two quotients of the phase, and the word after k draws is one affine map of the
// word the seed pass left in front of the window (a2amd_noisemap.h).  Lane = frame.  Lane j keeps the map of j + 1
// draws for the whole launch, makes "the window's draw j + 1" from the window's seed with one multiply-add, and every
// frame fetches the draw it holds from the lane that made it (ds_bpermute): no loop over the draws.
//
// A wavefront owns up to 64 voices (one per lane: state words, gains, output bus) for the WHOLE batch and walks its
// fragments in order - the sample a sparse oscillator holds may come from many fragments back, so the batch is not
// cut into time slices.  The bus sums of a fragment stay in registers: one atomic add per (fragment, channel, frame)
// and wavefront, flushed where the output bus changes (the list is sorted by bus: a2amd_quiet.h's bus-run walk, which
// the two quiet filter kernels' workers share).  At the end the wavefront stores
// what k_win_ctl's ctl_store would have left for the same windows - phase, held sample, generator word, the rampers
// at their targets - with plain vector stores: nobody else touches the voice during the launch.
//
// A voice with records this batch (runs[v].count != 0) is the window / records kernels' and is skipped untouched.
// The host (upload(), a2amd_sched.cpp) leaves a voice without the stand-in run only while its amplitude, volume and
// pan are at rest; a stretch of device-seeded fragments only exists while every noise oscillator's pitch is.  A voice
// that is not at rest all the same is left alone here, as one with records is.
#include <hip/hip_runtime.h>
#include "a2amd_device.h"
#include "a2amd_noisevoice.h"
#include "a2amd_quiet.h"

#define NP_WPB 4	// wavefronts per workgroup

__global__ __launch_bounds__(64 * NP_WPB)
void k_leaf_noisepan(const A2DParams *__restrict__ pp, const int *__restrict__ list, int nlist, int vpw,
		const A2DVoice *__restrict__ voices, const A2DRun *__restrict__ runs, int *ustate,
		const uint32_t *__restrict__ nseed, const int32_t *__restrict__ nslot, int nnoise, int nfrags,
		int *__restrict__ busmem)
{
	const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const int lane = threadIdx.x & 63;
	const int first = ((int)blockIdx.x * NP_WPB + wv) * vpw;
	if(first >= nlist)
		return;
	const int nv = min(vpw, nlist - first);

	// lane j: the map of j + 1 draws
	uint32_t mapA, mapC;
	a2nm_map((unsigned)lane + 1u, &mapA, &mapC);

	// lane v: voice v of this wavefront's run
	int u0 = 0, u1 = 0, my_off = -1, my_nch = 2;
	NoiseV nz = { 0, 0, 0, 0, 0, 0, 0 };
	PanRest pg = { 0, 0, 0, 0 };
	bool ok = false;
	if(lane < nv) {
		const int slot = list[first + lane];
		if(runs[slot].count == 0) {
			const A2DVoice &vc = voices[slot];
			u0 = vc.unit[0];
			u1 = vc.unit[1];
			my_off = vc.out_off;
			my_nch = vc.out_nch;
			const int *w0 = ustate + (size_t)u0 * A2D_USTATE;
			const int *w1 = ustate + (size_t)u1 * A2D_USTATE;
			nz.d = (unsigned)w0[OW_DPHASE];
			// at rest: wtosc_run_pitch returns early, and a2_PrepareRamper finds every ramper arrived
			ok = vc.nunits == 2 && my_off >= 0 && w0[OW_MODE] == A2D_OSC_NOISE && nz.d && !w0[OW_PRAMPING] &&
					a2s_at_rest(w0 + OW_P) && a2s_at_rest(w0 + OW_A) && a2s_at_rest(w1 + PW_VOL) && a2s_at_rest(w1 + PW_PAN);
			if(ok) {
				noisev_load(nz, w0, u0, nseed, nslot, nnoise);
				panrest_load(pg, w1);
			}
		}
	}
	const unsigned long long todo = __ballot(ok);
	if(!todo)
		return;
	const QuietOut out = { busmem, nullptr, false, lane };	// (a wavefront of its own: straight to the buses)

	unsigned total_frames = 0;
	for(int f = 0; f < nfrags; ++f) {
		const int n = min((int)pp->fragframes[f], A2D_FRAG);
		if(n <= 0)
			continue;
		// the generator word in front of each voice's window: the seed pass's, or - no column in this batch - the word
		// its last window left
		if(nz.col)
			nz.seed = noisev_seed(nz, nseed, f, nnoise);
		BusRun run = busrun_begin();
		const unsigned fl = (unsigned)min(lane, n - 1);	// (lanes beyond the fragment's frames: the last frame's, dropped below)
		for(unsigned long long m = todo; m; m &= m - 1) {
			const int v = (int)__builtin_ctzll(m);
			busrun_voice(run, out, f, my_off, my_nch, v);
			const int x = noisev_window(nz, v, lane, fl, n, mapA, mapC);
			if(lane < n) {
				const int y = a2nm_out(x, rdl(nz.g, v));
				run.acc0 = wadd(run.acc0, mul64s(y, rdl(pg.v0, v), 24));
				run.acc1 = wadd(run.acc1, mul64s(y, rdl(pg.v1, v), 24));
			}
		}
		busrun_end(run, out, f);
		// every voice moves on by n frames (all lanes at once)
		nz.phlo += (unsigned)n * nz.d;
		total_frames += (unsigned)n;
		pg.v0 = pg.v0r;
		pg.v1 = pg.v1r;
	}

	// state out: ctl_store's words for the same windows
	if(ok)
		noisev_store(nz, total_frames, ustate + (size_t)u0 * A2D_USTATE, ustate + (size_t)u1 * A2D_USTATE);
}

// voices per wavefront: at most 64 (one per lane)
int a2d_launch_leaf_noisepan(const A2DParams *dparams, const A2DParams &hp, const int *dlist, int nlist, int vpw, void *stream)
{
	if(nlist <= 0)
		return 0;
	vpw = vpw < 1 ? 1 : vpw > 64 ? 64 : vpw;
	const int nwaves = (nlist + vpw - 1) / vpw;
	const dim3 grid((nwaves + NP_WPB - 1) / NP_WPB), block(64 * NP_WPB);
	hipLaunchKernelGGL(k_leaf_noisepan, grid, block, 0, (hipStream_t)stream, dparams, dlist, nlist, vpw, hp.voices, hp.runs,
			hp.ustate, hp.nseed, hp.nslot, hp.nnoise, hp.nfrags, hp.busmem);
	return hipGetLastError() != hipSuccess;
}
