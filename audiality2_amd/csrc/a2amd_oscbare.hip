// a2amd_oscbare.hip - k_leaf_oscbare: the quiet kernel of bare "wtosc, wired, adding" leaf voices - the chain of
// `struct { wtosc }`, one oscillator that adds straight into channel 0 of its parent's bus, no panmix behind it - in
// the batches in which they carry no record.
//
// Ownership is k_leaf_noisepan's (a2amd_noisepan.hip): a wavefront owns up to 64 voices of its run of the list, one per
// lane, for the WHOLE batch and walks the fragments in order - no time slices, no staged commit, no slots in memory.
// The arithmetic is the window kernels' (a2amd_win.hip).  Once per fragment, lane = voice, osc_window_v()
// (a2amd_winctl.h) steps the oscillator's control state over the window - pitch and amplitude rampers, mip level, the
// wrap of a looped wave, a one-shot wave's end, a pitch out of range, an unloaded wave - and leaves the closed-form
// words k_win_render renders from; then, lane = frame, the voices that play take their turn: the words out of the lanes
// with v_readlane, two coefficient-table taps as win_taps_issue / win_oscs_finish take them (a2amd_quiet.h's OscTaps,
// shared with k_leaf_osc3filtpan), the next voice's loads
// issued before this one's arithmetic.  The sum of the wavefront's voices stays in a register: one atomic add per
// (fragment, frame) and wavefront into channel 0, flushed where the output bus changes (the list is sorted by bus;
// neighbouring buses may have different channel counts).  At the end the wavefront stores every OW_* word of its voices
// with plain stores - what ctl_store would have left for the same windows: nobody else touches them during the launch.
//
// A gliding voice is this kernel's too (the host gives the class no stand-in record): the rampers are stepped here.
// A voice with records this batch (runs[v].count != 0) is the general kernel's and is skipped untouched, and so is an
// oscillator on the noise generator: every window of one carries a record or the stand-in run (upload()).
#include <hip/hip_runtime.h>
#include "a2amd_device.h"
#include "a2amd_dsp.h"
#include "a2amd_taps.h"
#include "a2amd_winctl.h"
#include "a2amd_quiet.h"

#define OB_WPB 4	// wavefronts per workgroup

__global__ __launch_bounds__(64 * OB_WPB)
void k_leaf_oscbare(const A2DParams *__restrict__ pp, const int *__restrict__ list, int nlist, int vpw,
		const A2DVoice *__restrict__ voices, const A2DRun *__restrict__ runs, int *ustate,
		const A2DWave *__restrict__ waves, const uint32_t *__restrict__ ptab, const int *__restrict__ wavecoef,
		int nfrags, int *__restrict__ busmem)
{
	// the pitch table: read in every window of a gliding voice, from LDS (as k_win_ctl)
	__shared__ PTab s_ptab;
	for(int k = (int)threadIdx.x; k < 128; k += 64 * OB_WPB)
		s_ptab[k] = ptab[k];
	__syncthreads();
	const int wv = rfl((int)(threadIdx.x >> 6));
	const int lane = threadIdx.x & 63;
	const int first = ((int)blockIdx.x * OB_WPB + wv) * vpw;
	if(first >= nlist)
		return;
	const int nv = min(vpw, nlist - first);

	// lane v: voice v of this wavefront's run, loaded as ctl_load loads an oscillator
	OscV o;
	oscv_clear(o);
	o.cmm = -2;
	int u0 = 0, my_off = -1, my_nch = 1;
	bool ok = false;
	if(lane < nv) {
		const int slot = list[first + lane];
		if(runs[slot].count == 0) {
			const A2DVoice &vc = voices[slot];
			u0 = vc.unit[0];
			my_off = vc.out_off;
			my_nch = vc.out_nch;
			oscv_load(o, ustate + (size_t)u0 * A2D_USTATE);
			ok = vc.nunits == 1 && my_off >= 0 && my_nch >= 1 && (o.mode == A2D_OSC_MIPWAVE || o.mode == A2D_OSC_OFF);
		}
	}
	const unsigned long long todo = __ballot(ok);
	if(!todo)
		return;
	const CoefRsrc rs = coef_rsrc(wavecoef);

	for(int f = 0; f < nfrags; ++f) {
		const int n = min((int)pp->fragframes[f], A2D_FRAG);
		if(n <= 0)
			continue;
		// control, lane = voice: the window's words and what its frames are made of
		int w[6] = { 0, 0, 0, 0, 0, 0 };
		int mode = WM_SILENT;
		if(ok)
			mode = osc_window_v(waves, s_ptab, o, n, w);
		unsigned long long m = todo & __ballot(mode == WM_TAPS);
		if(!m)
			continue;
		// render, lane = frame.  (lanes beyond the fragment's frames: the last frame's address, their share dropped)
		const unsigned fl = (unsigned)min(lane, n - 1);
		const bool in = lane < n;
		int acc = 0, cur_off = -1, cur_nch = 1;
		int k = (int)__builtin_ctzll(m);
		m &= m - 1;
		OscTaps T0;
		osctaps_issue(w, k, rs, fl, T0);
		for(;;) {
			const int kn = m ? (int)__builtin_ctzll(m) : -1;
			OscTaps T1;
			if(kn >= 0)
				osctaps_issue(w, kn, rs, fl, T1);
			const int voff = rdl(my_off, k);
			if(voff != cur_off) {
				if(cur_off >= 0 && acc)
					atomicAdd(&busmem[cur_off + (size_t)f * cur_nch * A2D_FRAG + lane], acc);
				acc = 0;
				cur_off = voff;
				cur_nch = rdl(my_nch, k);
			}
			const int x = osctaps_finish(T0, fl);
			acc = wadd(acc, in ? x : 0);
			if(kn < 0)
				break;
			m &= m - 1;
			k = kn;
			T0 = T1;
		}
		if(cur_off >= 0 && acc)
			atomicAdd(&busmem[cur_off + (size_t)f * cur_nch * A2D_FRAG + lane], acc);
	}

	// state out: ctl_store's words of an oscillator
	if(ok)
		oscv_store(ustate + (size_t)u0 * A2D_USTATE, o);
}

// voices per wavefront: at most 64 (one per lane)
int a2d_launch_leaf_oscbare(const A2DParams *dparams, const A2DParams &hp, const int *dlist, int nlist, int vpw, void *stream)
{
	if(nlist <= 0)
		return 0;
	vpw = vpw < 1 ? 1 : vpw > 64 ? 64 : vpw;
	const int nwaves = (nlist + vpw - 1) / vpw;
	const dim3 grid((nwaves + OB_WPB - 1) / OB_WPB), block(64 * OB_WPB);
	hipLaunchKernelGGL(k_leaf_oscbare, grid, block, 0, (hipStream_t)stream, dparams, dlist, nlist, vpw, hp.voices, hp.runs,
			hp.ustate, hp.waves, hp.ptab, hp.wavecoef, hp.nfrags, hp.busmem);
	return hipGetLastError() != hipSuccess;
}
