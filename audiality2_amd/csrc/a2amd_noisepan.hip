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
// and wavefront, flushed where the output bus changes (the list is sorted by bus).  At the end the wavefront stores
// what k_win_ctl's ctl_store would have left for the same windows - phase, held sample, generator word, the rampers
// at their targets - with plain vector stores: nobody else touches the voice during the launch.
//
// A voice with records this batch (runs[v].count != 0) is the window / records kernels' and is skipped untouched.
// The host (upload(), a2amd_sched.cpp) leaves a voice without the stand-in run only while its amplitude, volume and
// pan are at rest; a stretch of device-seeded fragments only exists while every noise oscillator's pitch is.  A voice
// that is not at rest all the same is left alone here, as one with records is.
#include <hip/hip_runtime.h>
#include "a2amd_device.h"
#include "a2amd_dsp.h"
#include "a2amd_noisemap.h"

#define NP_WPB 4	// wavefronts per workgroup

static __device__ __forceinline__ int np_rdl(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

// a ramper a2_PrepareRamper (a2_dsp.h:128-149) leaves at its target with delta and timer 0 whatever the window's length:
// the timer at 0, or - a write without a duration that has not met a window yet, a2_SetRamper :161-170 - below one frame
// with the value already there
static __device__ __forceinline__ bool np_at_rest(const int *r) { return !r[3] || ((unsigned)r[3] < 256u && r[0] == r[1]); }

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
	int u0 = 0, u1 = 0, my_off = -1, my_nch = 2, col = 0;
	unsigned d_l = 0, phlo_l = 0, phhi_l = 0, seed_l = 0;
	int h_l = 0, g_l = 0, v0_l = 0, v1_l = 0, v0r_l = 0, v1r_l = 0;
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
			d_l = (unsigned)w0[OW_DPHASE];
			// at rest: wtosc_run_pitch returns early, and a2_PrepareRamper finds every ramper arrived
			ok = vc.nunits == 2 && my_off >= 0 && w0[OW_MODE] == A2D_OSC_NOISE && d_l && !w0[OW_PRAMPING] &&
					np_at_rest(w0 + OW_P) && np_at_rest(w0 + OW_A) && np_at_rest(w1 + PW_VOL) && np_at_rest(w1 + PW_PAN);
			if(ok) {
				phlo_l = (unsigned)w0[OW_PHASE_LO];
				phhi_l = (unsigned)w0[OW_PHASE_HI];
				h_l = w0[OW_NOISE];
				seed_l = (unsigned)w0[OW_SEED];
				g_l = w0[OW_A + 1];
				// its column of the batch's seed table (a2d_noise_seed's bounds)
				if(nseed) {
					const int k = nslot[u0];
					col = k > 0 && k <= nnoise ? k : 0;
				}
				// panmix_process12's two gains (panmix.c:84-104) as k_leaf_oscpan's settled path derives them.  Whether
				// they are clamped is decided in front of a2_PrepareRamper (panmix.c:120-124): the first window still
				// sees the value a finished ramp stopped at, the others the target
				const int vol = w1[PW_VOL + 1], pan = w1[PW_PAN + 1], pwas = w1[PW_PAN];
				const int vp = mul64s(pan, vol, 24), lim = wshl(vol, 1);
				const int v0 = wsub(vol, vp), v1 = wadd(vol, vp);
				const bool cr = pan > 0xffffff || pan < -0xffffff, c0 = cr || pwas > 0xffffff || pwas < -0xffffff;
				v0_l = c0 && v0 > lim ? lim : v0;
				v1_l = c0 && v1 > lim ? lim : v1;
				v0r_l = cr && v0 > lim ? lim : v0;
				v1r_l = cr && v1 > lim ? lim : v1;
			}
		}
	}
	const unsigned long long todo = __ballot(ok);
	if(!todo)
		return;

	unsigned total_frames = 0;
	for(int f = 0; f < nfrags; ++f) {
		const int n = min((int)pp->fragframes[f], A2D_FRAG);
		if(n <= 0)
			continue;
		// the generator word in front of each voice's window: the seed pass's, or - no column in this batch - the word
		// its last window left
		if(col)
			seed_l = nseed[(size_t)f * (size_t)nnoise + (size_t)(col - 1)];
		int acc0 = 0, acc1 = 0;
		int cur_off = -1, cur_nch = 2;
		const unsigned fl = (unsigned)min(lane, n - 1);	// (lanes beyond the fragment's frames: the last frame's, dropped below)
		for(unsigned long long m = todo; m; m &= m - 1) {
			const int v = (int)__builtin_ctzll(m);
			const int voff = np_rdl(my_off, v);
			if(voff != cur_off) {
				if(cur_off >= 0) {
					int *dst = busmem + cur_off + (size_t)f * cur_nch * A2D_FRAG;
					if(acc0)
						atomicAdd(&dst[lane], acc0);
					if(acc1)
						atomicAdd(&dst[A2D_FRAG + lane], acc1);
				}
				acc0 = acc1 = 0;
				cur_off = voff;
				cur_nch = np_rdl(my_nch, v);
			}
			const unsigned d = (unsigned)np_rdl((int)d_l, v), ph = (unsigned)np_rdl((int)phlo_l, v);
			const unsigned s0 = (unsigned)np_rdl((int)seed_l, v);
			const int h = np_rdl(h_l, v);
			// draw j + 1 of the window, in lane j
			const uint32_t w = a2nm_word(mapA, mapC, s0);
			const int val = a2nm_value(w);
			// the draw this lane's frame holds
			const unsigned c = a2nm_upto(ph, d, fl);
			const int got = __builtin_amdgcn_ds_bpermute((int)(((c - 1u) & 63u) << 2), val);
			const int x = c ? got : h;
			// what the window leaves: the last frame's sample, the word after its last draw
			const unsigned total = (unsigned)np_rdl((int)c, n - 1);
			const int hn = np_rdl(x, n - 1);
			const unsigned sn = total ? (unsigned)np_rdl((int)w, (int)total - 1) : s0;
			const bool me = lane == v;
			h_l = me ? hn : h_l;
			seed_l = me ? sn : seed_l;
			if(lane < n) {
				const int y = a2nm_out(x, np_rdl(g_l, v));
				acc0 = wadd(acc0, mul64s(y, np_rdl(v0_l, v), 24));
				acc1 = wadd(acc1, mul64s(y, np_rdl(v1_l, v), 24));
			}
		}
		if(cur_off >= 0) {
			int *dst = busmem + cur_off + (size_t)f * cur_nch * A2D_FRAG;
			if(acc0)
				atomicAdd(&dst[lane], acc0);
			if(acc1)
				atomicAdd(&dst[A2D_FRAG + lane], acc1);
		}
		// every voice moves on by n frames (all lanes at once)
		phlo_l += (unsigned)n * d_l;
		total_frames += (unsigned)n;
		v0_l = v0r_l;
		v1_l = v1r_l;
	}

	// state out: ctl_store's words for the same windows
	if(ok) {
		int *w0 = ustate + (size_t)u0 * A2D_USTATE;
		int *w1 = ustate + (size_t)u1 * A2D_USTATE;
		const uint64_t ph = ((uint64_t)(unsigned)w0[OW_PHASE_LO] | ((uint64_t)phhi_l << 32)) + (uint64_t)total_frames * d_l;
		w0[OW_PHASE_LO] = (int)(unsigned)ph;
		w0[OW_PHASE_HI] = (int)(unsigned)(ph >> 32);
		w0[OW_NOISE] = h_l;
		w0[OW_SEED] = (int)seed_l;
		// (a2_PrepareRamper on a ramper at rest: value = target, delta = timer = 0)
		w0[OW_P] = w0[OW_P + 1]; w0[OW_P + 2] = w0[OW_P + 3] = 0;
		w0[OW_A] = w0[OW_A + 1]; w0[OW_A + 2] = w0[OW_A + 3] = 0;
		w1[PW_VOL] = w1[PW_VOL + 1]; w1[PW_VOL + 2] = w1[PW_VOL + 3] = 0;
		w1[PW_PAN] = w1[PW_PAN + 1]; w1[PW_PAN + 2] = w1[PW_PAN + 3] = 0;
	}
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
