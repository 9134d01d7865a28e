// a2amd_osc2tame.hip - k_leaf_osc2tame: the quiet kernel of WHOLE WAVEFRONTS of settled, tame `wtosc; wtosc; panmix`
// voices on power-of-two levels, in batches of whole fragments - what the flagship workload consists of.
//
// It is k_leaf_osc2pan's voice-major walk of tame voices (a2amd_fast.hip: osc2_superchunk<true, true>) and nothing else
// of that kernel: the same grid, slices, tile and level copy in LDS, the same fetch/use order, the same sums - with a
// register allocation of its own.  In the general kernel that walk shares its scalar registers with six others (203 of
// them spilled to lanes), tests every chunk for a modulus that is no mask, and parks end phases voice by voice.  Here
// the modulus is a mask by the wavefront's eligibility (a2amd_device.h: a2d_osc2tame_voice, a2d_osc2tame_wave), every
// fragment is whole by the host's launch rule (a2d_osc2_all_whole), and the end phases are one closed form per launch.
//
// The hand-over: the host launches this kernel in front of k_leaf_osc2pan with the same shape.  Every wavefront decides
// from the state at the batch's start - the same in all its slices - whether all its voices are eligible; slice 0 writes
// the decision to taken[wavefront].  An eligible wavefront renders its voices and leaves their state as the general
// kernel leaves a settled voice's (the two phases, the commit's marks, the tame count); an ineligible one does nothing,
// and the general kernel, whose wavefronts return at their top where taken[] is set, renders it.
#include <hip/hip_runtime.h>
#include "a2amd_device.h"
#include "a2amd_dsp.h"
#include "a2amd_settled.h"
#include "a2amd_taps.h"

#define O2T_FCH A2D_OSC2_FCH
#define O2T_SCH A2D_OSC2_SCH
#define O2T_WPE 4

// a voice's constants, wave-uniform, over a super-chunk: per oscillator the increment at the level, the level's mask
// ((size << 24) - 1), its place in the 16 byte table, the amplitude, the phase at the level (unwrapped between chunks)
struct O2tVoice {
	unsigned dph[2];
	uint64_t mask[2];
	int cb[2], amp[2];
	uint64_t ph[2];
};
struct O2tLds {
	const LdsInt *level[2];
	unsigned m16[2];	// coef4_lds()'s mask of a staged level: (size - 1) << 4
};

// One chunk of O2T_FCH whole fragments, lane = frame: osc2_chunk<true, ST, true>'s mask branch and its halves of two
// fragments (a2amd_fast.hip has the reasons for the order).  ST: a2d_osc2_stage()'s mask.
template<int ST>
DEV void o2t_chunk(const CoefRsrc &crs, O2tVoice &s, const unsigned (&ldph)[2], const O2tLds &lv, int (&xs)[O2T_FCH])
{
	constexpr int H = O2T_FCH / 2;
	Coef4x ka[2][H], kb[2][H];
	unsigned pa[2][O2T_FCH], pb[2][O2T_FCH];
#pragma unroll
	for(int o = 0; o < 2; ++o) {
		const unsigned dph = s.dph[o];
		uint64_t phs[O2T_FCH];
#pragma unroll
		for(int j = 0; j < O2T_FCH; ++j)
			phs[j] = (s.ph[o] + (uint64_t)dph * (unsigned)(j * A2D_FRAG)) & s.mask[o];
		s.ph[o] = phs[O2T_FCH - 1] + (uint64_t)dph * (unsigned)A2D_FRAG;
#pragma unroll
		for(int j = 0; j < O2T_FCH; ++j) {
			pa[o][j] = tap_phase(phs[j], ldph[o]);
			asm("" : "+v"(pa[o][j]));	// (32 bit offsets: scalar-base loads)
			pb[o][j] = pa[o][j] + (dph >> 17);
		}
	}
	auto fetch = [&](int o, int h, int slot) {
#pragma unroll
		for(int j = 0; j < H; ++j) {
			if((ST >> o) & 1) {
				ka[slot][j] = coef4_lds(lv.level[o], pa[o][h * H + j], lv.m16[o]);
				kb[slot][j] = coef4_lds(lv.level[o], pb[o][h * H + j], lv.m16[o]);
			} else {
				ka[slot][j] = coef4_at(crs, s.cb[o], pa[o][h * H + j]);
				kb[slot][j] = coef4_at(crs, s.cb[o], pb[o][h * H + j]);
			}
		}
	};
	auto use = [&](int o, int h, int slot) {
#pragma unroll
		for(int j = 0; j < H; ++j) {
			const int x = wadd(hermite_fused(ka[slot][j], pa[o][h * H + j]), hermite_fused(kb[slot][j], pb[o][h * H + j]));
			const int y = mul64s(x, s.amp[o], 17);
			// the second oscillator adds into the scratch buffer (wrap-around)
			xs[h * H + j] = o ? wadd(xs[h * H + j], y) : y;
		}
	};
	fetch(0, 0, 0);
	fetch(0, 1, 1);
	__builtin_amdgcn_sched_barrier(0);
	use(0, 0, 0);
	__builtin_amdgcn_sched_barrier(0);
	fetch(1, 0, 0);
	__builtin_amdgcn_sched_barrier(0);
	use(0, 1, 1);
	__builtin_amdgcn_sched_barrier(0);
	fetch(1, 1, 1);
	__builtin_amdgcn_sched_barrier(0);
	use(1, 0, 0);
	use(1, 1, 1);
}

// a voice's nsc chunks of a super-chunk into the wavefront's tile
template<int ST>
DEV void o2t_voice_chunks(const CoefRsrc &crs, O2tVoice &s, const unsigned (&ldph)[2], const O2tLds &lv, int nsc, int v0, int v1,
		int lane, int (*tile)[2][A2D_FRAG])
{
	for(int k = 0; k < nsc; ++k) {
		// (a last chunk of fewer than 4 fragments: the rows past the batch's end are computed - from phases inside the
		// wave - and never flushed)
		int xs[O2T_FCH];
		o2t_chunk<ST>(crs, s, ldph, lv, xs);
#pragma unroll
		for(int j = 0; j < O2T_FCH; ++j) {
			tile_add(&tile[k * O2T_FCH + j][0][lane], mul64s(xs[j], v0, 24));
			tile_add(&tile[k * O2T_FCH + j][1][lane], mul64s(xs[j], v1, 24));
		}
	}
}

__global__ __launch_bounds__(64 * FAST_WPB) __attribute__((amdgpu_waves_per_eu(O2T_WPE, O2T_WPE)))
void k_leaf_osc2tame(const A2DParams *__restrict__ pp, const int *__restrict__ list, int nlist, int vpw, int per,
		const A2DVoice *__restrict__ voices, const int *ustate, int *ustage, const A2DWave *__restrict__ waves,
		int *__restrict__ busmem, unsigned char *__restrict__ staged, int lds_taps, const int *__restrict__ wavecoef4,
		unsigned long long *__restrict__ tame_count, unsigned char *__restrict__ taken,
		unsigned long long *__restrict__ taken_count)
{
	const A2DParams &p = *pp;
	const int wv = rfl((int)(threadIdx.x >> 6));
	const int lane = threadIdx.x & 63;
	const int w = blockIdx.x * FAST_WPB + wv;
	const int first = w * vpw;
	if(first >= nlist)
		return;
	const int nv = min(vpw, nlist - first);
	const int nfrags = p.nfrags;
	// this wavefront's time slice: a2d_osc2_slice()'s chunks, from the chunks per slice the host took from that function
	// for this batch's fragments (per: its divisions are the host's - the kernel has none)
	const int slice = blockIdx.y;
	const int nchunks = (nfrags + O2T_FCH - 1) / O2T_FCH;
	const int c_lo = slice * per, c_hi = min(c_lo + per, nchunks);
	if(c_lo >= nchunks)
		return;
	const bool last_slice = c_hi * O2T_FCH >= nfrags;

	// ---- lane = voice: the general kernel's prologue, and the eligibility of the voice ----
	// What stays in the lane over the launch is what the walk fetches per voice and super-chunk: per oscillator the
	// increment, the level's size, its place in the table, the amplitude and the phase AT the level; the pan gains, the
	// bus and the staging mask.  The level itself and the state's phase are needed again only for the end phases.
	int mm_l[2] = { 0, 0 }, dph_l[2] = { 0, 0 }, size_l[2] = { 0, 0 }, cb_l[2] = { 0, 0 }, amp_l[2] = { 0, 0 };
	int phlo_l[2] = { 0, 0 }, phhi_l[2] = { 0, 0 };
	int v0l = 0, v1l = 0, stage_l = 0, my_off = -1, my_nch = 2, uu[2] = { 0, 0 };
	bool ok = false;
	if(lane < nv) {
		const int slot = list[first + lane];
		const A2DVoice &vc = voices[slot];
		my_off = vc.out_off;
		my_nch = vc.out_nch;
		bool osc[2];
		int wave_l[2];
		unsigned periodic[2] = { 0, 0 }, tame_lv[2] = { 0, 0 };
		uint64_t phl[2] = { 0, 0 };
#pragma unroll
		for(int o = 0; o < 2; ++o) {
			uu[o] = vc.unit[o];
			const int *ws = ustate + (size_t)uu[o] * A2D_USTATE;
			wave_l[o] = ws[OW_WAVE];
			dph_l[o] = ws[OW_DPHASE];	// (the state's increment; the level's below)
			amp_l[o] = ws[OW_A];
			phlo_l[o] = ws[OW_PHASE_LO];
			phhi_l[o] = ws[OW_PHASE_HI];
			osc[o] = a2s_osc_settled(ws[OW_MODE], (unsigned)dph_l[o], ws[OW_PRAMPING], ws + OW_P, ws + OW_A);
		}
		const int *wp = ustate + (size_t)vc.unit[2] * A2D_USTATE;
		int sp[8];
#pragma unroll
		for(int k = 0; k < 8; ++k)
			sp[k] = wp[k];		// vol ramper, pan ramper
		const bool pan = a2s_arrived(sp + PW_VOL, sp + PW_PAN);
		bool wok = false;
		if(osc[0] && osc[1] && pan) {
			wok = true;
#pragma unroll
			for(int o = 0; o < 2; ++o) {
				int od[4];
				wok = settled_wave(waves + wave_l[o], (unsigned)dph_l[o], od, wok, &periodic[o], &tame_lv[o]);
				mm_l[o] = od[0];
				dph_l[o] = od[1];
				size_l[o] = od[2];
				cb_l[o] = coef4_base((unsigned)od[3]);
				phl[o] = ((uint64_t)(unsigned)phlo_l[o] | ((uint64_t)(unsigned)phhi_l[o] << 32)) >> mm_l[o];
			}
			a2s_pan_gains(sp[PW_VOL], sp[PW_PAN], a2s_pan_over(sp[PW_PAN]), &v0l, &v1l);
		}
		ok = wok && a2d_osc2tame_voice((unsigned)p.runs[slot].count, osc[0], osc[1], pan, wok, tame_lv[0], tame_lv[1],
				(unsigned)size_l[0], (unsigned)size_l[1], (unsigned)dph_l[0], (unsigned)dph_l[1], phl[0], phl[1],
				(unsigned)nfrags * A2D_FRAG);
		if(ok) {
			if(lds_taps)
				stage_l = (int)a2d_osc2_stage((unsigned)size_l[0], periodic[0], (unsigned)size_l[1], periodic[1]);
#pragma unroll
			for(int o = 0; o < 2; ++o) {
				phlo_l[o] = (int)(unsigned)phl[o];
				phhi_l[o] = (int)(unsigned)(phl[o] >> 32);
			}
		}
	}
	const bool eligible = a2d_osc2tame_wave(__ballot(ok), nv);
	if(slice == 0 && lane == 0) {
		taken[w] = eligible ? 1 : 0;
		if(eligible) {
			atomicAdd(tame_count, (unsigned long long)nv);
			atomicAdd(taken_count, 1ull);
		}
	}
	if(!eligible)
		return;

	// ---- this slice, lane = frame: super-chunks of up to O2T_SCH whole fragments, voice by voice ----
	__shared__ int tiles[FAST_WPB][O2T_SCH][2][A2D_FRAG];
	__shared__ __attribute__((aligned(16))) int levels[FAST_WPB][A2D_OSC2_LDS_ENT * 4];
	int (*const tile)[2][A2D_FRAG] = tiles[wv];
	LdsInt *const level = (LdsInt *)levels[wv];
#pragma unroll
	for(int r = 0; r < O2T_SCH; ++r)
		tile[r][0][lane] = tile[r][1][lane] = 0;
	const CoefRsrc crs = coef4_rsrc(wavecoef4);
	const int dbg = p.debug;
	for(int s_lo = c_lo; s_lo < c_hi; s_lo += O2T_SCH / O2T_FCH) {
		const int s_hi = min(c_hi, s_lo + O2T_SCH / O2T_FCH);
		const int fa = s_lo * O2T_FCH, nfs = min(nfrags, s_hi * O2T_FCH) - fa, nsc = s_hi - s_lo;
		const unsigned before = (unsigned)fa * A2D_FRAG;	// (frames of the batch before the super-chunk: all whole)
		int cur_off = rdl(my_off, 0), cur_nch = rdl(my_nch, 0);
		for(int v = 0; v < nv; ++v) {
			const int voff = rdl(my_off, v);
			if(voff != cur_off) {
				flush_tile(busmem, cur_off, cur_nch, fa, nfs, nsc * O2T_FCH, lane, dbg, tile);
				cur_off = voff;
				cur_nch = rdl(my_nch, v);
			}
			const int v0 = rdl(v0l, v), v1 = rdl(v1l, v);
			O2tVoice s;
			unsigned ldph[2], size[2];
#pragma unroll
			for(int o = 0; o < 2; ++o) {
				s.dph[o] = (unsigned)rdl(dph_l[o], v);
				size[o] = (unsigned)rdl(size_l[o], v);
				s.mask[o] = ((uint64_t)size[o] << 24) - 1;
				s.cb[o] = rdl(cb_l[o], v);
				s.amp[o] = rdl(amp_l[o], v);
				s.ph[o] = ((uint64_t)(unsigned)rdl(phlo_l[o], v) | ((uint64_t)(unsigned)rdl(phhi_l[o], v) << 32)) +
						(uint64_t)before * s.dph[o];
				ldph[o] = lane_dph(lane, s.dph[o]);
			}
			// the voice's staged levels, oscillator 1 behind oscillator 0: lanes read what other lanes wrote, and write
			// where other lanes read for the voice before - a wavefront fence on both sides of the stores
			O2tLds lv = { { level, level }, { 0, 0 } };
			const int st = rdl(stage_l, v);
			if(st) {
				lds_wave_fence();
				if(st & 1) {
					lv.m16[0] = (size[0] - 1) << 4;
					stage_level4(level, wavecoef4, s.cb[0], size[0], lane);
				}
				if(st & 2) {
					LdsInt *const l1 = (st & 1) ? level + size[0] * 4 : level;
					lv.level[1] = l1;
					lv.m16[1] = (size[1] - 1) << 4;
					stage_level4(l1, wavecoef4, s.cb[1], size[1], lane);
				}
				lds_wave_fence();
			}
			switch(st) {
			case 0: o2t_voice_chunks<0>(crs, s, ldph, lv, nsc, v0, v1, lane, tile); break;
			case 1: o2t_voice_chunks<1>(crs, s, ldph, lv, nsc, v0, v1, lane, tile); break;
			case 2: o2t_voice_chunks<2>(crs, s, ldph, lv, nsc, v0, v1, lane, tile); break;
			default: o2t_voice_chunks<3>(crs, s, ldph, lv, nsc, v0, v1, lane, tile); break;
			}
		}
		flush_tile(busmem, cur_off, cur_nch, fa, nfs, nsc * O2T_FCH, lane, dbg, tile);
	}

	// ---- state out, lane = voice, the last slice: the phases moved on, as wtosc.c:284 leaves them - the wrapped start
	// of the batch's last fragment plus its frames times the increment, back at the state's scale ----
	if(lane < nv && last_slice) {
#pragma unroll
		for(int o = 0; o < 2; ++o) {
			const uint64_t dph = (unsigned)dph_l[o];
			const uint64_t mask = ((uint64_t)(unsigned)size_l[o] << 24) - 1;
			const uint64_t phl = (uint64_t)(unsigned)phlo_l[o] | ((uint64_t)(unsigned)phhi_l[o] << 32);
			const uint64_t start = (phl + dph * ((uint64_t)(unsigned)(nfrags - 1) * A2D_FRAG)) & mask;
			const uint64_t endph = (start + dph * A2D_FRAG) << mm_l[o];
			int *ws = ustage + (size_t)uu[o] * A2D_USTATE;
			ws[OW_PHASE_LO] = (int)(unsigned)endph;
			ws[OW_PHASE_HI] = (int)(unsigned)(endph >> 32);
		}
	}
	if(ustage != ustate && lane < nv)
		stage_mark(staged + first + lane, true, true, last_slice, false);
}

int a2d_launch_leaf_osc2tame(const A2DParams *dparams, const A2DParams &hp, const int *dlist, int nlist, int vpw, int ysplit,
		int *ustage, unsigned char *staged, void *stream, int lds_taps, unsigned long long *tame_count, unsigned char *taken,
		unsigned long long *taken_count)
{
	if(nlist <= 0 || hp.nfrags <= 0)
		return 0;
	a2d_osc2_shape(&vpw, &ysplit, ustage && staged);
	const int nwaves = (nlist + vpw - 1) / vpw;
	const int nblocks = (nwaves + FAST_WPB - 1) / FAST_WPB;
	// (the chunks per slice: slice 0's, which starts at chunk 0 and is never the short one unless it is the only one)
	int c_lo, c_hi, nslices;
	a2d_osc2_slice(hp.nfrags, ysplit, 0, &c_lo, &c_hi, &nslices);
	hipLaunchKernelGGL(k_leaf_osc2tame, dim3(nblocks, ysplit), dim3(64 * FAST_WPB), 0, (hipStream_t)stream,
			dparams, dlist, nlist, vpw, c_hi - c_lo, hp.voices, (const int *)hp.ustate, ysplit > 1 ? ustage : hp.ustate, hp.waves,
			hp.busmem, staged, lds_taps, hp.wavecoef4, tame_count, taken, taken_count);
	return (int)hipGetLastError();
}
