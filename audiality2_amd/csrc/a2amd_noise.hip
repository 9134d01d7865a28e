// a2amd_noise.hip - the seed pass: the engine's noise generator word in front of every window of a stretch of
// fragments in which nothing but settled noise oscillators draws from it (a2amd_fragment_repeat_noise).
//
// The reference has ONE generator for all noise oscillators (a2_Noise: s = s * 1566083941 + 1) and draws from
// it in the order of its voice walk: fragment after fragment, and within a fragment oscillator after
// oscillator.  A settled oscillator (wtosc_run_pitch returns early, wtosc.c:89-105) with phase ph and
// increment d draws
//     d >= 2^23 :  n                                   times in a window of n frames (wtosc.c:140-145),
//     else      :  ((ph + n * d) >> 23) - (ph >> 23)
// which telescopes over consecutive windows.  So the word in front of oscillator k's window in fragment j of
// the stretch is the start word advanced by
//     sum over ALL oscillators of their draws in fragments [0, j)      (closed form, one reduction)
//   + sum over oscillators < k of their draws in fragment j            (an exclusive prefix sum over k)
// steps, and n steps of an LCG are one affine map: (A2, C2) o (A1, C1) = (A2 * A1, A2 * C1 + C2) mod 2^32,
// n-fold by 32 squarings.  The multiplier is 1 mod 4 and the increment odd: the period is 2^32, so the step
// counts are kept mod 2^32 and every sum below may wrap.
//
// One workgroup per fragment of the stretch, lane = oscillator, the list walked in tiles of the workgroup's
// size: a wavefront scan (__shfl_up), the wavefronts' totals through LDS, a carry from tile to tile.
#include <hip/hip_runtime.h>
#include "a2amd_device.h"

#define NZ_BLOCK 1024
#define NZ_WAVES (NZ_BLOCK / 64)

static __device__ __forceinline__ unsigned nz_jump(unsigned s, unsigned n)
{
	unsigned a = 1566083941u, c = 1u;
#pragma unroll
	for(int b = 0; b < 32; ++b) {
		s = ((n >> b) & 1u) ? a * s + c : s;
		c = a * c + c;
		a = a * a;
	}
	return s;
}

// draws of one oscillator over the first 'nframes' frames of the stretch
static __device__ __forceinline__ unsigned nz_cum(const A2DNoiseOsc &o, unsigned nframes)
{
	if(o.dphase >= (1u << 23))
		return nframes;
	const uint64_t ph = (uint64_t)o.ph_lo | ((uint64_t)o.ph_hi << 32);
	return (unsigned)(((ph + (uint64_t)nframes * o.dphase) >> 23) - (ph >> 23));
}

// inclusive sum over the lanes of a wavefront
static __device__ __forceinline__ unsigned nz_wave_scan(unsigned v, int lane)
{
#pragma unroll
	for(int d = 1; d < 64; d <<= 1) {
		const unsigned t = (unsigned)__shfl_up((int)v, d, 64);
		if(lane >= d)
			v += t;
	}
	return v;
}

__global__ __launch_bounds__(NZ_BLOCK)
void k_noise_seeds(const A2DNoiseOsc *__restrict__ osc, int n, unsigned start, int f0, unsigned frames,
		uint32_t *__restrict__ seed, int stride, size_t seed_words, int32_t *__restrict__ nslot, int nunits)
{
	__shared__ unsigned s_wave[NZ_WAVES];
	const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int j = (int)blockIdx.x;
	const unsigned before = (unsigned)j * frames;

	// every oscillator's draws in the fragments in front of this one
	unsigned part = 0;
	for(int k = tid; k < n; k += NZ_BLOCK)
		part += nz_cum(osc[k], before);
	part = nz_wave_scan(part, lane);
	if(lane == 63)
		s_wave[wv] = part;
	__syncthreads();
	unsigned carry = 0;
#pragma unroll
	for(int w = 0; w < NZ_WAVES; ++w)
		carry += s_wave[w];
	__syncthreads();

	// ... and, oscillator by oscillator, those of this fragment
	for(int base = 0; base < n; base += NZ_BLOCK) {
		const int k = base + tid;
		A2DNoiseOsc o = { 0, 0, 0, -1, -1, { 0, 0, 0 } };
		unsigned mine = 0;
		if(k < n) {
			o = osc[k];
			mine = nz_cum(o, before + frames) - nz_cum(o, before);
		}
		const unsigned incl = nz_wave_scan(mine, lane);
		if(lane == 63)
			s_wave[wv] = incl;
		__syncthreads();
		unsigned below = 0, all = 0;
#pragma unroll
		for(int w = 0; w < NZ_WAVES; ++w) {
			const unsigned t = s_wave[w];
			below += w < wv ? t : 0u;
			all += t;
		}
		if(k < n) {
			const size_t at = (size_t)(f0 + j) * (size_t)stride + (size_t)o.slot;
			if(o.slot >= 0 && o.slot < stride && at < seed_words)
				seed[at] = nz_jump(start, carry + below + incl - mine);
			if(j == 0 && o.unit >= 0 && o.unit < nunits)
				nslot[o.unit] = o.slot + 1;
		}
		carry += all;
		__syncthreads();
	}
}

int a2d_launch_noise_seeds(const A2DNoiseOsc *osc, int n, uint32_t start, int f0, int count, unsigned frames,
		uint32_t *seed, int stride, size_t seed_words, int32_t *nslot, int nunits, void *stream)
{
	if(n <= 0 || count <= 0)
		return 0;
	hipLaunchKernelGGL(k_noise_seeds, dim3(count), dim3(NZ_BLOCK), 0, (hipStream_t)stream, osc, n, start, f0, frames,
			seed, stride, seed_words, nslot, nunits);
	return (int)hipGetLastError();	// (the code itself: the caller formats it)
}
