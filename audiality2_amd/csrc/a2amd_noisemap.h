// a2amd_noisemap.h - one window of a settled noise oscillator in closed form, for the host and the device alike:
// k_leaf_noisepan (a2amd_noisepan.hip) and k_leaf_noisefiltpan (a2amd_noisefiltpan.hip) render with it, a2amd_noise_window()
// and a2amd_noise_filter_window() (a2amd_host.cpp) export it for tests.
//
// wtosc_noise (wtosc.c:129-152) with wtosc_run_pitch returning early (:89-105): a window of n <= 64 frames that the
// oscillator enters with phase ph, increment d, held sample h, the engine's generator word s0 in front of it.
//   c(s) = draws made up to and including frame s: s + 1 where d >= 2^23, else ((ph + (s + 1) d) >> 23) - (ph >> 23)
//          (a difference of two quotients of which the low 32 bits of ph decide: (s + 1) d < 2^29, and a count of at
//          most 64 is its own residue mod 2^9)
//   w_k  = the generator word after k draws: k steps of s -> s * 1566083941 + 1 are ONE affine map (A_k, C_k), the
//          k-fold composition, built by squaring: (A, C) o (A, C) = (A A, A C + C)
//   v_k  = (int)((w_k * (w_k >> 16)) >> 16) - 32767                                      (a2_Noise, a2_dsp.h:37-42)
//   x(s) = c(s) ? v_c(s) : h,    out(s) = (x(s) * (a.value >> 10)) >> 6, the product wrapping
// and afterwards h = x(n - 1), ph += n d, the generator word w_c(n-1).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define NZM static inline __host__ __device__
#else
#define NZM static inline
#endif

#define A2NM_MUL 1566083941u
#define A2NM_MAXDRAWS 64	// a window is a fragment at most: one draw per frame

// draws up to and including frame s (s < 64) of a window entered with phase phlo (its low 32 bits) and increment d
NZM unsigned a2nm_upto(uint32_t phlo, uint32_t d, unsigned s)
{
	if(d >= (1u << 23))
		return s + 1;
	return (((phlo + (s + 1) * d) >> 23) - (phlo >> 23)) & 0x1ffu;
}

// the map of k draws, k <= A2NM_MAXDRAWS (seven squarings: no loop over the draws)
NZM void a2nm_map(unsigned k, uint32_t *A, uint32_t *C)
{
	uint32_t a = A2NM_MUL, c = 1u, ra = 1u, rc = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
	for(int b = 0; b < 7; ++b) {
		if((k >> b) & 1u) {
			rc = a * rc + c;
			ra = a * ra;
		}
		c = a * c + c;
		a = a * a;
	}
	*A = ra;
	*C = rc;
}

NZM uint32_t a2nm_word(uint32_t A, uint32_t C, uint32_t s0) { return A * s0 + C; }

// noise_next()'s value for the generator word it has just made, less the offset wtosc_noise takes off
NZM int32_t a2nm_value(uint32_t w) { return (int32_t)((w * (w >> 16)) >> 16) - 32767; }

// wtosc.c:148: the held sample at the oscillator's amplitude
NZM int32_t a2nm_out(int32_t x, int32_t avalue) { return (int32_t)((uint32_t)x * (uint32_t)(avalue >> 10)) >> 6; }

// One step of filter12 at rest (f12_process, filter12.c:98-117) in the formula of filt_step (a2amd_filt.h), which the
// device runs lane = voice: x5 = the input >> 5, qq = q.value >> 12, ff = f1 >> 12; every sum and product wraps.
NZM int32_t a2nm_filt(int32_t x5, int32_t qq, int32_t ff, int32_t lp, int32_t bp, int32_t hp, int32_t *d1, int32_t *d2)
{
	const int32_t d1s = *d1 >> 4;
	const int32_t l = (int32_t)((uint32_t)*d2 + (uint32_t)((int32_t)((uint32_t)ff * (uint32_t)d1s) >> 8));
	const int32_t h = (int32_t)((uint32_t)x5 - (uint32_t)l - (uint32_t)((int32_t)((uint32_t)qq * (uint32_t)d1s) >> 8));
	const int32_t b = (int32_t)((uint32_t)((int32_t)((uint32_t)ff * (uint32_t)(h >> 4)) >> 8) + (uint32_t)*d1);
	*d1 = b;
	*d2 = l;
	return (int32_t)((uint32_t)l * (uint32_t)lp + (uint32_t)b * (uint32_t)bp + (uint32_t)h * (uint32_t)hp) >> 3;
}
