// a2amd_noisemap.h - one window of a settled noise oscillator in closed form, for the host and the device alike:
// k_leaf_noisepan (a2amd_noisepan.hip) renders with it, a2amd_noise_window() (a2amd_host.cpp) exports it for tests.
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
