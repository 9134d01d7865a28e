// a2amd_wavetame.h - does a wave level keep every product of a2_Hermite inside 32 bits?
// Pure C/C++: no HIP, no context.  (a2amd_wave_upload asks it of every level it is handed; tests/wavetame_probe.cpp
// runs it under the sanitizers.)
#pragma once
#include <stdint.h>

// a2_Hermite (a2_dsp.h:64-74) takes three Horner steps (v * x) >> 15 with x = frac << 7, frac = 0 .. 255, in 32 bit
// wrap-around arithmetic.  v * x = (v * frac) << 7 leaves 32 bits as soon as the product p = v * frac leaves
// [-2^24, 2^24), and the reference then returns the wrapped value's bits: the kernels reproduce that with a 17 bit
// field extract per step (a2amd_taps.h: hermite_step).  Where NO product of a level wraps, a step is
//	(v * frac) >> 8 = floor(v * frac / 256)
// and the addend that follows it folds into the multiply as a multiple of 256:
//	t = (a * f + (b << 8)) >> 8	= floor(a * f / 256) + b
//	t = (t * f + (c << 8)) >> 8	= floor(t * f / 256) + c
//	y = (t * f + (d0 << 8)) >> 8	= floor(t * f / 256) + d0: a2_Hermite's result
// exactly, because >> is a floor and the addend has no bits below 256 (a2amd_taps.h: hermite_fused; operand ranges:
// |t| < 2^19 as hermite_step()'s comment derives, 0 <= f <= 255, |a * f + (b << 8)| < 2^24 + 2^26 < 2^27).
//
// A level is "tame" when that holds for every window d[i-1 .. i+2] a tap can reach and every fraction.  It has to be
// proven per level: a single full-scale jump gives a = 65 534 (65 534 * 255 < 2^24, tame), the engine's built-in waves
// and synth.test_waves() - full-scale pulses and saws included - are tame in all their levels, full-scale white noise
// wraps in about 13 % of its windows.
// (docs/history/round4_measurement.md gave "|a| up to 90 109" for the built-in waves and dropped the folded step for
// it.  That maximum was taken over the flat sample array and comes from windows that straddle two mip levels, which no
// tap reads; with windows kept inside a level - pre-pad, payload, post-pad - the largest |a| of those waves is 65 534.)
//
// d: the level as the engine keeps it - pre pre-pad samples, size payload samples, post post-pad samples.
// Looks at every window that lies wholly inside the buffer and has its second sample at payload index i >= 0:
// i in [0, size + post - 3], a superset of what a tap reaches (a2amd_wavepads.h: index <= size + 126).  True when each
// of the three products of every window, evaluated as the reference evaluates them, stays in [-2^24, 2^24) for every
// frac in 0 .. 255.  Exhaustive, not a bound: a window is only spared the 256 fractions where magnitudes alone prove
// all three products small (|v1| <= |a|, |v2| <= |a| + |b| + 1, |v3| <= |a| + |b| + |c| + 2), which decides nearly
// every window of real audio.  False for no data, an empty level, no pre-pad, or no whole window.
#define A2W_TAME_LIM (1 << 24)

static inline int a2w_window_tame(int dm, int d0, int d1, int d2)
{
	const int c = (d1 - dm) >> 1;
	const int a = (3 * (d0 - d1) + d2 - dm) >> 1;
	const int b = dm - d0 + c - a;
	const int ma = a < 0 ? -a : a, mb = b < 0 ? -b : b, mc = c < 0 ? -c : c;
	if((ma + mb + mc + 2) * 255 < A2W_TAME_LIM)
		return 1;
	for(int f = 0; f < 256; ++f) {
		int p = a * f;		// (|a| <= 131 070: no host overflow in any of the three)
		if(p < -A2W_TAME_LIM || p >= A2W_TAME_LIM)
			return 0;
		p = ((p >> 8) + b) * f;
		if(p < -A2W_TAME_LIM || p >= A2W_TAME_LIM)
			return 0;
		p = ((p >> 8) + c) * f;
		if(p < -A2W_TAME_LIM || p >= A2W_TAME_LIM)
			return 0;
	}
	return 1;
}

static inline int a2w_level_tame(const int16_t *d, uint32_t size, uint32_t pre, uint32_t post)
{
	if(!d || !size || !pre)
		return 0;
	const int64_t last = (int64_t)size + (int64_t)post - 3;		// the last window's second sample
	if(last < 0)
		return 0;
	const int16_t *p = d + pre;
	for(int64_t i = 0; i <= last; ++i)
		if(!a2w_window_tame(p[i - 1], p[i], p[i + 1], p[i + 2]))
			return 0;
	return 1;
}
