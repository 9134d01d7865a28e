// a2amd_cutsweep.h - one window of a filter12's cutoff ramper, for the host and the device alike: the sweep pass
// (a2amd_cutsweep.hip) steps a listed filter over a stretch of repeated fragments with it, a2amd_fragment_repeat[_noise]
// (a2amd_host.cpp) steps the host's shadow ramper over the same stretch, a2amd_cutoff_sweep() exports it for tests.
//
// The head of f12_process (filter12.c:87-96) for a window of n frames, the ramper r = {value, target, delta, timer}:
//   a2_PrepareRamper(r, n)  (a2_dsp.h:128-149)
//     timer == 0           : value = target, delta = 0                         (arrived: the ramper snaps)
//     n <= timer >> 8      : delta = ((int64)(target - value) << 8) / timer, timer -= n << 8
//     else                 : delta = (target - value) / n, timer = 0           (the ramp ends inside this window)
//   delta != 0             : a2_RunRamper: value += delta * n, and f1 = f12_pitch2coeff of the pitch value >> 8
//   delta == 0             : the coefficient stays
// delta is recomputed from what is left in every window - a 64 bit quotient - so the recurrence over the windows of a
// stretch is serial.  Integer arithmetic only (sums, differences and products wrap as the reference's do on the
// machines it runs on); the sine of f12_pitch2coeff is the caller's: the device's table (a2vm::f1_of_pitch), the
// host's f12_coeff.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define A2CS static inline __host__ __device__
#else
#define A2CS static inline
#endif

// "no ramp in this window": coefficients are 0 .. 362 << 16, so any negative word serves - this one is what a
// byte-wise fill of the table with A2CS_NONE_BYTE leaves, and lies outside the pitch arguments (value >> 8, 24 bits
// sign-extended) the sweep pass keeps in a cell between its two kernels
#define A2CS_NONE_BYTE 0x80
#define A2CS_NONE ((int32_t)0x80808080u)

// is the ramper still to be stepped: a ramp under way, or the window behind it in which the ramper only snaps
A2CS bool a2cs_moving(const int32_t r[4]) { return r[3] || r[2] || r[0] != r[1]; }

// One window of 'frames' > 0 frames.  True: the cutoff moved, *pitch is the argument of f12_pitch2coeff behind it.
A2CS bool a2cs_step(int32_t r[4], int frames, int32_t *pitch)
{
	const int32_t diff = (int32_t)((uint32_t)r[1] - (uint32_t)r[0]);
	if(!r[3]) {
		r[0] = r[1];
		r[2] = 0;
	} else if(frames <= (r[3] >> 8)) {
		// (timer >= frames << 8 > 0 here)
		r[2] = (int32_t)(((int64_t)diff * 256) / r[3]);
		r[3] = (int32_t)((uint32_t)r[3] - ((uint32_t)frames << 8));
	} else {
		r[2] = diff / frames;
		r[3] = 0;
	}
	if(!r[2])
		return false;
	r[0] = (int32_t)((uint32_t)r[0] + (uint32_t)r[2] * (uint32_t)frames);
	*pitch = r[0] >> 8;
	return true;
}
