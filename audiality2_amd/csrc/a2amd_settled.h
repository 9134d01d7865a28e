// a2amd_settled.h - what a leaf kernel works out once per launch (or window) from a voice's state words before it
// may take a settled path, for the host and the device alike.  The one statement of these lines of the reference:
// the kernels, the window control pass and the host's phase shadow call it; tests/test_settled_header.py pins it.
#pragma once
#include <stdint.h>
#include "a2amd_device.h"

#ifdef __HIPCC__
#define A2S static inline __host__ __device__
#else
#define A2S static inline
#endif

// wtosc.c:250-258: the mip level a pitch plays at, *dph = the phase increment per frame at that level
A2S unsigned a2s_mip(uint32_t dphase, uint32_t period, uint32_t *dph)
{
	uint32_t d = ((dphase + 255) >> 8) * period, mm = 0;
	for(; (d > (A2D_MAXPHINC << 8)) && (mm < A2D_MIPS - 1); ++mm)
		d >>= 1;
	*dph = (uint32_t)(((uint64_t)dphase * period) >> mm);
	return mm;
}

// ... and may a settled path take the wave: loaded (wtosc.c:168-183), looped (A2_LOOPED: the phase wraps, :260-263),
// the increment within the interpolator's range at the last level too (:271)
A2S bool a2s_wave_ok(uint32_t size0, uint32_t flags, uint32_t dph)
{
	return size0 && (flags & 0x100u) && dph <= (A2D_MAXPHINC << 16);
}

// panmix_process12's two gains, panmix.c:84-104 (sums and the shift wrap).  Whether they are clamped is the caller's:
// panmix.c:120-124 asks a2s_pan_over() of the pan ramper's value and target in front of a2_PrepareRamper.
A2S bool a2s_pan_over(int32_t pan) { return pan > 0xffffff || pan < -0xffffff; }
A2S void a2s_pan_gains(int32_t vol, int32_t pan, bool clamp, int32_t *v0, int32_t *v1)
{
	const int32_t vp = (int32_t)(((int64_t)pan * (int64_t)vol) >> 24);
	int32_t a = (int32_t)((uint32_t)vol - (uint32_t)vp), b = (int32_t)((uint32_t)vol + (uint32_t)vp);
	if(clamp) {
		const int32_t lim = (int32_t)((uint32_t)vol << 1);
		if(a > lim) a = lim;
		if(b > lim) b = lim;
	}
	*v0 = a;
	*v1 = b;
}

// A ramper {value, target, delta, timer} that a2_PrepareRamper (a2_dsp.h:128-149) will not move - two tests, on purpose:
// "arrived" is the wavetable kernels', which go on reading the VALUE word: nothing pending at all (asked of a unit's two
// rampers at once - a wtosc's pitch and amplitude, a panmix's volume and pan - in the form the kernels were tuned with:
// one OR over the pending words).  "at rest" is the noise kernels', which read the TARGET: it also takes a ramper that
// will only snap (timer 0, whatever value and delta hold) and a write without a duration that has not met a window yet
// (a2_SetRamper, :161-170: a timer below one frame, the value already there).  Merging them would change which voices
// each kernel takes.
A2S bool a2s_arrived(const int32_t *a, const int32_t *b) { return !(a[3] | a[2] | b[3] | b[2]) && a[0] == a[1] && b[0] == b[1]; }
A2S bool a2s_at_rest(const int32_t *r) { return !r[3] || ((uint32_t)r[3] < 256u && r[0] == r[1]); }

// a settled wavetable oscillator: mip-mapped wave, a constant pitch (wtosc_run_pitch returns early, wtosc.c:89-105),
// pitch and amplitude rampers (p, a) arrived - over a batch only its phase moves
A2S bool a2s_osc_settled(int32_t mode, uint32_t dphase, int32_t p_ramping, const int32_t *p, const int32_t *a)
{
	return mode == A2D_OSC_MIPWAVE && dphase && !p_ramping && a2s_arrived(p, a);
}
