// a2amd_wavepads.h - are a wave level's pad samples the periodic continuation of its payload?
// Pure C/C++: no HIP, no context.  (a2amd_wave_upload asks it of every level it is handed; tests/wavepads_probe.cpp
// runs it under the sanitizers.)
#pragma once
#include <stdint.h>

// d: the level as the engine keeps it - pre pre-pad samples, size payload samples, post post-pad samples.
// True when the pre-pad in front of the payload is payload sample size - 1 and post-pad sample k is payload sample
// k mod size for every k < post: what a2_fix_pad writes for a looped wave (waves.c:90-100).  A wave whose pads were
// written by somebody else - or not at all - fails it, and its levels are then read through their pads.
//
// Why k_leaf_osc2pan may then read a level of size S from its S payload entries alone, indexed modulo S
// (a2amd_fast.hip: osc2_chunk's staged taps):
//  - a fragment's first tap stands at a wrapped phase, index <= S - 1; lane 63 of its 64 frames is 63 increments of
//    at most 2 samples further (a2s_mip, a2amd_settled.h:15-22: the level is the first whose increment is at most
//    A2D_MAXPHINC << 8; a2s_wave_ok, :26-29, refuses more at the last level): index <= S - 1 + 126, and tap B -
//    half an increment on (a2amd_fast.hip: pb = pa + (dph >> 17)) - one further at most: S + 126;
//  - coefficient entry i is made from samples i - 1 .. i + 2 (a2amd_taps.h:71-76; k_build_coef), so the furthest
//    sample read is S + 128 = post-pad sample 128 < 131 (A2_WAVEPOST), and the nearest is sample -1, the pre-pad;
//  - with periodic pads sample j equals sample j mod S for every j in [-1, S + 130], so entry i equals entry i mod S
//    for every i in [0, S + 128]: all a tap can reach.
static inline int a2w_pads_periodic(const int16_t *d, uint32_t size, uint32_t pre, uint32_t post)
{
	if(!d || !size || !pre)
		return 0;
	const int16_t *p = d + pre;
	if(p[-1] != p[size - 1])
		return 0;
	for(uint32_t k = 0, j = 0; k < post; ++k) {
		if(p[size + k] != p[j])
			return 0;
		if(++j == size)
			j = 0;
	}
	return 1;
}
