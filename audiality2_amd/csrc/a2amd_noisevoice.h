// a2amd_noisevoice.h - the quiet noise voice k_leaf_noisepan (a2amd_noisepan.hip) and k_leaf_noisefiltpan
// (a2amd_noisefiltpan.hip) share, device only: a settled noise oscillator's words carried lane = voice for the whole
// launch, one window of it lane = frame (a2amd_noisemap.h's closed form), the gains of a panmix at rest, and the state
// both kernels leave behind.
#pragma once
#include "a2amd_device.h"
#include "a2amd_dsp.h"
#include "a2amd_noisemap.h"

// lane v: increment, phase, the generator word in front of the next window, held sample, amplitude (the ramper's
// target), its column of the batch's seed table + 1 (0: none)
struct NoiseV { unsigned d, phlo, phhi, seed; int h, g, col; };

// the words of an oscillator at rest (the caller has tested it, and set d for the test)
DEV void noisev_load(NoiseV &o, const int *w0, int unit, const uint32_t *nseed, const int32_t *nslot, int nnoise)
{
	o.phlo = (unsigned)w0[OW_PHASE_LO];
	o.phhi = (unsigned)w0[OW_PHASE_HI];
	o.h = w0[OW_NOISE];
	o.seed = (unsigned)w0[OW_SEED];
	o.g = w0[OW_A + 1];
	if(nseed) {	// (a2d_noise_seed's bounds)
		const int k = nslot[unit];
		o.col = k > 0 && k <= nnoise ? k : 0;
	}
}

// the generator word in front of window f of a voice with a column: the seed pass's (without one the voice keeps the
// word its last window left)
DEV unsigned noisev_seed(const NoiseV &o, const uint32_t *nseed, int f, int nnoise)
{
	return nseed[(size_t)f * (size_t)nnoise + (size_t)(o.col - 1)];
}

// One window of n frames of voice v, lane = frame (fl: this lane's frame, clamped to the window): the sample the frame
// holds, in front of the amplitude.  Lane v is left the window's last sample and the word after its last draw.
DEV int noisev_window(NoiseV &o, int v, int lane, unsigned fl, int n, uint32_t mapA, uint32_t mapC)
{
	const unsigned d = (unsigned)rdl((int)o.d, v), ph = (unsigned)rdl((int)o.phlo, v);
	const unsigned s0 = (unsigned)rdl((int)o.seed, v);
	const int h = rdl(o.h, v);
	// draw j + 1 of the window, in lane j
	const uint32_t w = a2nm_word(mapA, mapC, s0);
	const int val = a2nm_value(w);
	// the draw this lane's frame holds
	const unsigned c = a2nm_upto(ph, d, fl);
	const int got = __builtin_amdgcn_ds_bpermute((int)(((c - 1u) & 63u) << 2), val);
	const int x = c ? got : h;
	const unsigned total = (unsigned)rdl((int)c, n - 1);
	const int hn = rdl(x, n - 1);
	const unsigned sn = total ? (unsigned)rdl((int)w, (int)total - 1) : s0;
	const bool me = lane == v;
	o.h = me ? hn : o.h;
	o.seed = me ? sn : o.seed;
	return x;
}

// panmix_process12's two gains of a panmix (wp) whose volume and pan are at rest: v0, v1 for the first window the voice
// meets, v0r, v1r for the later ones.  Whether they are clamped is decided in front of a2_PrepareRamper
// (panmix.c:120-124): the first window still sees the value a finished ramp stopped at, the others the target.
struct PanRest { int v0, v1, v0r, v1r; };

DEV void panrest_load(PanRest &g, const int *wp)
{
	const int vol = wp[PW_VOL + 1], pan = wp[PW_PAN + 1];
	const bool cr = a2s_pan_over(pan), c0 = cr || a2s_pan_over(wp[PW_PAN]);
	a2s_pan_gains(vol, pan, c0, &g.v0, &g.v1);
	a2s_pan_gains(vol, pan, cr, &g.v0r, &g.v1r);
}

// state out after 'frames' frames: the oscillator's (w0) and the panmix's (wp) words as ctl_store leaves them for the
// same windows
DEV void noisev_store(const NoiseV &o, unsigned frames, int *w0, int *wp)
{
	const uint64_t ph = ((uint64_t)(unsigned)w0[OW_PHASE_LO] | ((uint64_t)o.phhi << 32)) + (uint64_t)frames * o.d;
	w0[OW_PHASE_LO] = (int)(unsigned)ph;
	w0[OW_PHASE_HI] = (int)(unsigned)(ph >> 32);
	w0[OW_NOISE] = o.h;
	w0[OW_SEED] = (int)o.seed;
	ramp_settle(w0 + OW_P);
	ramp_settle(w0 + OW_A);
	ramp_settle(wp + PW_VOL);
	ramp_settle(wp + PW_PAN);
}
