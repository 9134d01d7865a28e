/* osc2tame_probe.cpp - k_leaf_osc2tame's eligibility rule (csrc/a2amd_device.h: a2d_osc2tame_voice, a2d_osc2tame_wave,
 * a2d_osc2_all_whole, a2d_osc2_shape) on a host compiler, fed from state words through the settled tests the kernel
 * applies (csrc/a2amd_settled.h); a program of its own so that it can run under the sanitizers:
 *   g++ -std=c++17 -Wall -Werror -g -fsanitize=address,undefined -fno-sanitize-recover=all -I audiality2_amd/csrc
 *       -o osc2tame_probe tests/osc2tame_probe.cpp && ./osc2tame_probe
 * Prints "ok <checks>" and returns 0, or says what failed and returns 1.  (tests/test_osc2tame_rule.py builds it without
 * the sanitizers and runs it.) */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "a2amd_device.h"
#include "a2amd_settled.h"

static int checks, failed;
static void expect(int got, int want, const char *what, long tag)
{
	++checks;
	if(got != want) {
		++failed;
		printf("FAILED: %s, %ld: got %d, want %d\n", what, tag, got, want);
	}
}

// a voice as the kernel's prologue sees it
struct Osc {
	int32_t mode;
	uint32_t dphase;	// the state's increment
	int32_t p_ramping;
	int32_t p[4], a[4];	// {value, target, delta, timer}
	uint32_t size0, flags, period;	// the wave: level 0's size, A2_LOOPED in flags, the period
	uint32_t size;		// the level's size
	uint32_t tame;
	uint64_t phase;		// the state's
};
struct Voice {
	uint32_t records;
	Osc o[2];
	int32_t vol[4], pan[4];
};

static Voice good()
{
	Voice v = {};
	for(int k = 0; k < 2; ++k) {
		Osc &o = v.o[k];
		o.mode = A2D_OSC_MIPWAVE;
		o.dphase = 0x00012345u + 77u * (unsigned)k;
		o.p[0] = o.p[1] = 4711;
		o.a[0] = o.a[1] = 1000 + k;
		o.size0 = 256;
		o.flags = 0x100;
		o.period = 256;
		o.size = 256;
		o.tame = 1;
		o.phase = (uint64_t)(100 + k) << 24;
	}
	v.vol[0] = v.vol[1] = 1 << 16;
	v.pan[0] = v.pan[1] = -3000;
	return v;
}

static bool eligible(const Voice &v, unsigned frames)
{
	bool osc[2], wok = true;
	uint32_t dph[2];
	uint64_t phl[2];
	for(int k = 0; k < 2; ++k) {
		const Osc &o = v.o[k];
		osc[k] = a2s_osc_settled(o.mode, o.dphase, o.p_ramping, o.p, o.a);
		const unsigned mm = a2s_mip(o.dphase, o.period, &dph[k]);
		wok = wok && a2s_wave_ok(o.size0, o.flags, dph[k]);
		phl[k] = o.phase >> mm;
	}
	const bool pan = a2s_arrived(v.vol, v.pan);
	return a2d_osc2tame_voice(v.records, osc[0], osc[1], pan, wok, v.o[0].tame, v.o[1].tame, v.o[0].size, v.o[1].size,
			dph[0], dph[1], phl[0], phl[1], frames);
}

int main()
{
	const unsigned frames = 33 * A2D_FRAG;
	expect(eligible(good(), frames), 1, "a settled, tame voice on power-of-two levels", 0);

	// sizes that are and are not powers of two, in either oscillator
	const unsigned sizes[] = { 1, 2, 32, 64, 128, 256, 4096, 1u << 20, 0, 3, 96, 193, 769, 3001, 255, 257, (1u << 20) + 1 };
	for(unsigned s : sizes)
		for(int k = 0; k < 2; ++k) {
			Voice v = good();
			v.o[k].size = s;
			expect(eligible(v, frames), s && !(s & (s - 1)), "level size", (long)s * 2 + k);
		}
	// each tame bit off
	for(int m = 0; m < 4; ++m) {
		Voice v = good();
		v.o[0].tame = m & 1;
		v.o[1].tame = m >> 1;
		expect(eligible(v, frames), m == 3, "tame bits", m);
	}
	// a run
	for(unsigned r : { 1u, 2u, 1000u }) {
		Voice v = good();
		v.records = r;
		expect(eligible(v, frames), 0, "records", r);
	}
	// each settled condition off
	for(int k = 0; k < 2; ++k) {
		Voice v = good(); v.o[k].mode = A2D_OSC_OFF; expect(eligible(v, frames), 0, "mode off", k);
		v = good(); v.o[k].mode = A2D_OSC_NOISE; expect(eligible(v, frames), 0, "mode noise", k);
		v = good(); v.o[k].dphase = 0; expect(eligible(v, frames), 0, "no increment", k);
		v = good(); v.o[k].p_ramping = 1; expect(eligible(v, frames), 0, "pitch ramping", k);
		for(int w = 0; w < 4; ++w) {
			v = good(); v.o[k].p[w] += 1; expect(eligible(v, frames), 0, "pitch ramper word", k * 4 + w);
			v = good(); v.o[k].a[w] += 1; expect(eligible(v, frames), 0, "amplitude ramper word", k * 4 + w);
		}
		v = good(); v.o[k].size0 = 0; expect(eligible(v, frames), 0, "wave not loaded", k);
		v = good(); v.o[k].flags = 0; expect(eligible(v, frames), 0, "wave not looped", k);
		// (an increment beyond the interpolator's range at the last level: 2 samples a frame is the limit)
		v = good(); v.o[k].dphase = 1u << 24; v.o[k].period = 1u << 12; expect(eligible(v, frames), 0, "increment out of range", k);
	}
	for(int w = 0; w < 4; ++w) {
		Voice v = good(); v.vol[w] += 1; expect(eligible(v, frames), 0, "volume ramper word", w);
		v = good(); v.pan[w] += 1; expect(eligible(v, frames), 0, "pan ramper word", w);
	}
	// a phase at the mask branch's limit: the phase at the level plus the batch's increments stays below 2^48
	{
		uint32_t dph;
		Voice v = good();
		const unsigned mm = a2s_mip(v.o[0].dphase, v.o[0].period, &dph);
		const uint64_t room = ((uint64_t)1 << 48) - (uint64_t)frames * dph;	// the first phase at the level that is too far
		for(int k = 0; k < 2; ++k) {
			v = good(); v.o[k].dphase = v.o[0].dphase; v.o[k].phase = (room - 1) << mm; expect(eligible(v, frames), 1, "phase below the limit", k);
			v = good(); v.o[k].dphase = v.o[0].dphase; v.o[k].phase = room << mm; expect(eligible(v, frames), 0, "phase at the limit", k);
			v = good(); v.o[k].dphase = v.o[0].dphase; v.o[k].phase = (room - 1) << mm; expect(eligible(v, frames + 1), 0, "one frame more", k);
			v = good(); v.o[k].phase = ((uint64_t)1 << 48) << mm; expect(eligible(v, 0), 0, "phase of 2^48, no frames", k);
		}
		// ... and so does a wrapped phase plus a fragment's increments: levels of 2^24 entries and more are out
		v = good(); v.o[1].size = 1u << 23; expect(eligible(v, frames), 1, "a level of 2^23", 0);
		v = good(); v.o[1].size = 1u << 24; expect(eligible(v, frames), 0, "a level of 2^24", 0);
	}

	// the wavefront: every one of its nv voices, nv from 1 to 64
	for(int nv = 1; nv <= 64; ++nv) {
		const unsigned long long all = nv == 64 ? ~0ull : (1ull << nv) - 1;
		expect(a2d_osc2tame_wave(all, nv), 1, "all voices", nv);
		for(int b = 0; b < nv; ++b)
			expect(a2d_osc2tame_wave(all & ~(1ull << b), nv), 0, "one voice missing", nv * 64 + b);
		expect(a2d_osc2tame_wave(0, nv), 0, "no voice", nv);
	}
	expect(a2d_osc2tame_wave(0, 0), 0, "no lanes", 0);
	expect(a2d_osc2tame_wave(~0ull, 65), 0, "more voices than lanes", 65);

	// the host's side: every fragment whole, by the kernel's slices and super-chunks (heap blocks of exactly nfrags entries)
	for(int nfrags : { 1, 3, 4, 5, 16, 17, 33, 256 })
		for(int ysplit : { 1, 2, 16 }) {
			std::vector<unsigned> fr((size_t)nfrags, A2D_FRAG);
			const int y = ysplit < (nfrags + A2D_OSC2_FCH - 1) / A2D_OSC2_FCH ? ysplit : (nfrags + A2D_OSC2_FCH - 1) / A2D_OSC2_FCH;
			expect(a2d_osc2_all_whole(fr.data(), nfrags, y), 1, "whole batch", nfrags * 100 + ysplit);
			for(int f : { 0, nfrags / 2, nfrags - 1 }) {
				std::vector<unsigned> cut = fr;
				cut[(size_t)f] = 37;
				expect(a2d_osc2_all_whole(cut.data(), nfrags, y), 0, "a cut fragment", (nfrags * 100 + ysplit) * 1000 + f);
			}
		}
	expect(a2d_osc2_all_whole(nullptr, 0, 1), 0, "no fragments", 0);
	// ... and the shape both launches take
	{
		int vpw = 0, y = 16;
		a2d_osc2_shape(&vpw, &y, true); expect(vpw, 1, "vpw floor", 0); expect(y, 16, "slices kept", 0);
		vpw = 99; y = 0;
		a2d_osc2_shape(&vpw, &y, true); expect(vpw, 64, "vpw ceiling", 0); expect(y, 1, "slices floor", 0);
		vpw = 32; y = 16;
		a2d_osc2_shape(&vpw, &y, false); expect(vpw, 32, "vpw kept", 0); expect(y, 1, "nothing to stage: one slice", 0);
	}

	if(failed) {
		printf("%d of %d checks failed\n", failed, checks);
		return 1;
	}
	printf("ok %d\n", checks);
	return 0;
}
