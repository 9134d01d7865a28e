/* wavepads_probe.cpp - csrc/a2amd_wavepads.h and a2d_osc2_stage() (csrc/a2amd_device.h) on a host compiler, a program of
 * its own so that it can run under the sanitizers:
 *   g++ -std=c++17 -Wall -Werror -g -fsanitize=address,undefined -fno-sanitize-recover=all -I audiality2_amd/csrc
 *       -o wavepads_probe tests/wavepads_probe.cpp && ./wavepads_probe
 * Every level is a heap block of exactly pre + size + post samples: a read past either end is the sanitizer's to find.
 * Prints "ok <checks>" and returns 0, or says what failed and returns 1.  (tests/test_osc2_lds_rule.py builds it
 * without the sanitizers and runs it.) */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "a2amd_device.h"
#include "a2amd_wavepads.h"

enum { PRE = 1, POST = 131 };	// A2_WAVEPRE, A2_WAVEPOST (include/a2amd.h)

static int checks, failed;
static void expect(int got, int want, const char *what, unsigned size)
{
	++checks;
	if(got != want) {
		++failed;
		printf("FAILED: %s, size %u: got %d, want %d\n", what, size, got, want);
	}
}

// a level with the pads a2_fix_pad writes for a looped wave (waves.c:90-100)
static int16_t *level(unsigned size)
{
	int16_t *d = (int16_t *)malloc((PRE + size + POST) * sizeof(int16_t));
	if(!d)
		exit(2);
	for(unsigned i = 0; i < size; ++i)
		d[PRE + i] = (int16_t)((i * 2654435761u >> 13) | 1u);		// (never 0, no two neighbours equal)
	d[0] = d[PRE + size - 1];
	for(unsigned k = 0; k < POST; ++k)
		d[PRE + size + k] = d[PRE + k % size];
	return d;
}

int main()
{
	static const unsigned sizes[] = { 1, 2, 63, 64, 2048 };
	for(unsigned size : sizes) {
		int16_t *d = level(size);
		expect(a2w_pads_periodic(d, size, PRE, POST), 1, "periodic pads", size);
		d[0] ^= 1;
		expect(a2w_pads_periodic(d, size, PRE, POST), 0, "pre-pad wrong", size);
		d[0] ^= 1;
		d[PRE + size] ^= 1;
		expect(a2w_pads_periodic(d, size, PRE, POST), 0, "first post-pad sample wrong", size);
		d[PRE + size] ^= 1;
		d[PRE + size + POST - 1] ^= 1;
		expect(a2w_pads_periodic(d, size, PRE, POST), 0, "last post-pad sample wrong", size);
		d[PRE + size + POST - 1] ^= 1;
		expect(a2w_pads_periodic(d, size, PRE, POST), 1, "periodic pads again", size);
		// a payload sample changed: both pads that repeat it are now wrong
		d[PRE + size - 1] ^= 1;
		expect(a2w_pads_periodic(d, size, PRE, POST), 0, "last payload sample changed", size);
		free(d);
	}
	// an unlooped level's pads are zeros (waves.c:101-105): not periodic unless the payload is
	{
		int16_t *d = level(64);
		memset(d + PRE + 64, 0, POST * sizeof(int16_t));
		d[0] = 0;
		expect(a2w_pads_periodic(d, 64, PRE, POST), 0, "zero pads", 64);
		free(d);
	}
	expect(a2w_pads_periodic(nullptr, 64, PRE, POST), 0, "no data", 64);
	{
		int16_t one = 0;
		expect(a2w_pads_periodic(&one, 0, PRE, POST), 0, "empty level", 0);
	}

	// the rule: size0, periodic0, size1, periodic1 -> mask
	static const unsigned rule[][5] = {
		{ 64, 1, 64, 1, 3 }, { 128, 1, 128, 1, 1 }, { 128, 1, 64, 1, 1 }, { 256, 1, 64, 1, 2 }, { 64, 1, 256, 1, 1 },
		{ 32, 1, 32, 1, 3 }, { 96, 1, 64, 1, 2 }, { 64, 1, 96, 1, 1 }, { 256, 1, 256, 1, 0 }, { 64, 0, 64, 1, 2 },
		{ 64, 1, 64, 0, 1 }, { 64, 0, 64, 0, 0 }, { 128, 0, 128, 1, 2 }, { 1, 1, 1, 1, 3 }, { 0, 1, 64, 1, 2 },
		{ 64, 1, 0, 1, 1 }, { 127, 1, 129, 1, 0 }, { 64, 1, 32, 1, 3 }, { 2048, 1, 1024, 1, 0 }, { 0x80000000u, 1, 128, 1, 2 },
	};
	for(const auto &r : rule)
		expect((int)a2d_osc2_stage(r[0], r[1], r[2], r[3]), (int)r[4], "a2d_osc2_stage", r[0] * 1000 + r[2]);
	// ... and what it promises the kernel for every pair of sizes: staged levels are powers of two and fit together
	for(unsigned s0 = 0; s0 <= 300; ++s0)
		for(unsigned s1 = 0; s1 <= 300; ++s1) {
			const unsigned m = a2d_osc2_stage(s0, 1, s1, 1);
			const unsigned used = ((m & 1) ? s0 : 0) + ((m & 2) ? s1 : 0);
			const bool pow2 = (!(m & 1) || (s0 && !(s0 & (s0 - 1)))) && (!(m & 2) || (s1 && !(s1 & (s1 - 1))));
			if(used > A2D_OSC2_LDS_ENT || !pow2 || m > 3)
				expect((int)m, -1, "a2d_osc2_stage out of its bounds", s0 * 1000 + s1);
		}
	++checks;
	if(failed)
		return 1;
	printf("ok %d\n", checks);
	return 0;
}
