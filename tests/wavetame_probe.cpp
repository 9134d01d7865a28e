/* wavetame_probe.cpp - csrc/a2amd_wavetame.h and a2d_osc2_tame() (csrc/a2amd_device.h) on a host compiler, a program of
 * its own so that it can run under the sanitizers:
 *   g++ -std=c++17 -Wall -Werror -g -fsanitize=address,undefined -fno-sanitize-recover=all -I audiality2_amd/csrc
 *       -o wavetame_probe tests/wavetame_probe.cpp && ./wavetame_probe
 * Every level is a heap block of exactly pre + size + post samples: a read past either end is the sanitizer's to find.
 * Prints "ok <checks>" and returns 0, or says what failed and returns 1.  (tests/test_wave_tame.py builds it without
 * the sanitizers and runs it.) */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "a2amd_device.h"
#include "a2amd_wavetame.h"

enum { PRE = 1, POST = 131 };	// A2_WAVEPRE, A2_WAVEPOST (include/a2amd.h)

static int checks, failed;
static void expect(int got, int want, const char *what, long tag)
{
	++checks;
	if(got != want) {
		++failed;
		printf("FAILED: %s, %ld: got %d, want %d\n", what, tag, got, want);
	}
}

static int16_t *level(unsigned size, unsigned pre, unsigned post)
{
	int16_t *d = (int16_t *)calloc(pre + size + post ? pre + size + post : 1, sizeof(int16_t));
	if(!d)
		exit(2);
	return d;
}

// the rule without the short cut: every fraction of every window, the reference's three products in 64 bits
static int plain(const int16_t *d, unsigned size, unsigned pre, unsigned post)
{
	const int16_t *p = d + pre;
	for(long i = 0; i <= (long)size + (long)post - 3; ++i) {
		const long dm = p[i - 1], d0 = p[i], d1 = p[i + 1], d2 = p[i + 2];
		const long c = (d1 - dm) >> 1, a = (3 * (d0 - d1) + d2 - dm) >> 1, b = dm - d0 + c - a;
		for(long f = 0; f < 256; ++f) {
			long v = a * f;
			if(v < -(1l << 24) || v >= (1l << 24)) return 0;
			v = ((v >> 8) + b) * f;
			if(v < -(1l << 24) || v >= (1l << 24)) return 0;
			v = ((v >> 8) + c) * f;
			if(v < -(1l << 24) || v >= (1l << 24)) return 0;
		}
	}
	return 1;
}

int main()
{
	// the windows at the edge of the 24 bit product: (dm, d0, d1, d2), tame
	static const int edge[][5] = {
		{ 32251, 32767, -32768, -32768, 1 },	// a = 65 793: 2^24 - 1 at frac 255
		{ 32249, 32767, -32768, -32768, 0 },	// a = 65 794: wraps at frac 255 only
		{ -32252, -32768, 32767, 32767, 1 },	// a = -65 793
		{ -32250, -32768, 32767, 32767, 0 },	// a = -65 794
	};
	const unsigned size = 64;
	// (the window's second sample: in the payload, in the post-pad, the last whole window of the buffer, the pre-pad window)
	static const unsigned at[] = { 20, size + 100, size + POST - 3, 0 };
	for(const auto &e : edge)
		for(unsigned i : at) {
			int16_t *d = level(size, PRE, POST);
			expect(a2w_level_tame(d, size, PRE, POST), 1, "silence", i);
			for(int k = 0; k < 4; ++k)
				d[PRE + i - 1 + k] = (int16_t)e[k];
			expect(a2w_level_tame(d, size, PRE, POST), e[4], "edge window", e[0] * 1000l + i);
			expect(plain(d, size, PRE, POST), e[4], "edge window, plain", e[0] * 1000l + i);
			free(d);
		}
	// full-scale alternation: a = +-131 070, far beyond
	{
		int16_t *d = level(size, PRE, POST);
		for(unsigned i = 0; i < PRE + size + POST; ++i)
			d[i] = (i & 1) ? 32767 : -32768;
		expect(a2w_level_tame(d, size, PRE, POST), 0, "alternation", 0);
		free(d);
	}
	// a single full-scale jump is tame (a = 65 534)
	{
		int16_t *d = level(size, PRE, POST);
		for(unsigned i = PRE + 30; i < PRE + size + POST; ++i)
			d[i] = 32767;
		for(unsigned i = 0; i < PRE + 30; ++i)
			d[i] = -32767;
		expect(a2w_level_tame(d, size, PRE, POST), 1, "one jump", 0);
		free(d);
	}
	// the short cut decides as the plain loop does: noise at amplitudes around the edge
	{
		unsigned seed = 12345;
		for(int amp = 9000; amp <= 33000; amp += 1500) {
			const unsigned n = 97;
			int16_t *d = level(n, PRE, POST);
			for(unsigned i = 0; i < PRE + n + POST; ++i) {
				seed = seed * 1664525u + 1013904223u;
				long v = (long)((seed >> 8) % (2u * amp + 1u)) - amp;
				d[i] = (int16_t)(v > 32767 ? 32767 : v < -32768 ? -32768 : v);
			}
			expect(a2w_level_tame(d, n, PRE, POST), plain(d, n, PRE, POST), "noise against the plain loop", amp);
			free(d);
		}
	}
	// degenerate levels
	{
		int16_t *d = level(1, PRE, POST);
		expect(a2w_level_tame(d, 1, PRE, POST), 1, "size 1", 1);
		expect(a2w_level_tame(d, 0, PRE, POST), 0, "size 0", 0);
		expect(a2w_level_tame(d, 1, 0, POST), 0, "no pre-pad", 0);
		free(d);
		expect(a2w_level_tame(nullptr, 64, PRE, POST), 0, "no data", 64);
	}
	for(unsigned post = 0; post < 3; ++post)
		for(unsigned sz = 1; sz <= 4; ++sz) {
			// windows exist from size + post >= 3 on; fewer samples: nothing is proven, not tame
			int16_t *d = level(sz, PRE, post);
			expect(a2w_level_tame(d, sz, PRE, post), sz + post >= 3 ? 1 : 0, "short post-pad", sz * 10 + post);
			if(sz + post >= 3) {
				// ... and the last whole window is looked at, the samples behind it are not there
				d[PRE + sz + post - 1] = -32768;
				d[PRE + sz + post - 2] = -32768;
				d[PRE + sz + post - 3] = 32767;
				d[PRE + sz + post - 4] = 32249;
				expect(a2w_level_tame(d, sz, PRE, post), 0, "short post-pad, edge window", sz * 10 + post);
			}
			free(d);
		}

	// the voice's rule
	expect((int)a2d_osc2_tame(0, 0), 0, "a2d_osc2_tame", 0);
	expect((int)a2d_osc2_tame(1, 0), 0, "a2d_osc2_tame", 1);
	expect((int)a2d_osc2_tame(0, 1), 0, "a2d_osc2_tame", 2);
	expect((int)a2d_osc2_tame(1, 1), 1, "a2d_osc2_tame", 3);
	if(failed)
		return 1;
	printf("ok %d\n", checks);
	return 0;
}
