// settled_probe.cpp - csrc/a2amd_settled.h under a host compiler: one line of results per line of standard input
// (tests/test_settled_header.py).
//   g vol pan clamp 0        ->  v0 v1 a2s_pan_over(pan)
//   m dphase period size0 flags ->  mm dph a2s_wave_ok(size0, flags, dph)
//   r value target delta timer  ->  a2s_arrived(r, a ramper that has arrived) a2s_arrived(that one, r) a2s_at_rest(r)
//                                   a2s_osc_settled(an oscillator with r as its pitch ramper)
#include <stdio.h>
#include "a2amd_settled.h"

int main()
{
	char op;
	long long a, b, c, d;
	while(scanf(" %c %lld %lld %lld %lld", &op, &a, &b, &c, &d) == 5) {
		if(op == 'g') {
			int32_t v0, v1;
			a2s_pan_gains((int32_t)a, (int32_t)b, c != 0, &v0, &v1);
			printf("%d %d %d\n", v0, v1, (int)a2s_pan_over((int32_t)b));
		} else if(op == 'm') {
			uint32_t dph;
			const unsigned mm = a2s_mip((uint32_t)a, (uint32_t)b, &dph);
			printf("%u %u %d\n", mm, dph, (int)a2s_wave_ok((uint32_t)c, (uint32_t)d, dph));
		} else if(op == 'r') {
			const int32_t r[4] = { (int32_t)a, (int32_t)b, (int32_t)c, (int32_t)d }, still[4] = { 5, 5, 0, 0 };
			printf("%d %d %d %d\n", (int)a2s_arrived(r, still), (int)a2s_arrived(still, r), (int)a2s_at_rest(r),
					(int)a2s_osc_settled(A2D_OSC_MIPWAVE, 1u, 0, r, still));
		} else
			return 1;
	}
	return 0;
}
