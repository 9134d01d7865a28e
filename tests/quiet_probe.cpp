// quiet_probe.cpp - csrc/a2amd_quiet.h's worker split under a host compiler: one line of results per line of standard
// input (tests/test_quiet_header.py).
//   nv todo(hex)  ->  a2q_worker_voices(wv, nv, todo) for wv = 0 .. QUIET_WAVES - 1 (hex), then QUIET_WAVES QUIET_WORKERS
#include <stdio.h>
#include "a2amd_quiet.h"

int main()
{
	int nv;
	unsigned long long todo;
	while(scanf(" %d %llx", &nv, &todo) == 2) {
		for(int wv = 0; wv < QUIET_WAVES; ++wv)
			printf("%llx ", (unsigned long long)a2q_worker_voices(wv, nv, (uint64_t)todo));
		printf("%d %d\n", QUIET_WAVES, QUIET_WORKERS);
	}
	return 0;
}
