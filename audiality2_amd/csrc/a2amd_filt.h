// a2amd_filt.h - filter12's recurrence, lane = voice: what the filter wavefront of k_leaf_oscfiltpan / k_leaf_osc2filtpan
// (a2amd_fast.hip), of k_leaf_noisefiltpan (a2amd_noisefiltpan.hip) and of k_leaf_osc3filtpan / k_leaf_osc3filtpan_win
// (a2amd_osc3filtpan.hip) runs along a voice's row of an LDS tile.
#pragma once
#include "a2amd_device.h"
#include "a2amd_dsp.h"

// one filter step (f12_process, filter12.c:98-117).  The filter wavefront's chain of dependent
// instructions is what a pipeline step waits for, so two things that are not part of the recurrence
// are done by the stages around it, all lanes busy: the oscillator stage stores the input already
// shifted (x5 = in >> 5), and where the whole workgroup runs pure low pass filters (LPRAW) the row
// keeps l and the pan stage scales it, (l * lp) >> 3.  12 instructions per frame instead of 15.
template<bool LPRAW>
DEV int filt_step(int x5, int qq, int ff, int lp, int bp, int hp, int &d1, int &d2)
{
	const int d1s = d1 >> 4;
	const int l = wadd(d2, wmul(ff, d1s) >> 8);
	const int h = wsub(wsub(x5, l), wmul(qq, d1s) >> 8);
	const int b = wadd(wmul(ff, h >> 4) >> 8, d1);
	d1 = b;
	d2 = l;
	return LPRAW ? l : (wadd(wadd(wmul(l, lp), wmul(b, bp)), wmul(h, hp)) >> 3);
}

// the filter along one voice's row: n frames in place.  The LDS round trip (~130
// cycles) must not sit on the recurrence: a full fragment is taken sixteen frames at
// a time - sixteen reads in flight, sixteen steps in registers, sixteen writes.
template<bool LPRAW, bool QREST>
DEV void filt_row(int *row, int n, int ff, int lp, int bp, int hp, int &d1, int &d2, int &qv, int qdelta)
{
	if(n == A2D_FRAG) {
		// (round 4: the next sixteen frames are on their way from the LDS while these sixteen are filtered -
		// two register sets; before, each of a fragment's four groups waited out its own LDS round trip)
		int xb[2][16];
#pragma unroll
		for(int k = 0; k < 16; ++k)
			xb[0][k] = row[k];
#pragma unroll
		for(int g = 0; g < A2D_FRAG / 16; ++g) {
			if(g + 1 < A2D_FRAG / 16) {
#pragma unroll
				for(int k = 0; k < 16; ++k)
					xb[(g + 1) & 1][k] = row[(g + 1) * 16 + k];
			}
#pragma unroll
			for(int k = 0; k < 16; ++k) {
				xb[g & 1][k] = filt_step<LPRAW>(xb[g & 1][k], qv >> 12, ff, lp, bp, hp, d1, d2);
				if(!QREST)
					qv = wadd(qv, qdelta);
			}
#pragma unroll
			for(int k = 0; k < 16; ++k)
				row[g * 16 + k] = xb[g & 1][k];
		}
		return;
	}
	for(int s = 0; s < n; ++s) {
		row[s] = filt_step<LPRAW>(row[s], qv >> 12, ff, lp, bp, hp, d1, d2);
		if(!QREST)
			qv = wadd(qv, qdelta);
	}
}

// filt_row for a row format and a q ramper that only the running wavefront knows (lpraw, qrest: wave-uniform; qdelta is
// not read where q rests): the quiet kernels' one statement of the four instantiations.  (k_leaf_oscfiltpan and
// k_leaf_osc2filtpan choose for themselves, a2amd_fast.hip.)
DEV void filt_row_pick(bool lpraw, bool qrest, int *row, int n, int ff, int lp, int bp, int hp, int &d1, int &d2, int &qv, int qdelta)
{
	if(qrest) {
		if(lpraw)
			filt_row<true, true>(row, n, ff, lp, bp, hp, d1, d2, qv, 0);
		else
			filt_row<false, true>(row, n, ff, lp, bp, hp, d1, d2, qv, 0);
	} else {
		if(lpraw)
			filt_row<true, false>(row, n, ff, lp, bp, hp, d1, d2, qv, qdelta);
		else
			filt_row<false, false>(row, n, ff, lp, bp, hp, d1, d2, qv, qdelta);
	}
}

// a workgroup barrier that waits for this wavefront's LDS traffic only: loads from device memory
// stay in flight across it (__syncthreads() is a fence: it waits for them too)
DEV void filt_barrier()
{
	asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
