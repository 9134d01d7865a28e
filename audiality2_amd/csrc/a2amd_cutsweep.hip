// a2amd_cutsweep.hip - the sweep pass: the filter coefficient behind every window of a stretch of repeated fragments for
// the filter12 units whose cutoff is ramping (a2amd_fragment_repeat / a2amd_fragment_repeat_noise).
//
// In a fragment walked by calls the host runs a ramping filter's cutoff ramper and f12_pitch2coeff and ships the result
// as an R_F1RAMP record.  A repeated fragment has no calls and no records: the batch's table cutf[fragment][column] stands
// in for the record, read through a2d_cut_coeff() (a2amd_device.h).  A cell holds the coefficient the head of f12_process
// (filter12.c:87-96) would have made for that window, or a negative word where the ramper did not move (a2amd_cutsweep.h).
//
// The ramper's recurrence over the windows is serial - its delta is a 64 bit quotient of what is left, taken anew in every
// window - so k_cut_sweep is lane = filter with one loop over the stretch.  The coefficient is a gather from the 8 MB table
// f1tab (a2vm::f1_of_pitch: the reference's float / libm expression for everything a2_P2I can return), at an address the
// step has just made.  Of the two ways to keep that load out of the serial chain this file takes the TWO-KERNEL form: the
// loop stores the pitch argument (value >> 8: 24 bits, sign-extended - told from the marker by its range), and
// k_cut_resolve, fully parallel over fragment x column, replaces it by the table's entry.  Why: it holds whatever the
// compiler makes of the loop (the other form - gather in the loop, shown from the ISA to overlap - would have to be shown
// again after every change of compiler or loop), the loop then has no load at all, the gathers of a whole batch are in
// flight together, and one resolve launch serves all stretches of the batch.  The cost is a second pass over a table of
// fragments x columns words that is still in L2.
//
// Stores are coalesced where the list is in column order (columns are handed out in list order): lane = consecutive slots.
// No LDS.
#include <hip/hip_runtime.h>
#include "a2amd_device.h"
#include "a2amd_cutsweep.h"

#define CS_BLOCK 256

__global__ __launch_bounds__(CS_BLOCK)
void k_cut_sweep(const A2DCutSweep *__restrict__ list, int n, int f0, int count, int frames,
		int32_t *__restrict__ cutf, int stride, size_t words, int32_t *__restrict__ cslot, int nunits)
{
	const int k = (int)(blockIdx.x * CS_BLOCK + threadIdx.x);
	if(k >= n)
		return;
	const A2DCutSweep e = list[k];
	if(e.slot < 0 || e.slot >= stride)
		return;
	if(e.unit >= 0 && e.unit < nunits)
		cslot[e.unit] = e.slot + 1;
	int32_t r[4] = { e.ramper[0], e.ramper[1], e.ramper[2], e.ramper[3] };
	size_t at = (size_t)f0 * (size_t)stride + (size_t)e.slot;
	for(int j = 0; j < count; ++j, at += (size_t)stride) {
		int32_t pitch;
		const bool moved = a2cs_step(r, frames, &pitch);
		if(at < words)
			cutf[at] = moved ? pitch : A2CS_NONE;
	}
}

// every cell of the batch's table that holds a pitch argument: the coefficient (a2vm::f1_of_pitch's index: the shift count
// a2_P2I derives from the octave, and the 16 fraction bits)
__global__ __launch_bounds__(CS_BLOCK)
void k_cut_resolve(int32_t *__restrict__ cutf, size_t words, const int32_t *__restrict__ f1tab)
{
	const size_t step = (size_t)gridDim.x * CS_BLOCK;
	for(size_t i = (size_t)blockIdx.x * CS_BLOCK + threadIdx.x; i < words; i += step) {
		const int32_t pitch = cutf[i];
		if(pitch < -(1 << 23) || pitch >= (1 << 23))
			continue;	// (the marker)
		const unsigned frac = (unsigned)pitch & 0xffffu, sh = (unsigned)(7 - (pitch >> 16)) & 31u;
		cutf[i] = f1tab[(size_t)sh * 65536u + frac];
	}
}

int a2d_launch_cut_sweep(const A2DCutSweep *list, int n, int f0, int count, unsigned frames, int32_t *cutf, int stride,
		size_t words, int32_t *cslot, int nunits, void *stream)
{
	if(n <= 0 || count <= 0 || !frames)
		return 0;
	hipLaunchKernelGGL(k_cut_sweep, dim3((n + CS_BLOCK - 1) / CS_BLOCK), dim3(CS_BLOCK), 0, (hipStream_t)stream, list, n, f0,
			count, (int)frames, cutf, stride, words, cslot, nunits);
	return (int)hipGetLastError();	// (the code itself: the caller formats it)
}

int a2d_launch_cut_resolve(int32_t *cutf, size_t words, const int32_t *f1tab, void *stream)
{
	if(!words)
		return 0;
	const size_t blocks = (words + CS_BLOCK - 1) / CS_BLOCK;
	hipLaunchKernelGGL(k_cut_resolve, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(CS_BLOCK), 0, (hipStream_t)stream,
			cutf, words, f1tab);
	return (int)hipGetLastError();
}
