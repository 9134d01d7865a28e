/* a2amd_wavepool.h - part of include/a2amd.h (which includes it): what the host has done with the wave pool and the
 * tables that follow it, for tests that must know that the event they are about really happened.
 *
 * Every wavetable kernel reads its taps through tables the host moves, rebuilds and re-labels while voices play them:
 * the sample pool, the 12 byte Hermite entries, the 16 byte entries of the fused steps (a2amd_osc2tame.h) and the
 * per-wave descriptor with its raw-taps bit.  The pool starts at 8 388 608 samples and is reallocated when an upload
 * does not fit; a dropped wave's region goes to a free list (first fit, neighbours merged, the pool's tail given back);
 * once the pool's 12 byte entries outgrow A2AMD_COEF_CACHE_MB the 16 byte table is freed for good and every live
 * mip-mapped wave of 4 096 samples or more is flagged to be read as samples.  Host bookkeeping only: nothing here
 * touches the device or waits for it. */
#ifndef A2AMD_WAVEPOOL_H
#define A2AMD_WAVEPOOL_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct a2amd_ctx;

/* (a struct tag, not a typedef: the call below has the same name) */
struct a2amd_wave_pool_info {
	uint64_t used;		/* samples of the pool in use: the end of the last region (regions on the free list included) */
	uint64_t capacity;	/* samples the pool holds before it is reallocated */
	uint64_t free_samples;	/* samples on the free list (regions still held for the batch being recorded are not) */
	uint32_t coef4;		/* 1: the 16 byte table of the fused steps exists */
	uint32_t raw_waves;	/* live waves flagged to be read as samples (the footprint policy, or A2AMD_RAW=1) */
	uint32_t reallocations;	/* times the pool was reallocated since a2amd_open() */
	uint32_t regions_reused;	/* uploads since a2amd_open() that were placed in a region from the free list */
};

int a2amd_wave_pool_info(const struct a2amd_ctx *ctx, struct a2amd_wave_pool_info *out);

#ifdef __cplusplus
}
#endif
#endif /* A2AMD_WAVEPOOL_H */
