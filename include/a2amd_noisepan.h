/* a2amd_noisepan.h - part of include/a2amd.h (which includes it): the quiet kernel of settled
 * "wtosc (noise) -> panmix" voices, k_leaf_noisepan - who rendered the noise voices of the most recent
 * batch, and the kernel's arithmetic for tests.
 *
 * In a batch with fragments from a2amd_fragment_repeat_noise() (include/a2amd_noise.h) a noise voice
 * that has no record of its own is rendered from the seeds the device made.  A voice of the chain
 * wtosc -> panmix (1 -> 2, wired, adding) whose oscillator plays the noise generator and whose amplitude,
 * volume and pan are at rest goes to a kernel of its own, lane = frame, no loop over the draws; every
 * other noise voice - a filter or a second oscillator in its chain, a ramp in flight - is given a stand-in
 * record and goes to the window / records kernels or the general kernel, as any voice with records does.
 * A2AMD_NOISE_QUIET=0 in the environment sends all of them there (A/B). */
#ifndef A2AMD_NOISEPAN_H
#define A2AMD_NOISEPAN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct a2amd_ctx;

typedef struct a2amd_noise_batch_info {
	uint32_t quiet_launched;   /* 1: k_leaf_noisepan was launched for the most recent batch */
	uint32_t quiet_voices;     /* voices of the class it rendered (no record this batch, at rest) */
	uint32_t class_voices;     /* voices in the launch class wtosc (noise)-panmix */
	uint32_t standin_voices;   /* noise voices given the stand-in run this batch (any class) */
} a2amd_noise_batch_info;
int a2amd_last_batch_noise(const struct a2amd_ctx *ctx, a2amd_noise_batch_info *out);

/* One window of 'frames' <= 64 frames of a settled noise oscillator (wtosc.c:129-152 with wtosc_run_pitch
 * returning early) in the closed form the kernel uses, no device needed: the oscillator enters the window
 * with the engine's generator word 'seed' in front of it, phase 'phase', increment 'dphase' and the sample
 * 'held' from its last draw.  values[s] (when values is not null) is the sample frame s holds - before the
 * amplitude - and *seed_after (when not null) the generator word behind the window's last draw.  Returns
 * the number of draws; the sample held afterwards is values[frames - 1]. */
uint32_t a2amd_noise_window(uint32_t seed, uint64_t phase, uint32_t dphase, int32_t held, unsigned frames,
		int32_t *values, uint32_t *seed_after);

#ifdef __cplusplus
}
#endif
#endif /* A2AMD_NOISEPAN_H */
