/* a2amd_noisefilt.h - part of include/a2amd.h (which includes it): the quiet kernel of settled
 * "wtosc (noise) -> filter12 -> panmix" voices, k_leaf_noisefiltpan - who rendered those voices in the
 * most recent batch, and the kernel's arithmetic for tests.
 *
 * In a batch with fragments from a2amd_fragment_repeat_noise() (include/a2amd_noise.h) a noise voice
 * that has no record of its own is rendered from the seeds the device made.  A voice of the chain
 * wtosc -> filter12 (1 channel) -> panmix (1 -> 2, wired, adding) whose oscillator plays the noise
 * generator and whose amplitude, q, volume and pan are at rest - the hat, snare and cymbal shape - goes to
 * a kernel of its own: the oscillator lane = frame as in k_leaf_noisepan (a2amd_noisepan.h), the filter
 * lane = voice, a workgroup of up to 64 voices walking the batch's fragments as a pipeline.  It does so
 * from 'min_voices' such voices in the batch on (A2AMD_NZF_MIN in the environment; a launch lasts as long
 * as its filter's chain through the batch however few the voices); below that every one of them is given
 * the stand-in record like any other noise voice.  A2AMD_NOISE_QUIET=0 sends all of them there (A/B). */
#ifndef A2AMD_NOISEFILT_H
#define A2AMD_NOISEFILT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct a2amd_ctx;

typedef struct a2amd_noise_filter_batch_info {
	uint32_t quiet_launched;   /* 1: k_leaf_noisefiltpan was launched for the most recent batch */
	uint32_t quiet_voices;     /* voices of the class left to it: no record this batch, at rest by the host's books (the
	                            * kernel tests the device's words again and leaves alone a voice that is not) */
	uint32_t class_voices;     /* voices in the launch class wtosc (noise)-filter12-panmix */
	uint32_t min_voices;       /* the threshold in force: recordless voices in a batch from which the kernel takes them */
} a2amd_noise_filter_batch_info;
int a2amd_last_batch_noise_filter(const struct a2amd_ctx *ctx, a2amd_noise_filter_batch_info *out);

/* One window of 'frames' <= 64 frames of such a voice up to the filter's output, in the arithmetic the
 * kernel uses, no device needed: the oscillator (wtosc.c:129-152 with wtosc_run_pitch returning early)
 * enters the window with the engine's generator word 'seed' in front of it, phase 'phase', increment
 * 'dphase', the sample 'held' from its last draw and the amplitude ramper's value 'avalue'; the filter
 * (f12_process, filter12.c:74-119, no cutoff ramp) with its q ramper's value 'qvalue' at rest, the pitch
 * coefficient 'f1', the mix 'lp', 'bp', 'hp' (24:8) and *d1, *d2, which are stepped.  values[s] (when
 * values is not null) is the filter's output for frame s, *seed_after (when not null) the generator word
 * behind the window's last draw, *held_after (when not null) the sample held behind the window.  Returns
 * the number of draws. */
uint32_t a2amd_noise_filter_window(uint32_t seed, uint64_t phase, uint32_t dphase, int32_t held, int32_t avalue,
		int32_t qvalue, int32_t f1, int32_t lp, int32_t bp, int32_t hp, int32_t *d1, int32_t *d2,
		unsigned frames, int32_t *values, uint32_t *seed_after, int32_t *held_after);

#ifdef __cplusplus
}
#endif
#endif /* A2AMD_NOISEFILT_H */
