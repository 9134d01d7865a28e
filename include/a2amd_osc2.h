/* a2amd_osc2.h - part of include/a2amd.h (which includes it): how the quiet kernel of `wtosc; wtosc; panmix`
 * voices, k_leaf_osc2pan, walked the settled voices of the most recent batch.
 *
 * The launch cuts the batch into time slices of whole 4-fragment chunks; a wavefront renders its voices over one
 * slice, in super-chunks of at most 16 fragments counted from the slice's first chunk.  A super-chunk whose
 * fragments all have the full 64 frames is walked voice by voice: a voice's constants are fetched once for the
 * whole super-chunk, its phases are carried from chunk to chunk, and the bus sums of the 16 fragments are kept
 * in LDS.  A super-chunk that holds a shorter fragment (the engine cut a fragment for a voice that woke up
 * inside it) is walked chunk by chunk with the sums in registers, as every super-chunk was before; so is every
 * super-chunk when bit 16 of A2AMD_DEBUG is set in the environment (A/B runs, tests).  Voices that still have
 * something moving take neither walk: the kernel steps them fragment by fragment.
 * The counts are the host's, by the rule the kernel applies (csrc/a2amd_device.h: a2d_osc2_slice,
 * a2d_osc2_whole) to the fragment lengths of the batch - nothing is read back from the device. */
#ifndef A2AMD_OSC2_H
#define A2AMD_OSC2_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct a2amd_ctx;

typedef struct a2amd_osc2_batch_info {
	uint32_t launched;       /* 1: k_leaf_osc2pan ran for the most recent batch */
	uint32_t voices;         /* voices on the kernel: the entries of its launch list (those with records this batch are skipped by it) */
	uint32_t vpw;            /* voices per wavefront of the launch */
	uint32_t ysplit;         /* time slices of the launch */
	uint32_t voice_major;    /* 1: the voice-major walk was allowed (A2AMD_DEBUG bit 16 clear) */
	uint32_t superchunks_voice_major;  /* super-chunks of the batch, over all its slices, walked voice by voice */
	uint32_t superchunks_chunk_major;  /* ... and walked chunk by chunk */
	uint32_t reserved;
	uint64_t chunk_major_mask;         /* bit i: the i-th super-chunk of the batch, in time order, was walked chunk by chunk (the first 64) */
} a2amd_osc2_batch_info;
int a2amd_last_batch_osc2(const struct a2amd_ctx *ctx, a2amd_osc2_batch_info *out);

#ifdef __cplusplus
}
#endif
#endif /* A2AMD_OSC2_H */
