/* a2amd_osc2tame_kernel.h - part of include/a2amd.h (which includes it): k_leaf_osc2tame, the quiet kernel of whole
 * wavefronts of settled, tame `wtosc; wtosc; panmix` voices, and what it took of the most recent batch.
 *
 * k_leaf_osc2pan (a2amd_osc2.h) renders every voice of the class that carries no record: settled or gliding, tame
 * (a2amd_osc2tame.h) or not, on levels of any size, in batches with or without cut fragments.  Its walk of the
 * settled, tame voices - all the voices of a large static scene - pays for that in registers.  k_leaf_osc2tame holds
 * that one walk: the host launches it in front of k_leaf_osc2pan, with the same launch shape, when
 *   - the fused steps are on (the 16 byte table exists, A2AMD_DEBUG bit 18 clear) and so is the voice-major walk (bit
 *     16 clear),
 *   - every fragment of the batch has its full 64 frames (every super-chunk of every slice is whole, a2amd_osc2.h),
 *   - the class has at least 1 024 voices (fewer: the second launch costs more than the walk saves), or bit 20 of
 *     A2AMD_DEBUG is set (tests), and
 *   - bit 19 of A2AMD_DEBUG is clear (A/B runs, tests: k_leaf_osc2pan alone, as before).
 * A wavefront of the launch takes its voices when every one of them is without a record, settled, tame, on levels whose
 * sizes are powers of two, at phases below 2^48 for the whole batch - decided from the state at the batch's start.  It
 * then renders them for the whole batch and leaves their state; every other wavefront leaves its voices to
 * k_leaf_osc2pan, whose wavefronts skip the ones that were taken.  The audio and the state are the same either way. */
#ifndef A2AMD_OSC2TAME_KERNEL_H
#define A2AMD_OSC2TAME_KERNEL_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct a2amd_ctx;

typedef struct a2amd_osc2quiet_batch_info {
	uint32_t launched;      /* 1: k_leaf_osc2tame ran in front of k_leaf_osc2pan for the most recent batch */
	uint32_t wavefronts;    /* wavefronts of the launch list (a2amd_osc2_batch_info: voices over vpw, rounded up); 0 when not launched */
	uint64_t taken_total;   /* wavefronts k_leaf_osc2tame took, summed over all its launches since the context was opened:
	                         * read from a device word after waiting for the context's stream, as a2amd_osc2_tame_voices()
	                         * reads its own (the difference over a batch is the number it took in that batch) */
} a2amd_osc2quiet_batch_info;
/* A batch that ran from a captured graph - a quiet batch recorded again, a step of a2amd_replay() - reports launched and
 * wavefronts as they were when its graph was captured: the capture goes through the same launch code and sets them, a
 * replay leaves them alone.  They are that batch's own all the same: a graph does not outlive the launch decision it
 * was captured under (a change of the rule's answer, of the hold, of the class drops it), so a replay runs the pair
 * exactly when the capture did.  taken_total is a device word and counts the wavefronts taken in replays as in any
 * other launch.  A batch launched without the pair, directly or into a new graph, reports 0 and 0. */
int a2amd_last_batch_osc2quiet(struct a2amd_ctx *ctx, a2amd_osc2quiet_batch_info *out);

/* hold != 0: from the next batch on this context launches k_leaf_osc2pan alone, as under bit 19; 0: by the rule above
 * again.  For A/B runs and tests inside one context - the state a batch leaves is the same whichever kernel left it, and
 * the next batch may go to the other.  Graphs captured with the other setting are dropped. */
int a2amd_osc2quiet_hold(struct a2amd_ctx *ctx, int hold);

#ifdef __cplusplus
}
#endif
#endif /* A2AMD_OSC2TAME_KERNEL_H */
