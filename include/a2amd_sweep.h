/* a2amd_sweep.h - part of include/a2amd.h (which includes it): filter12 cutoff sweeps in repeated fragments.
 *
 * a2amd_fragment_repeat() and a2amd_fragment_repeat_noise() record stretches of default windows without a
 * call per voice.  A filter12 whose cutoff is ramping needs a new coefficient in every window: in a fragment
 * walked by calls the host runs the cutoff ramper (a2_PrepareRamper / a2_RunRamper, a2_dsp.h:128-155) and
 * f12_pitch2coeff (filter12.c:65-72) and records the result; in a repeated fragment the device does - a pass
 * over the stretch (a2amd_cutsweep.hip) leaves, per fragment and sweeping filter, the coefficient behind the
 * window or "no ramp in this window", and the kernels that render default windows read it there.  The host
 * steps its own copy of the ramper over the stretch in integers; it evaluates no sine.
 *
 * Listed are the live filter12 units of voices the host drives whose ramper has a ramp under way or has not
 * yet snapped to its target.  A write to such a filter's voice between two stretches belongs to a fragment
 * walked by calls (A2AMD_ESTATE); A2AMD_RENDER_KEEP and a2amd_replay() on a batch with a sweep table are
 * refused (A2AMD_EUNSUPPORTED): a re-run would need the ramp to go on. */
#ifndef A2AMD_SWEEP_H
#define A2AMD_SWEEP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct a2amd_ctx;

typedef struct a2amd_sweep_batch_info {
	uint32_t pass_launched;    /* 1: the sweep pass ran for the most recent batch */
	uint32_t filters;          /* columns of the batch's table: filters listed by at least one of its stretches */
	uint32_t ramp_windows;     /* cells that hold a coefficient: windows in which a listed filter's cutoff moved */
	uint32_t standin_voices;   /* voices of listed filters without a record of their own in the batch, given the stand-in
	                            * record that keeps them away from the kernels of settled voices */
} a2amd_sweep_batch_info;
int a2amd_last_batch_sweeps(const struct a2amd_ctx *ctx, a2amd_sweep_batch_info *out);

/* The pass's arithmetic on the host, no device needed: the cutoff ramper 'ramper' = {value, target, delta,
 * timer} (A2_ramper, a2_dsp.h:105-111) is stepped over 'count' windows of 'frames' <= 64 frames each, as the
 * head of f12_process (filter12.c:87-96) steps it, and comes back as the last window leaves it.  coef[j] is
 * the coefficient behind window j - f12_pitch2coeff evaluated on the host for the pitch table 'ptab128'
 * (a2amd_set_pitch_table's layout) and 'samplerate' - where the ramper moved in it, and
 * A2AMD_SWEEP_NONE where it did not.  Returns the number of windows with a coefficient, or a negative error. */
#define A2AMD_SWEEP_NONE ((int32_t)0x80808080u)
int a2amd_cutoff_sweep(int32_t ramper[4], unsigned frames, unsigned count, const uint32_t *ptab128, int samplerate,
		int32_t *coef);

#ifdef __cplusplus
}
#endif
#endif /* A2AMD_SWEEP_H */
