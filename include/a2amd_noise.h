/* a2amd_noise.h - part of include/a2amd.h (which includes it): stretches of default windows for a scene
 * with noise oscillators, the engine's one noise generator advanced in closed form.
 *
 * The reference draws its noise from one engine-global generator (a2_Noise: s = s * 1566083941 + 1), in
 * the order of its voice walk.  A window of a noise oscillator that the engine calls for goes through
 * a2amd_unit_process(), which hands the generator word back advanced by that window's draws.  The entry
 * point below covers whole fragments without calls. */
#ifndef A2AMD_NOISE_H
#define A2AMD_NOISE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct a2amd_ctx;

/* a2amd_fragment_repeat() for a scene with SETTLED noise oscillators: 'count' further fragments in
 * which every live voice gets exactly its default window, the noise oscillators among them seeded on
 * the device.  *noisestate is the engine's generator word on entry (a2_Noise, one for the whole
 * engine); on return it is what 'count' walks by calls would have left there - computed on the host
 * in closed form, no device round trip.
 *
 * A noise oscillator is settled when wtosc_run_pitch (wtosc.c:89-105) would return early: its phase
 * increment is set and its pitch neither ramps nor has just been written.  Its amplitude may ramp.
 * The generator is drawn from in walk order, which the backend learns from the calls: the order in
 * which a2amd_unit_process() met the noise oscillators in the most recent fragment that was walked by
 * calls (a2amd_fragment()) is the order of every fragment of the stretch.
 *
 * Control writes belong to fragments walked by calls, as with a2amd_fragment_repeat(): a write to a voice
 * with a noise oscillator made after the last fragment was closed (between two stretches) is refused
 * here with A2AMD_ESTATE - walk a fragment by calls first.
 *
 * Refusals - the recording and *noisestate are then untouched:
 *   A2AMD_EUNSUPPORTED  a noise oscillator that is not settled; a filter cutoff ramp in flight; a
 *                       unit with clients; a distributed or grouped context (one generator shared
 *                       by several contexts has no defined order)
 *   A2AMD_ESTATE        a live noise oscillator that no call processed in that fragment (no such
 *                       fragment yet, or a voice born since); and what a2amd_fragment() refuses
 * A batch that holds such fragments is rendered once: a2amd_render() with A2AMD_RENDER_KEEP and
 * a2amd_replay() refuse it (a re-run would need a new generator word). */
int  a2amd_fragment_repeat_noise(struct a2amd_ctx *ctx, unsigned frames, unsigned count, uint32_t *noisestate);

/* The arithmetic of the above, for tests (no device needed):
 * the generator word after 'draws' steps of s = s * 1566083941 + 1, in O(log draws) ... */
uint32_t a2amd_noise_jump(uint32_t state, uint64_t draws);
/* ... and the draws a settled noise oscillator makes in a window of 'frames' frames that it enters
 * with phase 'phase' and increment 'dphase' (wtosc.c:140-145): 'frames' if dphase >= 1 << 23, else
 * ((phase + frames * dphase) >> 23) - (phase >> 23). */
uint64_t a2amd_noise_draws(uint64_t phase, uint32_t dphase, unsigned frames);

#ifdef __cplusplus
}
#endif
#endif /* A2AMD_NOISE_H */
