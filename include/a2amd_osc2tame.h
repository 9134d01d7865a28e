/* a2amd_osc2tame.h - part of include/a2amd.h (which includes it): which settled voices of k_leaf_osc2pan's voice-major
 * walk (a2amd_osc2.h) take the interpolation's fused multiply-add steps.
 *
 * The reference's Hermite interpolation (a2_Hermite, a2_dsp.h:64-74) multiplies in 32 bit wrap-around arithmetic, and a
 * product wraps once |value * fraction| reaches 2^24.  A mip level in which no window does that for any fraction is
 * "tame": there a Horner step and the add behind it are one 24 bit multiply-add and one shift, read from a second
 * coefficient table of 16 byte entries {a, b << 8, c << 8, d0 << 8} (csrc/a2amd_wavetame.h has the proof).
 * a2amd_wave_upload() checks every level of the samples it is handed, exhaustively; the levels of a wave the device
 * renders itself (a2amd_wave_upload_captured[_post]) are not checked and are never tame.  A settled voice takes the fused
 * steps when both its oscillators play tame levels; every other voice, the chunk-major walk and the voices with
 * something moving take the wrap-around steps as before.  The 16 byte table exists only while the wave pool is small
 * enough for the footprint policy to keep coefficient entries at all (A2AMD_COEF_CACHE_MB); once the pool outgrows that
 * the table is dropped and no voice is tame for the kernel.  Bit 18 of A2AMD_DEBUG in the environment: no voice is tame
 * (A/B runs, tests).
 *
 * A tame voice's staged levels (a2amd_osc2lds.h) are copied to LDS in the 16 byte layout, 2 048 bytes a wavefront; the
 * staging rule - a2amd_osc2_stage_rule() - is the same for both kinds of voices. */
#ifndef A2AMD_OSC2TAME_H
#define A2AMD_OSC2TAME_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct a2amd_ctx;

/* 1: no product of a2_Hermite wraps in `level` - A2AMD_WAVEPRE pre-pad samples, size payload samples, A2AMD_WAVEPOST
 * post-pad samples, as in a2amd_wavedesc.data[] - for any window inside it and any fraction: what a2amd_wave_upload()
 * asks of every level */
int a2amd_wave_level_tame(const int16_t *level, unsigned size);

/* 1: a settled voice whose oscillators play levels that are tame (tame0 / tame1) takes the fused steps, given that the
 * 16 byte table exists and bit 18 of A2AMD_DEBUG is clear */
unsigned a2amd_osc2_tame_rule(int tame0, int tame1);

/* The voices k_leaf_osc2pan gave the tame bit - settled, both levels tame, the table there, bit 18 clear - summed over
 * all its launches since the context was opened: a voice counts once per batch in which it had the bit.  Read from a
 * device word after waiting for the context's stream (tests: the difference over a batch is the number of voices that
 * took the fused steps in it, on the voice-major walk; the chunk-major walk of the same voices takes the wrap-around
 * steps and counts them all the same). */
int a2amd_osc2_tame_voices(struct a2amd_ctx *ctx, uint64_t *out);

#ifdef __cplusplus
}
#endif
#endif /* A2AMD_OSC2TAME_H */
