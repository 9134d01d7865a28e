/* a2amd_wavepost.h - part of include/a2amd.h (which includes it): a wave the device rendered that asks for
 * "normalize" and / or "xfade" is post-processed on the device as well.
 *
 * When the stream a2_RenderWave() wrote closes (a2_wave_stream_flush, src/waves.c:513-527), the reference
 *   1. with A2_NORMALIZE, takes the peak of every buffer that was written - one a2_Write() per chunk of the
 *      substate's A2_POFFLINEBUFFER frames, src/render.c:72-112 -, makes a gain 32767 * 256 / peak of each
 *      (1 for a silent buffer) and keeps the smallest, 1000 at most (waves.c:241-306, 405-418); the gain is 1
 *      without the flag,
 *   2. converts: >> 8 for a gain of exactly 1, (float)sample * (gain / 256) truncated otherwise (waves.c:155-237),
 *   3. with A2_XFADE, applies a triangular window, adds the second half to the first and copies the first
 *      half over the second (a2_postprocess, waves.c:326-344),
 *   4. fixes the pads and renders the mip levels (waves.c:89-130).
 * All of it is reproduced bit for bit by kernels that read the capture; neither the peaks nor the gain ever
 * reach the host, nothing is copied from it, and nothing waits.
 *
 * A2_REVMIX is NOT done here and never will be: a2_postprocess reads d[size] at i = 0 (waves.c:319-320) - the
 * first pad sample of a buffer that malloc() has just handed out, before any pad is written.  What the
 * reference computes depends on heap contents (unless A2_CLEAR is set); there is nothing to be identical to.
 * The caller uploads the engine's own copy of such a wave (a2amd_wave_upload). */
#ifndef A2AMD_WAVEPOST_H
#define A2AMD_WAVEPOST_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define A2AMD_NORMALIZE 0x00010000u   /* A2_NORMALIZE, include/a2_waves.h:113 */
#define A2AMD_XFADE     0x00040000u   /* A2_XFADE,     include/a2_waves.h:114 */
#define A2AMD_REVMIX    0x00080000u   /* A2_REVMIX,    include/a2_waves.h:115 */

/* a2amd_wave_upload_captured() for a wave whose w->flags may hold A2AMD_NORMALIZE and A2AMD_XFADE; with neither
 * it does exactly what that call does.  'chunk' is the number of frames per a2_Write() the reference made:
 * the A2_config.buffer of the substate that rendered the capture (every write but the last has that many).
 * A2AMD_EUNSUPPORTED - and nothing changed - for A2AMD_REVMIX, for A2AMD_XFADE on fewer than 2 samples
 * (a window step of 1 / 0), for A2AMD_NORMALIZE with chunk == 0, and for what a2amd_wave_upload_captured()
 * refuses (a capture on another GPU, a wave type without samples, a size that is not the capture's). */
int a2amd_wave_upload_captured_post(a2amd_ctx *ctx, uint64_t key, const a2amd_wavedesc *w,
		const a2amd_capture *cap, unsigned chunk);

/* The arithmetic of steps 1-3 on the host, written as the reference writes it (the window's gain summed up
 * sample by sample), for tests; no device needed.  pcm[n]: what was written (A2_I24), out16[n]: level 0
 * without pads.  Refuses like the call above (A2AMD_EUNSUPPORTED); A2AMD_EINVAL for a null pointer. */
int a2amd_wavepost_host(const int32_t *pcm, unsigned n, unsigned chunk, unsigned flags, int16_t *out16);

#ifdef __cplusplus
}
#endif
#endif /* A2AMD_WAVEPOST_H */
