/* a2amd_osc2lds.h - part of include/a2amd.h (which includes it): which taps of k_leaf_osc2pan's voice-major walk
 * (a2amd_osc2.h) come from LDS.
 *
 * A settled oscillator reads two Hermite coefficient entries per output frame, lane by lane, out of the mip level its
 * pitch plays at.  High notes play small levels: 128 or 64 entries, read thousands of times per voice and super-chunk.
 * On the voice-major walk the wavefront copies such a level's payload entries into 1 536 bytes of LDS of its own and
 * reads them there, indexed modulo the level's size; every other level, the chunk-major walk and the voices with
 * something moving read the global table as before.  The copy stands for the level only where the level's pads are the
 * periodic continuation of its payload (a2_fix_pad's, src/waves.c:90-100): a2amd_wave_upload() checks that on the
 * samples it is handed; the levels of a wave the device renders itself (a2amd_wave_upload_captured[_post]) are not
 * checked and are never copied.  Bit 17 of A2AMD_DEBUG in the environment: no level is copied (A/B runs, tests).
 *
 * The rule is the kernel's own (csrc/a2amd_device.h: a2d_osc2_stage): a level is a candidate when its pads are
 * periodic, its size is a power of two and at most 128 entries; oscillator 0 is taken if it is a candidate, then
 * oscillator 1 if it is one and both fit in the 128 entries together.  Nothing is read back from the device, and there is no
 * per-batch count of staged oscillators: the host's shadow of an oscillator holds its wave, pitch and phase, but not
 * the amplitude, volume and pan rampers that decide on the device whether a listed voice is settled, and nothing at all
 * for the voices the device VM runs.  Callers apply the rule to the sizes they uploaded. */
#ifndef A2AMD_OSC2LDS_H
#define A2AMD_OSC2LDS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bit o set: oscillator o of a settled voice whose oscillators play levels of size0 / size1 entries reads its taps
 * from LDS (periodic0 / periodic1: that level's pads are periodic) */
unsigned a2amd_osc2_stage_rule(unsigned size0, int periodic0, unsigned size1, int periodic1);

/* 1: `level` - A2AMD_WAVEPRE pre-pad samples, size payload samples, A2AMD_WAVEPOST post-pad samples, as in
 * a2amd_wavedesc.data[] - has periodic pads: what a2amd_wave_upload() asks of every level of a looped wave */
int a2amd_wave_level_periodic(const int16_t *level, unsigned size);

#ifdef __cplusplus
}
#endif
#endif /* A2AMD_OSC2LDS_H */
