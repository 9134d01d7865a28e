/* a2amd_osc3win.h - part of include/a2amd.h (which includes it): three-oscillator subtractive leads
 * (a2amd_osc3filt.h) in the batches in which their only records are cut windows - who kept the class's kernel in
 * the most recent batch, and who did not.
 *
 * A voice's VM that wakes inside a fragment cuts that fragment into windows for every descendant: in a song the
 * root wakes every 3 906 frames (core.c:1195), about every 61 fragments, so at a player's 64-fragment buffer
 * nearly every batch leaves each lead below it with a run of R_SEG records.  A lead with any run used to be the
 * general kernel's.  A run of windows alone need not be: every unit of the chain sees a window through
 * a2_PrepareRamper (a2_dsp.h:128-149), once per window and ramper, and through the frames it is asked for - so a
 * kernel that steps the pitch, amplitude, q, volume and pan rampers window by window, as the reference's
 * Process(offset, frames) calls would, renders the same bits.  That is k_leaf_osc3filtpan_win, the windows launch
 * of the class: the same workgroup as k_leaf_osc3filtpan, the windows read in place from the voice's run - no table,
 * so no cap on the windows of a voice.
 * Who goes there: a voice of the class, host-driven, none of whose oscillators left the mip-mapped waves in the
 * batch, without a filter in the batch's sweep table or a noise oscillator in a device-seeded stretch, whose run is
 * windows only and a tiling - every record an R_SEG, sorted by fragment, the windows of a fragment starting at
 * frame 0, following each other without gap or overlap, none empty, and ending at the fragment's last frame.
 * Records reach the library from outside, so the host checks that (as in a2amd_buswin.h).  A windows-only run that
 * does not tile (refused_tiling) is the general kernel's, as before, and so is any run with another record in it.
 * Such a voice keeps its run: it still counts in a2amd_osc3filt_batch_info.record_voices, the whole-fragment launch
 * skips it, and it stands on no other list - a2amd_batch_info.general_voices does not include it.  The unit
 * state the launch leaves is what either kernel of the class, or the general kernel, takes up in the next batch.
 * The switches, existing ones: bit 2048 of A2AMD_NO_FAST in the environment restores the old routing (A/B: every
 * lead with a run is the general kernel's); bit 1024 removes the class and with it this launch; A2AMD_F2VPW forces
 * the voices per workgroup of this launch too (1 .. 64; 0 or unset: a 256th of the window voices, 1 .. 64).
 * The counts are the host's: what upload() listed and what the launch was given, not something read back from
 * the device.  upload() resets them for every batch. */
#ifndef A2AMD_OSC3WIN_H
#define A2AMD_OSC3WIN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct a2amd_ctx;

typedef struct a2amd_osc3filt_windows_info {
	uint32_t launched;        /* 1: k_leaf_osc3filtpan_win ran for the most recent batch */
	uint32_t window_voices;   /* voices of the class whose windows-only run went to that launch */
	uint32_t gliding_voices;  /* ... of which with a ramper the host knows to be moving (moving_until beyond the batch's start) */
	uint32_t windows;         /* windows of those runs, summed: over a voice's fragments max(1, windows in the fragment) */
	uint32_t refused_tiling;  /* windows-only runs of the class left to the general kernel: the windows do not tile their fragments */
	uint32_t vpg;             /* voices per workgroup of the launch */
	uint32_t workgroups;      /* workgroups of the launch */
	uint32_t reserved;
} a2amd_osc3filt_windows_info;    /* 32 bytes */
int a2amd_last_batch_osc3filt_windows(const struct a2amd_ctx *ctx, a2amd_osc3filt_windows_info *out);  /* NULL arguments refused */

#ifdef __cplusplus
}
#endif
#endif /* A2AMD_OSC3WIN_H */
