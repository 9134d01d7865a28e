/* a2amd_buswin.h - part of include/a2amd.h (which includes it): delay-chain bus owners in the batches in which
 * their only records are cut windows - who kept its fast kernel in the most recent batch, and who did not.
 *
 * A voice's VM that wakes inside a fragment cuts that fragment into windows, for the voice and - through inline -
 * for every bus owner nested below it: in a song the root wakes every 3 906 frames (core.c:1195), so the master
 * section gets R_SEG records for one fragment of nearly every player's buffer.  A bus owner with any record is the
 * general kernel's.  For the two delay-chain classes a run of windows alone need not be:
 *   - fbdelay never sees a window (fbdelay.c:69-126 is a loop over frames: the same delay lines, outputs and
 *     position whether it is called once for a fragment or once per window), and inline picks its children's sum
 *     out of a bus they have filled independently.  A wired delay chain (k_bus_fbdchain, a2amd_bus.h) whose records
 *     are windows only has them dropped, as a driver chain at rest has (a2amd_bus_info.driver_windows_dropped): it
 *     is k_bus_fbdchain's and counts in a2amd_bus_info.fbd_voices.
 *   - panmix sees a window through a2_PrepareRamper alone (a2_dsp.h:128-149), once per window and ramper: at rest
 *     every window sets the same gains, while a ramp is under way each window computes its own delta.  A pan-tailed
 *     chain (k_bus_fbdpan, a2amd_fbdpan.h) whose records are windows only keeps its run and goes to a second launch
 *     of k_bus_fbdpan, the windows launch, which ignores the run at rest and otherwise steps the rampers window by
 *     window - the clamp variant chosen per window - before the frames are rendered as in any other batch.  It is
 *     not on the general kernel's list and does not end the self-cleaning buses (a2amd_bus.h: consume).
 * A batch in which at least one chain was kept this way, and no bus owner is the general kernel's, may also have its
 * root store the master bus straight into the host's buffer (a2amd_bus.h: master_direct) although voices carry
 * records - a batch without any of this takes that path only without records, as before.
 * Both hold only where the windows cover each fragment exactly once and in order.  Records reach the library from
 * outside, so the host checks that: every record an R_SEG, sorted by fragment, the windows of a fragment starting at
 * frame 0, following each other without gap or overlap, none empty, and ending at the fragment's last frame.  A run
 * that does not tile (refused_tiling), and a pan-tailed chain's run that needs more than window_cap table rows - a
 * row per window, one for a fragment without a record - (refused_cap) are the general kernel's, as before.
 * The voice must be below the root, host-driven and of its class with the class switched on (A2AMD_NO_FAST bits 32 /
 * 512).  A2AMD_BUS_WINDOWS set in the environment switches all of this off together with the drivers' dropped
 * windows (A/B: every bus owner with records is the general kernel's).
 * The counts are the host's: what upload() listed and what the launch was given, not something read back from the
 * device (as in a2amd_bus.h). */
#ifndef A2AMD_BUSWIN_H
#define A2AMD_BUSWIN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct a2amd_ctx;

typedef struct a2amd_bus_windows_info {
	uint32_t fbd_dropped;     /* wired delay chains whose windows-only records were dropped: k_bus_fbdchain's, counted in a2amd_bus_info.fbd_voices */
	uint32_t fbdpan_voices;   /* pan-tailed chains whose windows-only run went to k_bus_fbdpan's windows launch */
	uint32_t fbdpan_gliding;  /* ... of which within the host's bound for a moving volume or pan (moving_until) */
	uint32_t fbdpan_windows;  /* table rows those runs need, summed */
	uint32_t refused_tiling;  /* windows-only runs of either class left to the general kernel: the windows do not tile their fragments */
	uint32_t refused_cap;     /* ... more rows than window_cap */
	uint32_t window_cap;      /* FBW_MAXWIN */
	uint32_t launched;        /* 1: the windows launch ran for the most recent batch */
} a2amd_bus_windows_info;     /* 32 bytes */
int a2amd_last_batch_bus_windows(const struct a2amd_ctx *ctx, a2amd_bus_windows_info *out);  /* NULL arguments refused */

#ifdef __cplusplus
}
#endif
#endif /* A2AMD_BUSWIN_H */
