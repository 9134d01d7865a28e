/* a2amd_fbdpan.h - part of include/a2amd.h (which includes it): the quiet kernel of delay chains that end in a
 * panmix, k_bus_fbdpan - who rendered them in the most recent batch.
 *
 * The master section of most songs is `struct { inline 0 *; fbdelay * *; [fbdelay * *; ...] panmix * > }`: a stereo
 * bus, one to four fbdelay units, none of them wired (any of them may be in adding mode), and a panmix 2->2 that is
 * wired and adds into the parent's bus.  With every tap of every delay between one fragment and the delay line less
 * one fragment long, such a bus owner below the root is a launch class of its own.  In a batch in which it carries
 * no record it is rendered by k_bus_fbdpan - k_bus_fbdchain's rounds of floor(min(tap) / 64) fragments, 1 024 threads
 * over a round's frames, then panmix_process22 on each frame: with constant gains where volume and pan are at rest,
 * and where they are not, with the rampers stepped through the batch's fragments by one thread first, which also
 * stores their end state.  In a batch in which it carries records - a write to any of its units is one - it is the
 * general kernel's, like every bus owner - except where the records are cut windows only and tile their fragments: then
 * the voice keeps its run and is rendered by a second launch of k_bus_fbdpan, the windows launch, which steps the
 * rampers window by window (a2amd_buswin.h has the conditions and the counts).  A tap written out of that range makes the chain a general bus owner
 * until a tap write brings it back.  A root of this shape, a mono owner and a chain with any other unit in it
 * (a waveshaper in front of the delays) stay with the general kernel.
 * The class counts as a fast owner for the self-cleaning buses (a2amd_bus.h: consume), like the wired delay chains.
 * A2AMD_NO_FAST bit 512 in the environment switches the class off (A/B: every such voice is a general bus owner,
 * as before the class existed).
 * The counts are the host's: what upload() listed and what the launch was given, not something read back from the
 * device (as in a2amd_bus.h). */
#ifndef A2AMD_FBDPAN_H
#define A2AMD_FBDPAN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct a2amd_ctx;

typedef struct a2amd_fbdpan_batch_info {
	uint32_t launched;        /* 1: k_bus_fbdpan ran for the most recent batch (either of its launches) */
	uint32_t class_voices;    /* bus owners of the class on the depth lists */
	uint32_t quiet_voices;    /* ... of which without a run this batch: the kernel's (its launch over the class) */
	uint32_t gliding_voices;  /* ... of which within the host's bound for a moving volume or pan (a2amd_bus.h: driver_ramping's bound) */
	uint32_t record_voices;   /* ... of class_voices with records this batch: the general kernel's (also in a2amd_bus_info.generic_voices), less those a2amd_last_batch_bus_windows().fbdpan_voices counts */
	uint32_t max_delays;      /* longest chain of the class in the batch (1..4) */
	uint32_t reserved[2];
} a2amd_fbdpan_batch_info;    /* 32 bytes */
int a2amd_last_batch_fbdpan(const struct a2amd_ctx *ctx, a2amd_fbdpan_batch_info *out);

#ifdef __cplusplus
}
#endif
#endif /* A2AMD_FBDPAN_H */
