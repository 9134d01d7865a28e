/* a2amd_bus.h - part of include/a2amd.h (which includes it): who rendered the bus owners of the most
 * recent batch - the voices with an inline unit, i.e. the root and the group voices.
 *
 * A bus owner goes to one of four kernels.  k_bus_driver takes the chain inline -> panmix 2->2 -> xinsert
 * (the engine's root and group drivers) and its mono form, inline 0 1 -> panmix 1->2 [-> xinsert] under a stereo bus,
 * whose one channel it reads twice (a mono root stays with the general kernel), k_bus_fbdchain the chain inline -> fbdelay [-> fbdelay ...] of at
 * most four delays whose taps are all between one fragment and the delay line less one fragment long, k_bus_fbdpan
 * the same chain with no delay wired and a wired, adding panmix 2->2 behind the last one (a2amd_fbdpan.h, which has
 * its counts: fbd_voices below stays the wired-delay chains), the
 * general kernel every other chain - and any bus owner in a batch in which it carries records, unless the records of
 * a delay chain of either kind are cut windows only (a2amd_buswin.h).  The counts
 * are the host's: what upload() listed for each kernel and what the launches were given, not something read
 * back from the device.  A test that names one of the bus kernels asserts them to prove it got there. */
#ifndef A2AMD_BUS_H
#define A2AMD_BUS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct a2amd_ctx;

typedef struct a2amd_bus_info {
	uint32_t driver_voices;          /* bus owners on k_bus_driver's lists that carry no record this batch */
	uint32_t driver_ramping;         /* ... of which this many may have begun the batch with a volume or pan ramper not
	                                  * at rest, by the host's bound: any write to the panmix, gliding or not, made at
	                                  * frame T (the frames of all fragments before the one it was made in or in front
	                                  * of) with start and dur counts until frame T + ((start + dur) >> 8) + 256, the
	                                  * margin being for the fragment the write falls into and for the window that
	                                  * settles the ramper.  These are given the kernel's launch of one workgroup a
	                                  * voice as well, which renders the ones that are in fact unsettled; the bound is
	                                  * generous, and the ones already at rest render on the split path like the others */
	uint32_t driver_windows_dropped; /* driver chains at rest whose records - cut windows only - were dropped this
	                                  * batch: they stayed with k_bus_driver and are counted in driver_voices */
	uint32_t fbd_voices;             /* bus owners on k_bus_fbdchain's lists that carry no record this batch, those whose
	                                  * windows-only records were dropped included (a2amd_bus_windows_info.fbd_dropped) */
	uint32_t generic_voices;         /* bus owners the general kernel rendered: by their class, or because they carry
	                                  * records this batch (a pan-tailed delay chain only in such a batch, and not where its
	                                  * run went to k_bus_fbdpan's windows launch) */
	uint32_t consume;                /* as given to the last bus launch: 0 the buses are cleared by a memset and the
	                                  * root adds into the master bus, 1 the bus kernels zero what they read, 3 ... and
	                                  * the root stores the master bus */
	uint32_t master_direct;          /* 1: the root's kernel stored the batch straight into the host's readback buffer */
} a2amd_bus_info;
/* (a batch replayed from a captured graph reports consume and master_direct as they were at its capture) */
int a2amd_last_batch_buses(const struct a2amd_ctx *ctx, a2amd_bus_info *out);

#ifdef __cplusplus
}
#endif
#endif /* A2AMD_BUS_H */
