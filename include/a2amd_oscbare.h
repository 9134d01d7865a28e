/* a2amd_oscbare.h - part of include/a2amd.h (which includes it): the quiet kernel of bare wtosc voices,
 * k_leaf_oscbare, and the mono group drivers on k_bus_driver - who rendered them in the most recent batch.
 *
 * The simplest voice a script declares, `struct { wtosc }`, is one oscillator wired straight into its
 * parent's bus: wired, adding, one output - it adds into channel 0 of that bus, whatever its width.  Such a
 * voice is a launch class of its own.  In a batch in which it carries no record it is rendered by
 * k_leaf_oscbare - lane = frame, the rampers of a glide in flight stepped by the kernel itself; in a batch
 * in which it carries records, and whenever its oscillator plays the noise generator, by the general kernel.
 * A voice the device VM runs (a2amd_vm_adopt) is not of the class while it stays there.
 * The usual parent of these voices, the mono group `inline 0 1; panmix 1 > 2` (with or without an xinsert
 * behind the panmix), is a driver chain like the stereo one: k_bus_driver reads its one channel twice.
 * A2AMD_NO_FAST bit 256 in the environment switches the class off (A/B: every such voice goes to the general
 * kernel, as before the class existed), bit 4 the driver chains, mono ones included; A2AMD_VPW forces the
 * kernel's voices per wavefront (1 .. 64).
 * The counts are the host's: what upload() listed and what the launch was given, not something read back
 * from the device (as in a2amd_bus.h). */
#ifndef A2AMD_OSCBARE_H
#define A2AMD_OSCBARE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct a2amd_ctx;

typedef struct a2amd_bare_batch_info {
	uint32_t launched;        /* 1: k_leaf_oscbare ran for the most recent batch */
	uint32_t class_voices;    /* voices in the class's leaf segment */
	uint32_t quiet_voices;    /* ... of which without a run this batch: the kernel's */
	uint32_t gliding_voices;  /* ... of which with a ramper the host knows to be moving (moving_until) */
	uint32_t record_voices;   /* ... of class_voices with records: the general kernel's (also in a2amd_batch_info.general_voices) */
	uint32_t vpw;             /* voices per wavefront of the launch */
	uint32_t mono_drivers;    /* bus owners on k_bus_driver's lists whose own bus has one channel */
	uint32_t reserved;
} a2amd_bare_batch_info;
int a2amd_last_batch_bare(const struct a2amd_ctx *ctx, a2amd_bare_batch_info *out);

#ifdef __cplusplus
}
#endif
#endif /* A2AMD_OSCBARE_H */
