/* a2amd_osc3filt.h - part of include/a2amd.h (which includes it): the quiet kernel of three-oscillator
 * subtractive leads, k_leaf_osc3filtpan - who rendered them in the most recent batch.
 *
 * The class: `struct { wtosc; wtosc o2; wtosc o3; filter12; panmix }` - five units; the first wtosc replacing,
 * the second and third adding, none of them wired, each on a mip-mapped wave or off; a one-channel filter12,
 * replacing, not wired; a panmix 1 -> 2, wired and adding into an output bus of two channels or more.  A voice
 * the device VM runs (a2amd_vm_adopt) is not of the class while it stays there, nor is one with an
 * oscillator on the noise generator.
 * Who renders what: a voice of the class without a run in a batch - no record of its own, no filter with a
 * column of the batch's sweep table, no device-seeded noise window - is rendered by k_leaf_osc3filtpan, settled
 * or gliding: the kernel steps the pitch, amplitude, q, volume and pan rampers itself, fragment by fragment,
 * and the class is given no stand-in record for a glide.  A voice with any run is the general kernel's, as
 * every such voice was before the class existed; the unit state either kernel leaves is the other's to take
 * up in the next batch.  The kernel is launched only when the class has a voice without a run.
 * The one exception among the runs (a2amd_osc3win.h): a run of cut windows alone that tile the fragments keeps
 * the voice with its class - a second launch, k_leaf_osc3filtpan_win, renders it.  Such a voice still counts in
 * record_voices here (it has a run; launched, vpg and workgroups describe the whole-fragment launch only), but it
 * is not on the general kernel's list: a2amd_batch_info.general_voices no longer includes it.
 * The two switches, both existing ones: bit 1024 of A2AMD_NO_FAST in the environment switches the class off
 * (A/B: every such voice is CLS_GENERIC again); A2AMD_F2VPW forces the kernel's voices per workgroup
 * (1 .. 64; 0 or unset: one workgroup per 256th of the class, at least 1 and at most 64 voices each).
 * Out of scope: a voice of the class whose run holds anything but windows, or windows that do not tile, goes to
 * the general kernel; the device VM and the window kernels do not know the chain; noise on any of the three oscillators,
 * a cutoff sweeping inside the kernel, three oscillators without a filter and more than three oscillators are
 * other shapes; there is no launch threshold.
 * The counts are the host's: what upload() listed and what the launch was given, not something read back
 * from the device (as in a2amd_oscbare.h). */
#ifndef A2AMD_OSC3FILT_H
#define A2AMD_OSC3FILT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct a2amd_ctx;

typedef struct a2amd_osc3filt_batch_info {
	uint32_t launched;        /* 1: k_leaf_osc3filtpan ran for the most recent batch */
	uint32_t class_voices;    /* voices in the class's leaf segment */
	uint32_t quiet_voices;    /* ... of which without a run this batch: the kernel's */
	uint32_t gliding_voices;  /* ... of which with a ramper the host knows to be moving (moving_until beyond the batch's start) */
	uint32_t record_voices;   /* ... of class_voices with any run: the general kernel's (also in a2amd_batch_info.general_voices), less those of the windows launch (a2amd_osc3filt_windows_info.window_voices) */
	uint32_t vpg;             /* voices per workgroup of the launch */
	uint32_t workgroups;      /* workgroups of the launch */
	uint32_t reserved;
} a2amd_osc3filt_batch_info;
int a2amd_last_batch_osc3filt(const struct a2amd_ctx *ctx, a2amd_osc3filt_batch_info *out);

#ifdef __cplusplus
}
#endif
#endif /* A2AMD_OSC3FILT_H */
