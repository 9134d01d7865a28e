/*
 * a2amd_vmbatch.h - who ran the device VM's voices (include/a2amd_vm.h) in the most recent batch, in the manner of
 * a2amd_last_batch_bare / a2amd_last_batch_buses: what the host decided for it.  Nothing is read back from the device for
 * this, and nothing the kernels see changes.
 *
 * (A header of its own, included at the end of a2amd.h like its siblings - not part of a2amd_vm.h: liba2amd_walk.so is
 * stamped with that header's contents and can be rebuilt only where the engine's source tree is, build.build_walk.)
 *
 *   fused        the VMs of the class voices ran in the lane that carries their writes out: in a k_vm_win of this batch,
 *                or in the speculative pass this batch took (spec_taken).  0: through records (k_vm_count / k_vm_emit,
 *                like other_voices in every batch) - not_fused says why
 *   not_fused    0 fused (or no class voices); 1 no prediction stood, 2 other lists than predicted, 3 another time,
 *                4 another length, 5 a fragment across a predicted 64-frame boundary; A2AMD_VM_NOT_ASKED: the window
 *                kernels or k_vm_win are switched off (A2AMD_WIN / A2AMD_VMWIN), or k_vm_win has been given up
 *   spec_valid   a speculative pass had been run for the batch expected behind the last one
 *   spec_taken   ... and this batch was that batch: k_vm_commit in k_vm_win's place
 *   spec_miss    a valid pass not taken: 1 the batch was not the one predicted (not_fused says how), 2 other fragments
 *                or class counts, 3 the pass ran out of pool room, 4 a voice faulted in it
 *   spec_next    a pass for the batch expected next was launched behind this one
 *   spec_why_not ... or not: 1 switched off / too short a batch / no class voices, 2 no plan (the span is not whole
 *                64-frame fragments, or two announced cuts inside one), 3 over the slot budget, 4 the lists have only
 *                just changed
 *   records      records k_vm_emit made (0: it did not run)
 *   idle_known, idle[]  with spec_taken: the voices of each class the pass left to the quiet kernels
 *   quiet_launched[]    the quiet kernel of each class was launched this batch: it renders the class voices that have no
 *                run in it - the idle ones among the VM's (not launched where a taken pass says there are none, A2AMD_VMSKIP)
 */
#ifndef A2AMD_VMBATCH_H
#define A2AMD_VMBATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct a2amd_ctx;

#define A2AMD_VM_NOT_ASKED 6
typedef struct a2amd_vm_batch_info {
	uint32_t listed;		/* voices on the device VM's list */
	uint32_t class_voices[3];	/* ... of wtosc-panmix, 2 x wtosc-panmix, wtosc-filter12-panmix */
	uint32_t other_voices;		/* ... of any other chain */
	uint32_t pending;		/* adopted during this batch: carried to its end by the host */
	uint32_t fused, not_fused;
	uint32_t spec_valid, spec_taken, spec_miss;
	uint32_t spec_next, spec_why_not;
	uint32_t records;
	uint32_t idle_known, idle[3];
	uint32_t quiet_launched[3];	/* the class's quiet kernel (k_leaf_oscpan / _osc2pan / _oscfiltpan) was launched over its voices */
} a2amd_vm_batch_info;
int a2amd_last_batch_vm(const struct a2amd_ctx *ctx, a2amd_vm_batch_info *out);

#ifdef __cplusplus
}
#endif
#endif /* A2AMD_VMBATCH_H */
