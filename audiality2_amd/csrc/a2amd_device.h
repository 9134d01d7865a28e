// a2amd_device.h - data layout shared by the host recorder and the HIP kernels.
//
// Everything the kernels touch lives in a handful of flat device arrays; the
// host owns the *structure* (which units form a voice, where a voice's output
// lands), the device owns the *signal state* (phases, rampers, filter and
// delay memories) and only ever changes it by executing command records.
#pragma once
#include <stdint.h>

#define A2D_MAXCHAIN   16     // units per voice (A2AMD_MAXCHAIN).  Round 6: 8 -> 16, what a record's 4-bit chain position
			      // (A2D_RUNIT) addresses; the reference's unit list has no cap (core.c:163-300)
#define A2D_CHAIN_INLINE 8    // ... of which the voice record (A2DVoice: one 64-byte line that every kernel reads per voice) holds
			      // the first 8; units 8 - 15 of a longer chain stand in a side array only the general kernel reads
			      // (A2DVoiceExt).  (First cut: unit[16] in the record itself, 96 bytes - k_leaf_oscfiltpan 0.5539 against
			      // 0.5505 ms, k_leaf_osc2pan 2.198 against 2.186 ms, same box, interleaved x 3: profiles/r06_maxchain_ab.txt)
#define A2D_MAXBATCH 256
#define FBW_MAXWIN (2 * A2D_MAXBATCH)	// k_bus_fbdpan's windows launch: table rows (windows) per voice and batch, in LDS
#define A2D_USTATE    24      // int32 words of device state per unit
#define A2D_MAXCH      8
#define A2D_FRAG      64
#define A2D_MIPS      10
#define A2D_FBD_BUFSIZE 131072          // fbdelay.c:27
#define A2D_MAXPHINC  512               // a2_waves.h:57
#define A2D_COEF_WORDS 3                 // words per entry of the Hermite coefficient table (a2amd_fast.hip)
#define A2D_WTOSC_MAXLENGTH (0x01000000 - 1 - 131)   // wtosc.c:55

// unit kinds: numerically equal to a2amd_unitkind
enum { A2D_WTOSC = 0, A2D_PANMIX, A2D_FILTER12, A2D_FBDELAY, A2D_INLINE, A2D_XINSERT,
	A2D_FM1, A2D_FM2, A2D_FM3, A2D_FM4, A2D_FM3P, A2D_FM4P, A2D_FM2R, A2D_FM4R,
	A2D_DC, A2D_WAVESHAPER, A2D_DCBLOCK, A2D_LIMITER, A2D_XSINK, A2D_XSOURCE };
#define A2D_IS_FM(k) ((k) >= A2D_FM1 && (k) <= A2D_FM4R)

// wtosc Process variants (the reference swaps u->Process, wtosc.c:433-483)
enum { A2D_OSC_OFF = 0, A2D_OSC_NOISE, A2D_OSC_WAVE, A2D_OSC_MIPWAVE };

// packed static description of a unit instance (host owned)
//   bits 4 add (A2_PROCADD), 8-11 ninputs, 12-15 noutputs, 16 wired out, 24-31 kind
#define A2D_DESC(kind, add, nin, nout, wired) \
	(((uint32_t)(kind) << 24) | ((uint32_t)(add) << 4) | ((uint32_t)(nin) << 8) | \
	 ((uint32_t)(nout) << 12) | ((uint32_t)(wired) << 16))
#define A2D_KIND(d)  ((d) >> 24)
#define A2D_ADD(d)   (((d) >> 4) & 1u)
#define A2D_NIN(d)   (((d) >> 8) & 15u)
#define A2D_NOUT(d)  (((d) >> 12) & 15u)
#define A2D_WIRED(d) (((d) >> 16) & 1u)

// device unit state word indices ------------------------------------------
// ramper = 4 consecutive words {value, target, delta, timer} (a2_dsp.h:105)
enum {	// wtosc (A2_wtosc, wtosc.c:66-80)
	OW_MODE = 0, OW_WAVE, OW_DPHASE, OW_PHASE_LO, OW_PHASE_HI, OW_NOISE,
	OW_PRAMPING, OW_P = 7, OW_A = 11, OW_SEED = 15 };
enum {	// panmix (A2_panmix, panmix.c:35-40)
	PW_VOL = 0, PW_PAN = 4 };
enum {	// filter12 (A2_filter12, filter12.c:36-56); the cutoff ramper and the
	// float coefficient maths stay on the host, which ships f1 values
	FW_Q = 0, FW_LP = 4, FW_BP, FW_HP, FW_F1, FW_D1A, FW_D1B, FW_D2A, FW_D2B,
	FW_F1NEXT, FW_RAMP };
enum {	// fbdelay (A2_fbdelay, fbdelay.c:41-60)
	DW_FBDELAY = 0, DW_LDELAY, DW_RDELAY, DW_DRYGAIN, DW_FBGAIN, DW_LGAIN,
	DW_RGAIN, DW_BUFPOS, DW_BUFIDX };

enum {	// dc (A2_dc, dc.c:42-47)
	CW_VALUE = 0, CW_MODE = 4 };
enum {	// waveshaper (A2_waveshaper, waveshaper.c:44-48)
	SW_AMOUNT = 0 };
enum {	// dcblock (A2_dcblock, dcblock.c:33-49); the host ships f1
	BW_F1 = 0, BW_D1A, BW_D1B, BW_D2A, BW_D2B };
enum {	// limiter (A2_limiter, limiter.c:35-42); release / threshold computed by the host
	LW_RELEASE = 0, LW_THRESHOLD, LW_PEAK };
enum {	// fm (A2_fm, fm.c:95-105): the operators live in a pool of their own
	// (fmstate[slot][A2D_FMSTATE]); the unit's state words only name the slot
	MW_SLOT = 0 };
enum {	// one operator (A2_fmosc, fm.c:84-93), A2D_FMSTATE / 4 words
	FO_A = 0, FO_FB = 4, FO_P = 8, FO_LASTPITCH = 12, FO_PHASE, FO_DPHASE, FO_LAST, FO_WORDS };
#define A2D_FMSTATE 64

// A2DWave::flags, beside the engine's own (A2_LOOPED 0x100 ...): the settled wtosc -> panmix kernel reads this
// wave's samples themselves instead of its Hermite coefficient entries (a2amd_wave_upload decides)
#define A2D_WF_RAWTAPS 0x40000000u

// mirror of A2_wave for the device: offsets index the int16 wave pool and point
// at the first PAYLOAD sample of a level (i.e. data[level] + A2_WAVEPRE)
struct A2DWave {
	int32_t  type;
	uint32_t flags;
	uint32_t period;
	uint32_t size[A2D_MIPS];
	uint32_t off[A2D_MIPS];
	// (two half words in the place of the one word 'periodic' had before 'tame' came: A2D_MIPS bits each, and the struct
	// keeps its 96 bytes - every kernel that indexes waves[] keeps its instructions)
	uint16_t periodic;	// bit l: level l's pads are the periodic continuation of its payload (a2amd_wavepads.h; set by
				// a2amd_wave_upload from the samples it is handed, clear for the waves the device renders)
	uint16_t tame;		// bit l: no product of a2_Hermite wraps anywhere in level l (a2amd_wavetame.h; set and cleared as periodic is)
};

static_assert(A2D_MIPS <= 16 && sizeof(A2DWave) == 96, "A2DWave: a bit per level in a half word, 96 bytes");

// one voice = one unit chain (host owned)
struct A2DVoice {
	int32_t nunits;
	int32_t unit[A2D_CHAIN_INLINE];	// indices into udesc[] / ustate[]; the chain's further units: A2DVoiceExt
	int32_t out_off, out_nch;	// bus the wired outputs add into (int32 offset into busmem)
	int32_t own_off, own_nch;	// bus our 'inline' unit collects children in, or -1
	int32_t pad[3];
};

static_assert(sizeof(A2DVoice) == 64, "the voice record is one 64-byte line");
struct A2DVoiceExt { int32_t unit[A2D_MAXCHAIN - A2D_CHAIN_INLINE]; };	// [voice slot], where a context has a chain > 8 units

// command record, 16 bytes
struct A2DRec {
	uint32_t head;		// frag:16 | op:8 | unit:4 | reg:4
	int32_t  value;
	uint32_t dur;		// SEG: offset | frames << 16
	uint32_t start;
};
enum { R_SEG = 1, R_WRITE, R_INIT, R_KILL, R_F1SET, R_F1RAMP, R_NOISESEED, R_NOP };
#define A2D_HEAD(frag, op, unit, reg) \
	((uint32_t)(frag) | ((uint32_t)(op) << 16) | ((uint32_t)(unit) << 24) | ((uint32_t)(reg) << 28))
#define A2D_RFRAG(h) ((h) & 0xffffu)
#define A2D_ROP(h)   (((h) >> 16) & 0xffu)
#define A2D_RUNIT(h) (((h) >> 24) & 15u)
#define A2D_RREG(h)  (((h) >> 28) & 15u)

struct A2DRun { int32_t first, count; };

// ---- the scripted voice's VM on the device (include/a2amd_vm.h) ----------------
// One per adopted voice, device resident (the device is the authority on everything in it
// between adoption and recall): A2_vmstate (include/a2_vm.h:62-69), where a2_VoiceControl
// (core.c:143-149) sends each VM register, and the cutoff rampers of the voice's filter12 units,
// which for host-driven voices never leave the host (a2amd_host.h: HUnit::cutoff).
#define A2D_VM_NOWRITE 0xffu
#define A2D_VM_TRAPWRITE 0xfeu		// cmap: wired to something the device VM cannot write - the voice leaves before it would
#define A2D_VM_MAXCUT  2
#define A2D_VM_MAXENV  2
#define A2D_VM_MAXPOS  8		// chain positions the device VM's register map can name (cmap, A2DVmEnv::target: a nibble, of which 14 and
				// 15 mean something else): a voice with a longer chain stays the engine thread's (a2amd_vm_adopt)
#define A2D_VM_ENVPOS  14		// cmap chain position that stands for "the target register of env unit <register nibble>"
#define A2D_ENV_LUTSHIFT 6		// A2ENV_LUTSHIFT, env.c:27
#define A2D_ENV_LUTSIZE  (1 << A2D_ENV_LUTSHIFT)
#define A2D_ENV_LUTS     8		// A2ENVLUT_SPLINE, EXP1 .. EXP7 (env.c:36-47)
// src/units/env.c's A2_env (:88-99) for a voice the device VM runs: a control-rate unit without audio
// ports whose output is a register write on another unit through a control wire (env.c:135)
struct A2DVmEnv {
	int32_t ramper[4];		// A2_env.ramper
	int32_t lut;			// which table (A2ENVLUT_*)
	int32_t scale, offset, out;
	int32_t active;			// its Process is env_ProcessLUT (else env_ProcessOff)
	uint8_t regbase;		// VM register of its 'target' (then mode, down, time: env.c:50-56, registers[] = &vms->r[regbase])
	uint8_t k;			// units of the (backend) chain in front of it: a write to one of them takes effect behind the window
	uint8_t target;			// where its control output is wired: chain position << 4 | register, A2D_VM_NOWRITE = nowhere
	uint8_t pad;
};
struct A2DVmVoice {
	uint32_t waketime;		// A2_vmstate.waketime: 24:8 frames, engine time
	uint32_t code, ncode;		// the function's text in the code pool (32 bit words)
	uint16_t pc;
	uint8_t  state, ncut;
	int32_t  voice;			// backend voice slot (runs[] index)
	int32_t  fault;			// a trap the analysis should have ruled out (0 = none): the VM stopped there
	uint8_t  cmap[64];		// VM register -> chain position << 4 | unit register, A2D_VM_NOWRITE = none
	uint8_t  kind[A2D_MAXCHAIN];	// unit kinds of the chain
	uint8_t  cutpos[A2D_VM_MAXCUT];	// chain positions of the filter12 units whose cutoff the VM may write
	uint8_t  pad[2];
	int32_t  cut[A2D_VM_MAXCUT][4];	// ... and their cutoff rampers (A2_filter12.cutoff, filter12.c:38)
	A2DVmEnv env[A2D_VM_MAXENV];	// the voice's env units, nenv of them
	int32_t  nenv;
	uint32_t exit_when;		// has_exit: the VM run that starts at this wake time is the engine's (a2amd_vm_exit_time):
	int32_t  has_exit;		// the device VM stops in front of it (the walk has recalled the voice by then)
	int32_t  r[64];			// A2_vmstate.r
};

// what the VM kernel needs beside the voices (host copy: a2amd_ctx)
struct A2DVmParams {
	A2DVmVoice     *vmv;		// [vm slot]
	const int      *list;		// vm slots the kernel runs this batch
	int32_t         n;
	const uint32_t *code;		// code pool
	const uint32_t *ptab;
	const int32_t  *f1tab;		// [32][65536]: f12_pitch2coeff by (shift, fraction), or null
	const uint16_t *envlut;		// [A2D_ENV_LUTS][A2D_ENV_LUTSIZE + 2] (env.c:218-257), or null
	A2DRun         *runs;		// [voice slot]
	A2DRun         *vmrun;		// [list index]: where each voice's records go (count pass -> emit pass)
	A2DRec         *recs;		// the batch's record array (A2DParams::recs)
	uint32_t        rec_base, rec_cap;	// the VM's region of it, in records
	uint32_t       *total;		// records the count pass found; [1] = voices that faulted
	uint32_t        now;		// engine time of the batch's first frame
	uint32_t        msdur;		// A2_state.msdur
	int32_t         samplerate, basepitch;
	int32_t         nfrags;
	uint8_t         fragframes[A2D_MAXBATCH];
	uint8_t         fragbase[A2D_MAXBATCH];	// offset of each inside the engine's own fragment (core.c:1968)
};

// xinsert state words: client slot + 1 (0 = no clients) and A2AMD_XIO_* mode bits
enum { XW_SLOT = 0, XW_MODE = 1 };
#define A2D_XIO_HALF ((size_t)A2D_MAXBATCH * 8 * A2D_FRAG)	// words per direction of a slot
#define A2D_XIO_SLOT (2 * A2D_XIO_HALF)

#define A2D_FAST_FCH 8	// k_leaf_oscpan: fragments per chunk (the host sizes the time slices by it)
#define A2D_OSC2_FCH 4	// k_leaf_osc2pan: fragments per chunk
#define A2D_OSC2_SCH 16	// ... and per super-chunk (a multiple of the chunk): what a wavefront keeps bus sums for in LDS
#define A2D_OSC2_LDS_ENT 128	// ... and coefficient entries a wavefront may keep in LDS for the voice it walks (1 536 bytes)
#define A2D_MAXVPW   32       // voices one wavefront may walk per fragment

struct A2DParams {
	const A2DVoice *voices;
	const A2DVoiceExt *vext;	// units 8 - 15 of the chains that have them, or null (no such chain in the context)
	const uint32_t *udesc;
	int32_t        *ustate;		// [unit][A2D_USTATE]
	int32_t        *vactive;	// [voice slot]
	const A2DRun   *runs;		// [voice slot], this batch
	const A2DRec   *recs;
	const A2DWave  *waves;
	const int16_t  *wavepool;
	const int32_t  *wavecoef;	// [wave pool index][A2D_COEF_WORDS]: Hermite a, b, c:d0 of the window at that sample
	int32_t        *busmem;
	int32_t        *fbdmem;		// [bufidx][2][A2D_FBD_BUFSIZE]
	const uint32_t *ptab;		// 64 x {base, coeff}, pitch.c:70-96
	int32_t        *fmstate;	// [fm slot][A2D_FMSTATE]
	const uint32_t *fmsine;		// 2048 x {s[i], s[i+1]-s[i]} packed 16:16, fm.c:493-501
	int32_t *xio;			// xinsert client slots: [slot]{ tap[batch][ch][64], inject[batch][ch][64] }
	const uint32_t *nseed;		// [fragment][nnoise]: the engine's RNG word in front of a noise oscillator's default window, where
					// the batch has device-seeded fragments (a2amd_fragment_repeat_noise; k_noise_seeds), or null
	const int32_t  *nslot;		// [unit]: the oscillator's column of nseed + 1 (0: none; only read where nseed is set)
	int32_t         nnoise;
	const int32_t  *cutf;		// [fragment][ncut]: the coefficient behind a sweeping filter12's default window, or a negative word
					// ("no ramp in this window"), where the batch has stretches with cutoff sweeps (k_cut_sweep), or null
	const int32_t  *cslot;		// [unit]: the filter's column of cutf + 1 (0: none; only read where cutf is set)
	int32_t         ncut;
	int32_t         nfrags;
	int32_t         samplerate;
	int32_t         debug;		// A2AMD_DEBUG ablation bits (perf experiments only)
	uint8_t         fragframes[A2D_MAXBATCH];
	uint16_t        fragstart[A2D_MAXBATCH];	// frames before each fragment
	// (last: the members above keep the offsets every other kernel was compiled with)
	const int32_t  *wavecoef4;	// [wave pool index][4]: a, b << 8, c << 8, d0 << 8 of the window at that sample, for the fused steps on
					// tame levels (a2amd_wavetame.h; k_leaf_osc2pan), or null: the pool outgrew the footprint policy's entries
};

// How k_leaf_osc2pan walks a batch, for the kernel and for the host's report of it (include/a2amd_osc2.h) alike.
// Time slice 'slice' of 'ysplit' takes the chunks [*c_lo, *c_hi) of A2D_OSC2_FCH fragments, *nslices of the ysplit
// have any; false: this one is empty.
#ifdef __HIPCC__
#define A2D_HD static inline __host__ __device__
#else
#define A2D_HD static inline
#endif
A2D_HD bool a2d_osc2_slice(int nfrags, int ysplit, int slice, int *c_lo, int *c_hi, int *nslices)
{
	const int nchunks = (nfrags + A2D_OSC2_FCH - 1) / A2D_OSC2_FCH;
	const int per = (nchunks + ysplit - 1) / ysplit;
	*c_lo = slice * per;
	*c_hi = *c_lo + per < nchunks ? *c_lo + per : nchunks;
	*nslices = (nchunks + per - 1) / per;
	return *c_lo < nchunks;
}
// A slice is walked in super-chunks of at most A2D_OSC2_SCH fragments, counted from its first chunk.  One whose n
// fragments are all whole - A2D_FRAG frames each, so together n * A2D_FRAG: no fragment is longer - is walked voice by
// voice; one that holds a shorter fragment (a cut window) chunk by chunk.  From the frames before its first and its
// last fragment and that last one's length.
A2D_HD bool a2d_osc2_whole(unsigned start_first, unsigned start_last, unsigned frames_last, int n)
{
	return start_last + frames_last - start_first == (unsigned)n * A2D_FRAG;
}

// Which of a settled voice's two oscillators read their taps from the wavefront's copy of the level in LDS on the
// voice-major walk: bit o = oscillator o.  A level is a candidate when its pads are periodic (A2DWave::periodic), so that
// its payload entries indexed modulo the size are all a tap can reach (a2amd_wavepads.h), the size is a power of two -
// the modulus is a bit field - and at most A2D_OSC2_LDS_ENT.  Oscillator 0 first, then oscillator 1 if both still fit.
A2D_HD unsigned a2d_osc2_stage(unsigned size0, unsigned periodic0, unsigned size1, unsigned periodic1)
{
	const bool c0 = periodic0 && size0 && !(size0 & (size0 - 1)) && size0 <= A2D_OSC2_LDS_ENT;
	const bool c1 = periodic1 && size1 && !(size1 & (size1 - 1)) && size1 <= A2D_OSC2_LDS_ENT;
	return (c0 ? 1u : 0u) | (c1 && (c0 ? size0 : 0u) + size1 <= A2D_OSC2_LDS_ENT ? 2u : 0u);
}

// Does a settled voice of k_leaf_osc2pan's voice-major walk take the fused multiply-add steps (a2amd_taps.h:
// hermite_fused)?  When both its oscillators play tame levels (A2DWave::tame).  Its staged levels (a2d_osc2_stage, the
// same rule and the same masks for both kinds of voices) are then copied to LDS as 16 byte entries: A2D_OSC2_LDS_ENT of
// them are 2 048 bytes a wavefront, and the kernel's four workgroups still fit a CU's 160 KiB together.
A2D_HD unsigned a2d_osc2_tame(unsigned tame0, unsigned tame1)
{
	return tame0 && tame1 ? 1u : 0u;
}

// The launch shape both kernels of the class take: voices per wavefront within a wavefront's lanes, and one slice
// where nothing can be staged for a commit.
A2D_HD void a2d_osc2_shape(int *vpw, int *ysplit, bool can_stage)
{
	*vpw = *vpw < 1 ? 1 : (*vpw > 64 ? 64 : *vpw);
	if(*ysplit < 1 || !can_stage)
		*ysplit = 1;
}

// ---- k_leaf_osc2tame (a2amd_osc2tame.hip): the kernel of whole wavefronts of settled, tame, power-of-two voices ----
// It is launched in front of k_leaf_osc2pan, with that kernel's shape, for a class of at least A2D_OSC2TAME_MIN voices
// (fewer: the second launch costs more than the walk saves; profiles/osc2_tame_kernel.md) in a batch all of whose
// super-chunks are whole in every slice: frames[f] of the nfrags fragments, by the kernel's own rule.
#define A2D_OSC2TAME_MIN 1024
A2D_HD bool a2d_osc2_all_whole(const unsigned *frames, int nfrags, int ysplit)
{
	if(nfrags <= 0 || ysplit < 1)
		return false;
	for(int slice = 0; slice < ysplit; ++slice) {
		int c_lo, c_hi, nslices;
		if(!a2d_osc2_slice(nfrags, ysplit, slice, &c_lo, &c_hi, &nslices))
			break;
		for(int s_lo = c_lo; s_lo < c_hi; s_lo += A2D_OSC2_SCH / A2D_OSC2_FCH) {
			const int s_hi = s_lo + A2D_OSC2_SCH / A2D_OSC2_FCH < c_hi ? s_lo + A2D_OSC2_SCH / A2D_OSC2_FCH : c_hi;
			const int fa = s_lo * A2D_OSC2_FCH, fb = s_hi * A2D_OSC2_FCH < nfrags ? s_hi * A2D_OSC2_FCH : nfrags;
			unsigned n = 0;
			for(int f = fa; f < fb; ++f)
				n += frames[f];
			if(!a2d_osc2_whole(0, n - frames[fb - 1], frames[fb - 1], fb - fa))
				return false;
		}
	}
	return true;
}
// One voice, from its state at the batch's start.  records: runs[slot].count; osc0, osc1: a2s_osc_settled() of its
// oscillators; pan: a2s_arrived() of the panmix's rampers; waves: settled_wave() of both (a2s_wave_ok); tame0, tame1:
// A2DWave::tame's bits of the two levels (a2d_osc2_tame); size, dph: the levels' sizes and increments; ph: the phases AT
// the levels (the state's phase >> the level); frames: the batch's, nfrags * A2D_FRAG.
// The sizes are powers of two - the modulus is a mask - and both phases stay on the mask branch of the general kernel's
// chunk (osc2_chunk: !(ph >> 48)) wherever that kernel would test them: at a super-chunk's first chunk, ph + before * dph
// with before <= frames, and at every later chunk a wrapped phase plus a fragment's increments, below
// (size << 24) + A2D_FRAG * dph.
A2D_HD bool a2d_osc2tame_voice(unsigned records, bool osc0, bool osc1, bool pan, bool waves, unsigned tame0, unsigned tame1,
		unsigned size0, unsigned size1, unsigned dph0, unsigned dph1, uint64_t ph0, uint64_t ph1, unsigned frames)
{
	if(records || !(osc0 && osc1 && pan && waves) || !a2d_osc2_tame(tame0, tame1))
		return false;
	if(!size0 || (size0 & (size0 - 1)) || !size1 || (size1 & (size1 - 1)))
		return false;
	if((ph0 >> 48) || (ph1 >> 48))
		return false;
	if(((ph0 + (uint64_t)frames * dph0) >> 48) || ((ph1 + (uint64_t)frames * dph1) >> 48))
		return false;
	return !((((uint64_t)size0 << 24) + (uint64_t)A2D_FRAG * dph0) >> 48) && !((((uint64_t)size1 << 24) + (uint64_t)A2D_FRAG * dph1) >> 48);
}
// ... and the wavefront: every one of its nv voices (ok: bit v = a2d_osc2tame_voice() of voice v, no bit from nv on)
A2D_HD bool a2d_osc2tame_wave(unsigned long long ok, int nv)
{
	return nv >= 1 && nv <= 64 && ok == (nv == 64 ? ~0ull : (1ull << nv) - 1);
}

// A noise oscillator's default window - a fragment without records for its voice - takes the engine's RNG word from
// the batch's seed table (a window the engine called for carries an R_NOISESEED record instead).
// Invariant (the host's: a2amd_fragment_repeat_noise, upload()): in a batch with nseed set, a noise oscillator meets a
// fragment without records for its voice only inside a stretch that lists it - every other window of a noise oscillator
// is one the engine called for - so the cell read here was written by the seed pass.  nslot is cleared for every such
// batch before the pass fills it in: an oscillator without a column in THIS batch reads 0 and keeps its seed.
#ifdef __HIPCC__
static inline __host__ __device__ bool a2d_noise_seed(const A2DParams &p, int f, int ui, unsigned *seed)
{
	if(!p.nseed)
		return false;
	const int k = p.nslot[ui];
	if(k <= 0 || k > p.nnoise)
		return false;
	*seed = p.nseed[(size_t)f * (size_t)p.nnoise + (size_t)(k - 1)];
	return true;
}
#endif

// A filter12's default window - a fragment without records for its voice - takes what an R_F1RAMP record would have
// brought from the batch's sweep table: true and *f1 = the coefficient behind the window when the cutoff ramper moved in
// it (the caller sets f1next and ramp, as for the record), false - nothing changes - when it did not, or the filter has
// no column.
// Invariant (the host's: a2amd_fragment_repeat[_noise], upload()): a filter with cutoff_moving() meets a fragment
// without records for its voice only inside a stretch that lists it - in a fragment walked by calls its Process call
// leaves an R_F1RAMP record whenever the ramper moves, and a window in which it only snaps changes no coefficient - and
// the quiet kernels, which never ask, never see its voice (upload() gives it the stand-in run).  Every cell of the table
// is set to the marker and cslot is cleared for every batch that has a table, before the pass fills them in: a filter
// without a column in THIS batch reads 0 here, and a column's cells outside the stretches that list it say "no ramp".
#ifdef __HIPCC__
static inline __host__ __device__ bool a2d_cut_coeff(const A2DParams &p, int f, int ui, int *f1)
{
	if(p.ncut <= 0)		// (set with cutf)
		return false;
#if defined(__HIP_DEVICE_COMPILE__)
	// Through the CONSTANT address space (as a2amd_fast.hip's rec_issue): where the unit is the same in every lane these
	// are scalar loads, which take no vector registers from the kernels that ask - the parameter block is the host's, the
	// table and the columns are written by the sweep pass alone, before any kernel that reads them starts.
	// (... and behind the asm: the table's pointers are read here, where a batch has sweeps, instead of riding through
	// the callers' loops over fragments and voices in registers batch after batch)
	typedef const __attribute__((address_space(4))) A2DParams *CP;
	typedef const __attribute__((address_space(4))) int32_t *CI;
	uintptr_t qa = (uintptr_t)&p;
	asm volatile("" : "+s"(qa));
	const CP q = (CP)qa;
	const int ncut = q->ncut;
	const int k = *((CI)(uintptr_t)q->cslot + ui);
	if(k <= 0 || k > ncut)
		return false;
	const int v = *((CI)(uintptr_t)q->cutf + ((size_t)f * (size_t)ncut + (size_t)(k - 1)));
#else
	const int k = p.cslot[ui];
	if(k <= 0 || k > p.ncut)
		return false;
	const int v = p.cutf[(size_t)f * (size_t)p.ncut + (size_t)(k - 1)];
#endif
	if(v < 0)
		return false;
	*f1 = v;
	return true;
}
#endif

// a2amd_cutsweep.hip: the sweep pass.  One sweeping filter12 of a stretch of repeated fragments: its cutoff ramper
// {value, target, delta, timer} as the stretch finds it, its unit, its column of the batch's sweep table.
struct A2DCutSweep { int32_t ramper[4]; int32_t unit, slot, pad[2]; };
// k_cut_sweep: cutf[(f0 + j) * stride + list[k].slot] = the pitch argument of the coefficient behind window j of the
// stretch (count fragments of 'frames' frames each), or the marker; cslot[list[k].unit] = slot + 1.  cutf holds 'words'
// words, cslot nunits entries: an entry that would land outside is dropped.
int a2d_launch_cut_sweep(const A2DCutSweep *list, int n, int f0, int count, unsigned frames, int32_t *cutf, int stride,
		size_t words, int32_t *cslot, int nunits, void *stream);
// k_cut_resolve, once per batch behind every stretch's k_cut_sweep: pitch arguments -> coefficients (f1tab: [32][65536])
int a2d_launch_cut_resolve(int32_t *cutf, size_t words, const int32_t *f1tab, void *stream);

// a2amd_noise.hip: the seed pass.  One settled noise oscillator of a stretch of device-seeded fragments, in walk order:
// phase and increment as the stretch finds them, its unit, its column of the batch's seed table.
struct A2DNoiseOsc { uint32_t ph_lo, ph_hi, dphase; int32_t unit, slot, pad[3]; };
// seed[(f0 + j) * stride + osc[k].slot] = 'start' advanced by the draws of all n oscillators over fragments [0, j) of the
// stretch and of oscillators < k in fragment j (count fragments of 'frames' frames each); nslot[osc[k].unit] = slot + 1.
// seed holds seed_words words, nslot nunits entries: an entry that would land outside is dropped.
int a2d_launch_noise_seeds(const A2DNoiseOsc *osc, int n, uint32_t start, int f0, int count, unsigned frames,
		uint32_t *seed, int stride, size_t seed_words, int32_t *nslot, int nunits, void *stream);

// a2amd_noisepan.hip: k_leaf_noisepan, the quiet kernel of settled wtosc (noise) -> panmix voices in a batch with device-seeded
// fragments (hp.nseed set): the voices of the list without records this batch, 'vpw' (at most 64) of them per wavefront
int a2d_launch_leaf_noisepan(const A2DParams *dparams, const A2DParams &hp, const int *dlist, int nlist, int vpw, void *stream);
// a2amd_noisefiltpan.hip: k_leaf_noisefiltpan, the same for settled wtosc (noise) -> filter12 -> panmix voices: a workgroup per
// 'vpg' (at most 64) voices of the list, its filter wavefront lane = voice
int a2d_launch_leaf_noisefiltpan(const A2DParams *dparams, const A2DParams &hp, const int *dlist, int nlist, int vpg, void *stream);
// a2amd_oscbare.hip: k_leaf_oscbare, the quiet kernel of bare wtosc voices (one unit, wired, adding into channel 0 of the
// output bus): the voices of the list without records this batch, gliding or not, 'vpw' (at most 64) of them per wavefront
int a2d_launch_leaf_oscbare(const A2DParams *dparams, const A2DParams &hp, const int *dlist, int nlist, int vpw, void *stream);
// a2amd_osc3filtpan.hip: k_leaf_osc3filtpan, the quiet kernel of 3 x wtosc -> filter12 -> panmix voices: the voices of the list
// without a run this batch, gliding or not; a workgroup per 'vpg' (at most 64) voices, its filter wavefront lane = voice
int a2d_launch_leaf_osc3filtpan(const A2DParams *dparams, const A2DParams &hp, const int *dlist, int nlist, int vpg, void *stream);
// ... and k_leaf_osc3filtpan_win, its windows launch: the voices of the list WITH a run - windows only and a tiling, the host
// has checked both (seg_rows) - every ramper stepped window by window; the same workgroup
int a2d_launch_leaf_osc3filtpan_win(const A2DParams *dparams, const A2DParams &hp, const int *dlist, int nlist, int vpg, void *stream);

// a2amd_vm.hip: the count pass (emit = 0) or the emit pass of the VM kernel
int a2d_launch_vm(const A2DVmParams &vp, int emit, void *stream);
// k_vm_pool: the window pool entries k_vm_win would take for the batch described by vp (vp.list: VM slots, any
// classes) - one per window that begins inside a fragment - added to *out
int a2d_launch_vm_pool(const A2DVmParams &vp, unsigned *out, void *stream);
#define A2D_WIN_STAGED 2	/* further windows of a fragment a control lane keeps in LDS (WIN_EXL, a2amd_winctl.h) */
// Where k_vm_win leaves the state it has stepped - the voices' VM state, their units' control words, which of them are
// the quiet kernels' this batch (runs[]), the fault count.  Normally the live arrays; a SPECULATIVE pass (round 6,
// vm_speculate: the next batch's VM + control work done behind this batch, while the engine thread walks) leaves it in
// shadow arrays of the same shape, and k_vm_commit moves it over when the batch turns out to be the one predicted.
struct A2DVmwOut {
	A2DVmVoice *vmv;	// [vm slot]
	int        *ustate;	// [unit][A2D_USTATE]
	int        *vactive;	// [voice slot]
	A2DRun     *runs;	// [voice slot]
	uint32_t   *total;	// [1] += voices that faulted
	uint32_t   *idle;	// += voices of the list the VM leaves alone this batch (the quiet kernels'), or null
};
// a speculative pass's results into the live state: the voices of window class (nosc, filt) in vp.list (vm slots)
int a2d_launch_vm_commit(const A2DVmParams &vp, const A2DParams &hp, int nosc, int filt, const A2DVmwOut &from, void *stream);
// k_vm_win (a2amd_vmwin.hip): the VM voices of one window class (vp.list: their VM slots in the order of the
// class's voice list, vp.n) run through fragments [fa, fb) and write the window entries themselves - no records.
// now_fa: engine time of fragment fa's first frame, batch_end: of the batch's end; runs[voice].count says
// afterwards whose the voice is this batch (0: the quiet kernels').  Returns -1 for a class without a kernel.
int a2d_launch_vm_win(const A2DVmParams &vp, const A2DParams &hp, int nosc, int filt, int fa, int fb, uint32_t now_fa,
		uint32_t batch_end, int *wslot, int *wext, int *wscr, unsigned *widx, unsigned *wtop, unsigned wcap, void *stream,
		const A2DVmwOut *out = nullptr);	// (out: null = the live arrays)
#define A2D_VMW_ROW (64 - 1 - 1)	/* entries of wscr per voice of the list (A2D_WIN_WORDS each): a fragment's windows beyond
				 * the first and the staged ones - one at least (WIN_EXLN, a2amd_winctl.h) */

// launchers implemented in a2amd_kernels.hip (stream = hipStream_t)
// dparams / dlist are device pointers; 'vpw' voices of the list per wavefront
int a2d_launch_voices(const A2DParams *dparams, const int *dlist, int nlist, int vpw, void *stream);
// hp = host copy of *dparams (device pointers passed as direct kernel arguments)
// ysplit > 1 cuts the batch into time slices rendered by different wavefronts
// (needs the staging copy 'ustage' of the unit state array)
// a state commit a time-sliced leaf kernel left to be done (ustage -> ustate for its
// voices): rides along with the next driver-chain launch instead of one of its own
// staged[e]: what the kernel staged for entry e of its list in this batch - nothing (the voice carried records), the
// oscillators' phases (a settled voice: nothing else moved), or every word (a voice with something still moving)
enum { A2D_STAGED_NONE = 0, A2D_STAGED_PHASES, A2D_STAGED_FULL };
struct A2DCommit { const int *list; int nlist, nosc; const int *ustage; const unsigned char *staged; };
struct A2DCommitSet { A2DCommit c[2]; int n; };
int a2d_launch_leaf_oscpan(const A2DParams *dparams, const A2DParams &hp, const int *dlist, int nlist,
		int vpw, int ysplit, int *ustage, unsigned char *staged, void *stream, void *event_after_main, A2DCommit *defer);
int a2d_launch_bus_driver(const A2DParams *dparams, const int *dlist, int nlist, int nfrags, int consume,
		const A2DCommitSet *commits, void *stream, int *master_host = nullptr, int ramping = 0);	// ramping: the launch of the drivers still gliding (one workgroup each); master_host: where the root stores the master bus (pinned host memory) instead of the bus memory
int a2d_launch_commit(const A2DParams &hp, const A2DCommit &cm, void *stream);
// quiet "inline; fbdelay 2->2 ... ; fbdelay 2->2 >" voices (one workgroup each)
int a2d_launch_bus_fbdchain(const A2DParams *dparams, const int *dlist, int nlist, int consume, void *stream);
// k_bus_fbdpan: the same rounds with a panmix 2->2, wired and adding, behind the last delay (none of them wired)
// (windows: the launch over the voices whose run is windows only - R_SEG records that tile their fragments, at most
// FBW_MAXWIN table rows a voice, the host has checked both - and is read; without it a voice with a run is skipped)
int a2d_launch_bus_fbdpan(const A2DParams *dparams, const int *dlist, int nlist, int consume, void *stream, int windows = 0);
int a2d_launch_park(int32_t *stage, int32_t *bus, unsigned words, void *stream);
int a2d_launch_add_bus(int32_t *dst, int32_t *src, unsigned words, void *stream);
// bus[f][ch][64] (nch channels per fragment) += inj[f][ch][64] (8 channels per fragment), ch < n
int a2d_launch_add_inject(const int32_t *inj, int32_t *bus, int nch, int n, int nfrags, void *stream);
// Hermite coefficient entries for wave pool samples [lo, hi) (reads pool[lo-1 .. hi+1])
int a2d_launch_build_coef(const int16_t *pool, int *coef, int *coef4, unsigned lo, unsigned hi, void *stream);	// (coef4: the 16 byte table, or null)
// a2amd_wavecap.hip
int a2d_launch_capture(const int32_t *bus, int32_t *dst, const uint32_t *fragpos, int nfrags, int nch, void *stream);
int a2d_launch_wave_from_pcm(const int32_t *pcm, int16_t *pool, const uint32_t *off, const uint32_t *size, int levels, int looped,
		int pre, int post, void *stream);
int a2d_launch_wave_level0(const int32_t *pcm, int16_t *d, unsigned size, void *stream);
int a2d_launch_wave_finish(int16_t *pool, const uint32_t *off, const uint32_t *size, int levels, int looped, int pre, int post,
		void *stream);
// a2amd_wavepost.hip: level 0 with A2_NORMALIZE / A2_XFADE; scratch: a2d_wavepost_scratch_words() device words
unsigned a2d_wavepost_scratch_words(unsigned size, unsigned flags, unsigned chunk);
int a2d_launch_wave_level0_post(const int32_t *pcm, int16_t *d, unsigned size, unsigned flags, unsigned chunk, uint32_t *scratch,
		void *stream);
int a2d_osc2filtpan_max_vpg(void);
int a2d_launch_leaf_osc2filtpan(const A2DParams *dparams, const A2DParams &hp, const int *dlist, int nlist,
		int vpg, void *stream);
int a2d_launch_leaf_oscfiltpan(const A2DParams *dparams, const A2DParams &hp, const int *dlist, int nlist,
		int vpw, void *stream);
// runs[idx[i]] = val[i] for the few voices whose record run changed this batch
int a2d_launch_scatter_runs(const int *didx, const A2DRun *dval, int n, A2DRun *druns, void *stream);
int a2d_launch_leaf_osc2pan(const A2DParams *dparams, const A2DParams &hp, const int *dlist, int nlist,
		int vpw, int ysplit, int *ustage, unsigned char *staged, void *stream, A2DCommit *defer, int voice_major, int lds_taps,
		int tame, unsigned long long *tame_count, int *ysplit_used, const unsigned char *taken = nullptr);
// a2amd_osc2tame.hip: launched in front of the launch above, with its vpw and ysplit; taken[wavefront of the list]: 1 this
// kernel rendered it, 0 it is the launch above's; taken_count: the 1s, summed over the launches
int a2d_launch_leaf_osc2tame(const A2DParams *dparams, const A2DParams &hp, const int *dlist, int nlist, int vpw, int ysplit,
		int *ustage, unsigned char *staged, void *stream, int lds_taps, unsigned long long *tame_count, unsigned char *taken,
		unsigned long long *taken_count);
// wtosc[+wtosc] [-> filter12] -> panmix voices that carry records this batch (nosc = 1 | 2, filt = 0 | 1)
// skip_empty: the list's voices get their records from the device VM (a2amd_vm.hip); those it left
// without any this batch are rendered by their class's quiet kernel
struct A2Switches;	// (a2amd_switches.h: the launchers' forced shapes)
int a2d_launch_leaf_recs(const A2Switches &sw, const A2DParams *dparams, const A2DParams &hp, int nosc, int filt, const int *dlist,
		int nlist, int vpw, void *stream, int skip_empty = 0);
// Round 5 (a2amd_win.hip): the same voices in two passes.  The control pass (lane = voice) walks the
// records of fragments [fa, fb) and leaves closed-form window entries: the first window of fragment f for
// list position i in its slot wslot[((f - fa) * nlist + i) * A2D_WIN_SLOTWORDS(nosc, filt)], further windows
// of that fragment in the pool wext (A2D_WIN_WORDS apart) from index widx[(f - fa) * nlist + i] on (pool
// indices from the counter wtop[0], at most wcap; wtop[1] != 0: the pool was too small); wrc[i]: where a
// voice's walk through its records stands between two slabs of a batch.  The render pass (lane = frame)
// evaluates them.
#define A2D_WIN_WORDS 24
#define A2D_WIN_SLOTWORDS(nosc, filt) ((filt) ? ((nosc) == 1 ? 20 : 24) : ((nosc) == 1 ? 12 : 20))
int a2d_launch_win_ctl(const A2DParams *dparams, const A2DParams &hp, int nosc, int filt, const int *dlist, int nlist,
		int skip_empty, int fa, int fb, int *wslot, int *wext, unsigned *widx, unsigned *wtop, unsigned wcap, int *wrc,
		void *stream);
int a2d_launch_win_render(const A2Switches &sw, const A2DParams &hp, int nosc, int filt, const int *dlist, int nlist, int fa, int fb,
		const int *wslot, const int *wext, const unsigned *widx, void *stream);
// ... all four kinds in one launch: lists[k] / counts[k] for (nosc, filt) = (1,0) (2,0) (1,1) (2,1)
// skip_mask bit k: list k may hold voices without records this batch - their quiet kernel renders those (skip_empty)
int a2d_launch_leaf_recs_all(const A2Switches &sw, const A2DParams *dparams, const A2DParams &hp, const int *const *lists, const int *counts,
		int vpw, void *stream, int skip_mask = 0);
// fm -> panmix leaf voices of ONE unit kind (a2amd_unitkind A2AMD_FM1..FM4R)
int a2d_launch_leaf_fmpan(const A2DParams *dparams, const A2DParams &hp, int kind, const int *dlist, int nlist,
		int vpw, void *stream);
// ... or of all eight kinds in one launch (small voice counts); the list is
// grouped by kind in a2amd_unitkind order, count8[k] voices each
int a2d_launch_leaf_fmpan_all(const A2DParams *dparams, const A2DParams &hp, const int *dlist,
		const int *count8, int vpw, void *stream);
