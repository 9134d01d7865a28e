// a2amd_taps.h - what the lane = frame kernels share: wave-uniform <-> per-lane moves, the two
// Hermite tap forms (four fetched samples / a precomputed coefficient entry), the coefficient
// table's buffer descriptor, exact small divisions, the chunk's bus sums.
// (a2amd_fast.hip: the quiet kernels and k_leaf_recs; a2amd_win.hip: the window kernels)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "a2amd_device.h"
#include "a2amd_dsp.h"
#include "a2amd_fm.h"
#include "a2amd_settled.h"

#define FAST_WPB   4		// wavefronts per workgroup
#define FAST_FCH   A2D_FAST_FCH	// fragments whose bus sums stay in registers at a time

// park a wave-uniform value back in lane 'sel' of a per-lane register
#define WRL(reg, val) reg = me ? (val) : reg

// One Horner step of a2_Hermite (a2_dsp.h:64-74): (v * x wrapped to 32 bits) >> 15 with x = frac << 7,
// frac = the low byte of the 24:8 phase ph.  With p = v * frac exact, the low 32 bits of p << 7 are
// p's bits 0..24 moved up, so the reference's result is bits 8..24 of p, sign extended: one
// full-rate 24 bit multiply and one bit-field extract.  The multiply selects frac out of ph itself
// (SDWA: byte 0 of the second source, zero extended), so neither x nor frac is ever formed.
// Holds for |v| < 2^23: the multiplier takes v's low 24 bits, sign extended, and |p| < 2^31 then.
// Every operand the callers have is inside that: samples are int16, so a2_Hermite's |c| <= 32767,
// |a| <= (3 * 65535 + 65535) / 2 = 131070, |b| <= 65535 + 32767 + 131070 = 229372, a step's result
// is a 17 bit field (below 2^16 in magnitude), and the sums fed to the next step stay below
// 2^16 + 229372 < 2^19.  (Spelled as instructions: left to itself the compiler proves the 24 bit
// range for one of the three products only, and spells the byte select as a mask of its own.)
DEV int hermite_step(int v, unsigned ph)
{
	int p;
	asm("v_mul_i32_i24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0"
			: "=v"(p) : "v"(v), "v"(ph));
	return __builtin_amdgcn_sbfe(p, 8, 17);
}

// a2_Hermite on four already fetched samples, at the 24:8 phase ph (its low byte counts)
DEV int hermite4(int dm, int d0, int d1, int d2, unsigned ph)
{
	int c = (d1 - dm) >> 1;
	int a = (3 * (d0 - d1) + d2 - dm) >> 1;
	int b = dm - d0 + c - a;
	a = hermite_step(a, ph);
	a = hermite_step(a + b, ph);
	return d0 + hermite_step(a + c, ph);
}

// Four consecutive int16 samples as two dwords from a 2-byte aligned address
// (gfx950 global loads take any byte alignment in the HSA configuration).
struct __attribute__((packed, aligned(2))) Quad16 { uint32_t lo, hi; };

// Both taps of wtosc_Inter (wtosc.c:28-33): window A = d[i-1 .. i+2] for the tap
// at ph, window B = d[i'-1 .. i'+2] for the tap at ph + (dph16 >> 1), i' being i
// or i + 1 (dph16 <= 512 << 8).  Each window is one 8 byte load.
DEV int inter_quads(const Quad16 qa, const Quad16 qb, unsigned ph, unsigned ph2)
{
	int h0 = hermite4((int16_t)(qa.lo & 0xffff), (int)qa.lo >> 16, (int16_t)(qa.hi & 0xffff), (int)qa.hi >> 16, ph);
	int h1 = hermite4((int16_t)(qb.lo & 0xffff), (int)qb.lo >> 16, (int16_t)(qb.hi & 0xffff), (int)qb.hi >> 16, ph2);
	return h0 + h1;
}

// wtosc_Inter at 24:8 phase ph from wave data d (first payload sample)
DEV int inter_dwords(const int16_t *d, unsigned ph, unsigned dph16)
{
	const unsigned ph2 = ph + (dph16 >> 1);
	const Quad16 qa = *(const Quad16 *)(d + (int)(ph >> 8) - 1);
	const Quad16 qb = *(const Quad16 *)(d + (int)(ph2 >> 8) - 1);
	return inter_quads(qa, qb, ph, ph2);
}

// Hermite coefficients of one window, precomputed per wave sample when the wave is
// uploaded (k_build_coef): a2_Hermite's a, b and - packed - c (high half) and d[i]
// (low half), one 12 byte entry per wave sample (A2D_COEF_WORDS words).  The settled paths fetch one entry per tap instead of four samples and go
// straight into the three multiply-shift-add steps, which are the reference's own
// (a2_dsp.h:64-74: x = frac << 7, 32 bit wrap-around products, arithmetic >> 15) - no
// unpacking of samples, no deriving a, b, c for every output frame.
// The table is read through ONE buffer descriptor (stride = entry, indexed): the entry index
// phase >> 8 goes to the load as it is and the hardware scales it - no address
// arithmetic in the vector unit; the level's first payload sample is the load's scalar
// byte offset.  (Round 2 added a byte offset
// (phase >> 8) * 12 to a scalar base: one more vector instruction per tap.)
typedef int Coef4 __attribute__((ext_vector_type(3)));		// a, b, c:d0 (the halves come apart inside the adds: SDWA)
#define A2D_COEF_LOAD "llvm.amdgcn.struct.buffer.load.v3i32"
typedef int CoefRsrc __attribute__((ext_vector_type(4)));
extern "C" __device__ Coef4 a2d_coef_load(CoefRsrc rsrc, int vindex, int voffset, int soffset, int aux)
		__asm(A2D_COEF_LOAD);

// the descriptor of the coefficient table (gfx9 buffer resource: base, stride in word 1
// bits 16-29, no swizzle, num_records unlimited, DATA_FORMAT 32)
DEV CoefRsrc coef_rsrc(const int *wavecoef)
{
	const uint64_t b = (uint64_t)wavecoef;
	CoefRsrc r;
	r.x = rfl((int)(unsigned)b);
	r.y = rfl((int)(((unsigned)(b >> 32) & 0xffffu) | ((4u * A2D_COEF_WORDS) << 16)));
	r.z = -1;
	r.w = 0x00020000;
	return r;
}

// byte offset of the entry of pool sample doff (the table follows the pool: host, a2amd_host.cpp)
DEV int coef_base(unsigned doff) { return (int)(doff * (4u * A2D_COEF_WORDS)); }

// a2_Hermite from a coefficient entry at the 24:8 phase ph, without its d[i] term: the three steps of
// hermite_step() (the table is built from int16 samples, so its a, b and c are inside the bounds
// stated there)
DEV int hermite_ct(const Coef4 k, unsigned ph)
{
	int t = hermite_step(k.x, ph);
	t = hermite_step(wadd(t, k.y), ph);
	return hermite_step(wadd(t, k.z >> 16), ph);
}

// Both taps of wtosc_Inter (wtosc.c:28-33) from their coefficient entries.  The two d[i] - the low
// halves of the entries' third words - meet in one add that sign-extends both (SDWA).  No gain of its
// own: it keeps what the compiler made of the per-tap wadd((int16_t)k.z, t) before hermite_step()
// (wrapping adds are associative, so the sum is the same); with the steps above in the way it
// extracts one of the halves by itself, one instruction more per pair of taps.  Both operands are
// vector registers: an entry held wave-uniform would cost a v_mov here.
DEV int inter_coefs(const Coef4 ka, unsigned pa, const Coef4 kb, unsigned pb)
{
	int d;
	asm("v_add_u32_sdwa %0, sext(%1), sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_0"
			: "=v"(d) : "v"(ka.z), "v"(kb.z));
	return wadd(wadd(d, hermite_ct(ka, pa)), hermite_ct(kb, pb));
}

// The same two taps in the form the filter kernels keep (k_leaf_oscfiltpan, k_leaf_osc2filtpan: both
// stand at their register limit, and with the steps above their all-settled loops spill 6 and 1
// registers more): x = frac << 7 formed once per tap - one SDWA shift of the phase's low byte - and the
// reference's own 32 bit wrap-around products and arithmetic >> 15.
DEV int frac_x(unsigned ph)
{
	int x;
	const int seven = 7;
	asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0"
			: "=v"(x) : "v"(seven), "v"(ph));
	return x;
}

DEV int hermite_cx(const Coef4 k, unsigned ph)
{
	const int x = frac_x(ph);
	int t = wmul(k.x, x) >> 15;
	t = wmul(wadd(t, k.y), x) >> 15;
	t = wmul(wadd(t, k.z >> 16), x) >> 15;
	return wadd((int)(int16_t)(k.z & 0xffff), t);
}

DEV int inter_coefs_x(const Coef4 ka, unsigned pa, const Coef4 kb, unsigned pb)
{
	return hermite_cx(ka, pa) + hermite_cx(kb, pb);
}

// wtosc_Inter (wtosc.c:28-33) from the coefficient table: cb = coef_base() of the
// level's first payload sample, ph = 24:8 phase of the tap
DEV Coef4 coef_at(const CoefRsrc rs, int cb, unsigned ph)
{
	return a2d_coef_load(rs, (int)(ph >> 8), 0, cb, 0);
}

// ... and from a wavefront's copy of a whole mip level in LDS (k_leaf_osc2pan's staged oscillators, a2d_osc2_stage): the
// level's size payload entries in the table's own layout, written by stage_level() below.  The level's size is
// 1 << lg and its pads are periodic, so entry i is entry i mod size for every i a tap can reach (a2amd_wavepads.h):
// the index is a bit field of the phase - one extract where the gather had none, and one multiply-add for the
// address - and the entry three dword reads at immediate offsets 0, 4, 8.  (Entries are 4-byte aligned: the pointer
// says so, and the three reads must not become one 12-byte read, which is only fast at 16-byte alignment.)
typedef __attribute__((address_space(3))) int LdsInt;
DEV Coef4 coef_lds(const LdsInt *level, unsigned ph, unsigned lg)
{
	const LdsInt *e = level + A2D_COEF_WORDS * __builtin_amdgcn_ubfe(ph, 8, lg);
	Coef4 k;
	k.x = e[0];
	k.y = e[1];
	k.z = e[2];
	return k;
}

// The copy: entries [0, size) of the level whose first payload entry stands at byte cb of the table, size <=
// A2D_OSC2_LDS_ENT, as coalesced dword loads (at most 6 a lane) and dword stores in the same linear layout.  Lanes
// read entries other lanes wrote: the caller fences on both sides (the compiler cannot see that dependency).
DEV void stage_level(LdsInt *level, const int *wavecoef, int cb, unsigned size, int lane)
{
	const int *src = wavecoef + ((unsigned)cb >> 2);
	const unsigned n = size * A2D_COEF_WORDS;
#pragma unroll
	for(int r = 0; r < A2D_OSC2_LDS_ENT * A2D_COEF_WORDS / 64; ++r) {
		const unsigned i = (unsigned)(r * 64 + lane);
		if(i < n)
			level[i] = src[i];
	}
}

// ---- tame levels: the fused steps (a2amd_wavetame.h) ----
// An entry of the second table: a, b << 8, c << 8, d0 << 8 of the window at a pool sample (k_build_coef), 16 bytes, read
// through a descriptor of its own with stride 16 - one buffer_load_dwordx4, indexed like the 12 byte entry.
typedef int Coef4x __attribute__((ext_vector_type(4)));
extern "C" __device__ Coef4x a2d_coef4_load(CoefRsrc rsrc, int vindex, int voffset, int soffset, int aux)
		__asm("llvm.amdgcn.struct.buffer.load.v4i32");

DEV CoefRsrc coef4_rsrc(const int *wavecoef4)
{
	const uint64_t b = (uint64_t)wavecoef4;
	CoefRsrc r;
	r.x = rfl((int)(unsigned)b);
	r.y = rfl((int)(((unsigned)(b >> 32) & 0xffffu) | (16u << 16)));
	r.z = -1;
	r.w = 0x00020000;
	return r;
}

DEV int coef4_base(unsigned doff) { return (int)(doff * 16u); }

DEV Coef4x coef4_at(const CoefRsrc rs, int cb, unsigned ph)
{
	return a2d_coef4_load(rs, (int)(ph >> 8), 0, cb, 0);
}

// a2_Hermite from such an entry at the 24:8 phase ph, its d[i] term included, on a level where no product wraps: per
// step one 24 bit multiply-add - the addend is the next coefficient, 8 bits up - and one arithmetic shift.  Exact there:
// the addend is a multiple of 256 and >> is a floor, so (v * f + (k << 8)) >> 8 = floor(v * f / 256) + k, and
// floor(v * f / 256) is the reference's (v * x) >> 15 while v * f stays inside [-2^24, 2^24).  Operands: |a| < 2^17,
// the steps' sums below 2^19 (hermite_step), f <= 255: inside the multiplier's 24 bits; |v * f + (k << 8)| < 2^27.
// (The 24 bit multiply is asked for by name and the compiler folds the add into it - v_mad_i32_i24; spelled as an
// instruction string it costs a wait state behind every one that feeds the shift.)
DEV int mad24(int v, int f, int k)
{
	return wadd(__mul24(v, f), k);
}

DEV int hermite_fused(const Coef4x k, unsigned ph)
{
	const int f = (int)(ph & 0xffu);
	int t = mad24(k.x, f, k.y) >> 8;
	t = mad24(t, f, k.z) >> 8;
	return mad24(t, f, k.w) >> 8;
}

// ... from a wavefront's copy of a whole level in LDS, in this table's layout (stage_level4): 1 << lg entries at a
// 16 byte stride, so the entry's byte offset is a shift and a mask of the phase - (ph >> 4) & ((size - 1) << 4) - and the
// entry one aligned 16 byte read.  mask16 = (size - 1) << 4, wave-uniform.
typedef __attribute__((address_space(3))) Coef4x LdsCoef4x;
DEV Coef4x coef4_lds(const LdsInt *level, unsigned ph, unsigned mask16)
{
	typedef __attribute__((address_space(3))) char LdsChar;
	return *(const LdsCoef4x *)((const LdsChar *)level + ((ph >> 4) & mask16));
}

// The copy: entries [0, size) of the level whose first payload entry stands at byte cb of the 16 byte table, size <=
// A2D_OSC2_LDS_ENT: an entry a lane, at most two rounds.  The caller fences on both sides, as for stage_level().
DEV void stage_level4(LdsInt *level, const int *wavecoef4, int cb, unsigned size, int lane)
{
	const Coef4x *src = (const Coef4x *)(wavecoef4 + ((unsigned)cb >> 2));
	LdsCoef4x *dst = (LdsCoef4x *)level;
#pragma unroll
	for(int r = 0; r < A2D_OSC2_LDS_ENT / 64; ++r) {
		const unsigned i = (unsigned)(r * 64 + lane);
		if(i < size)
			dst[i] = src[i];
	}
}

// what orders a wavefront's LDS stores against its other lanes' reads (LDS operations of one wavefront execute in
// order: nothing to wait for, the compiler must only keep them where they are)
DEV void lds_wave_fence()
{
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
}

// The 24:8 phase of a tap: (ph + lane * dph) >> 16 for a wave-uniform 64 bit phase ph and
// ldph = lane * dph (below 2^31: dph <= A2D_MAXPHINC << 16 on the settled paths).  Split at
// bit 16 the sum needs no 64 bit vector arithmetic: the halves of ph stay scalar, the lane
// part is two adds (a 64 bit multiply-add and a funnel shift otherwise).  lo + ldph is below
// 2^31 + 2^16, so the shifted value is the upper 16 bit word of that sum, and the compiler folds
// the shift into the second add (v_add_u32_sdwa, WORD_1 of the sum, hi from its scalar register):
// left in C, because spelled as instructions hi would need one register class for every caller
// (it is a scalar register wherever ph is wave-uniform, a vector register elsewhere).
DEV unsigned tap_phase(uint64_t ph, unsigned ldph)
{
	const unsigned lo = (unsigned)ph & 0xffffu, hi = (unsigned)(ph >> 16);
	return hi + ((lo + ldph) >> 16);
}

// lane * dph once per voice and oscillator (opaque to the compiler, which otherwise folds it
// back into a multiply-add per fragment)
DEV unsigned lane_dph(int lane, unsigned dph)
{
	unsigned t = (unsigned)lane * dph;
	asm("" : "+v"(t));
	return t;
}

// trunc(n / d) for |n| < 2^52, 0 < d < 2^31, exactly: the quotient of the correctly rounded double
// division is at most one off, and the remainder says which way (the compiler's 64 bit integer
// division is a few hundred instructions; a scripted voice needs one per ramping control and window)
DEV int64_t div_trunc_exact(int64_t n, int d)
{
	int64_t q = (int64_t)((double)n / (double)d);
	const int64_t r = n - q * d;
	if(n >= 0) {
		if(r < 0) --q; else if(r >= d) ++q;
	} else {
		if(r > 0) ++q; else if(r <= -(int64_t)d) --q;
	}
	return q;
}


// add the register sums of a chunk of fragments into the bus and clear them
template<int N>
DEV void flush_acc(int *busmem, int off, int nch, int f0, int nf, int lane, int dbg,
		int (&acc0)[N], int (&acc1)[N])
{
#pragma unroll
	for(int j = 0; j < N; ++j) {
		if(j < nf && off >= 0 && !(dbg & 1)) {
			int *dst = busmem + off + (size_t)(f0 + j) * nch * A2D_FRAG;
			if(acc0[j])
				atomicAdd(&dst[lane], acc0[j]);
			if(acc1[j])
				atomicAdd(&dst[A2D_FRAG + lane], acc1[j]);
		}
		acc0[j] = 0;
		acc1[j] = 0;
	}
}

// The same sums kept in LDS, [fragment][channel][lane] (k_leaf_osc2pan's voice-major walk: sums for more fragments
// than registers hold).  A lane adds into its own words only, so the adds are free of conflicts, need no order among
// the lanes, and their result is not used: ds_add_u32 at an immediate offset from the lane's word, off the vector ALU.
DEV void tile_add(int *w, int x)
{
	(void)__hip_atomic_fetch_add(w, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// ... and their flush_acc(): the first nf of the tile's nrows used rows go to the bus, all nrows are cleared
DEV void flush_tile(int *busmem, int off, int nch, int f0, int nf, int nrows, int lane, int dbg, int (*tile)[2][A2D_FRAG])
{
	for(int r = 0; r < nrows; ++r) {
		const int a0 = tile[r][0][lane], a1 = tile[r][1][lane];
		tile[r][0][lane] = 0;
		tile[r][1][lane] = 0;
		if(r < nf && off >= 0 && !(dbg & 1)) {
			int *dst = busmem + off + (size_t)(f0 + r) * nch * A2D_FRAG;
			if(a0)
				atomicAdd(&dst[lane], a0);
			if(a1)
				atomicAdd(&dst[A2D_FRAG + lane], a1);
		}
	}
}

// ---- the time-sliced settled kernels' prologue and epilogue (k_leaf_oscpan, k_leaf_osc2pan, k_leaf_osc2tame) ----
// The four words DV_MM .. DV_DOFF (k_leaf_osc2pan's OD_MM .. OD_DOFF) of an oscillator at a constant pitch on wave w:
// mip level, increment there, that level's size and place in the pool.  False: no wave for the settled paths - or
// 'settled' was false already, and then the descriptor's test words are not read (k_leaf_osc2pan's second oscillator).
// periodic: A2DWave::periodic's bit of that level (k_leaf_osc2pan: may the level be copied to LDS)
// tame: A2DWave::tame's bit of it (k_leaf_osc2pan: may the level's taps take the fused steps)
DEV bool settled_wave(const A2DWave *w, unsigned dphase, int *d, bool settled = true, unsigned *periodic = nullptr,
		unsigned *tame = nullptr)
{
	unsigned dph;
	const unsigned mm = a2s_mip(dphase, w->period, &dph);
	d[0] = (int)mm;
	d[1] = (int)dph;
	d[2] = (int)w->size[mm];
	d[3] = (int)w->off[mm];
	if(periodic)
		*periodic = (w->periodic >> mm) & 1u;
	if(tame)
		*tame = (w->tame >> mm) & 1u;
	return settled && a2s_wave_ok(w->size[0], w->flags, dph);
}

// What a time-sliced launch staged for the voice at one entry of its list, for the commit: every entry is
// written in every batch, by exactly one wavefront - the slice that walked the voice if it had something
// moving, the last slice otherwise.
DEV void stage_mark(unsigned char *m, bool mine, bool settled, bool last_slice, bool walker)
{
	if(mine && !settled) {
		if(walker)
			*m = A2D_STAGED_FULL;
	} else if(last_slice)
		*m = mine ? A2D_STAGED_PHASES : A2D_STAGED_NONE;
}
