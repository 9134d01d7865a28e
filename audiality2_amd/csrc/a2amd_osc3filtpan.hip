// a2amd_osc3filtpan.hip - k_leaf_osc3filtpan: the quiet kernel of "wtosc (replacing) + wtosc (adding) + wtosc (adding) ->
// filter12 (1 ch) -> panmix 1->2, wired, adding" leaf voices - the three-oscillator subtractive lead,
// `struct { wtosc; wtosc o2; wtosc o3; filter12; panmix }` - in the batches in which they carry no record.
//
// Ownership and pipeline are k_leaf_noisefiltpan's (a2amd_noisefiltpan.hip), and what the two share word for word - the
// workgroup's constants, the split of its voices over the workers, the facts every wavefront derives alike, the bus sums,
// the bus-run walk, and the tap pair k_leaf_oscbare uses too - stands in a2amd_quiet.h.  A workgroup of 8 wavefronts owns
// up to 64 voices of its run of the bus-sorted list for the WHOLE batch and walks its fragments in order - no time slices,
// no staged commit.  Per fragment three stages meet over a ring of three [voices][64 + 1] LDS tiles, a barrier per step:
//   K/A(f)    workers.  Lane = voice, once per fragment: osc_window_v() (a2amd_winctl.h) steps each of the voice's three
//             oscillators over the window - pitch and amplitude rampers, mip level, the wrap of a looped wave, a one-shot
//             wave's end, a pitch out of range, an unloaded wave - and leaves the closed-form words of the window, as in
//             k_leaf_oscbare (a2amd_oscbare.hip).  Then lane = frame, voice by voice: the words out of the lanes, two
//             coefficient-table taps per oscillator that plays, the next voice's loads issued before this voice's
//             arithmetic; the replacing oscillator's value (0 where it is silent) and the two adders' in wtosc.c's wrapping
//             add; the row stored already shifted (x5 = sum >> 5, filter12.c:105: the shift is of the SUM)
//   B(f - 1)  wavefront 0, lane = voice: the q ramper prepared and run per fragment, filt_row (a2amd_filt.h) in place
//   C(f - 2)  workers.  Lane = voice: panmix_process12's head (panmix.c:84-95: the clamp flag in front of a2_PrepareRamper,
//             as ctl_window has it) on the voice's volume and pan rampers; lane = frame: the rows x the two gains - constant
//             where volume and pan rest, value + delta * frame otherwise (win_pan's arithmetic, a2amd_win.hip) - summed
//             over the voices of one output bus (the list is sorted by bus).  Where all the workgroup's voices mix into ONE
//             stereo bus the workers' sums meet in LDS and
//   D(f - 3)  the idle wavefront adds the workgroup's total to the bus in device memory: one atomic add per (fragment,
//             channel, frame) and workgroup.  A workgroup that spans several buses adds per worker and bus run instead.
// At the end every word the windows moved is stored with plain vector stores, as the general kernel or ctl_store would
// have left it: the three oscillators' (oscv_store) and the panmix's two rampers by the worker that carried them, the q
// ramper and FW_D1A / FW_D2A by wavefront 0 - a voice can change hands in either direction between any two batches.
//
// A gliding voice is this kernel's too (the host gives the class no stand-in record): every ramper is stepped here.
// A voice with a run this batch (runs[v].count != 0: records of its own, the stand-in of a sweeping cutoff or of a
// device-seeded noise oscillator) is the general kernel's and is skipped untouched, and so is a voice one of whose
// oscillators is neither on a mip-mapped wave nor off, or whose filter has a coefficient ramp pending (only records
// leave one): every wavefront of the workgroup reads the same words and comes to the same answer.
#include <hip/hip_runtime.h>
#include "a2amd_device.h"
#include "a2amd_dsp.h"
#include "a2amd_taps.h"
#include "a2amd_winctl.h"
#include "a2amd_filt.h"
#include "a2amd_quiet.h"

// ---- What k_leaf_osc3filtpan and k_leaf_osc3filtpan_win (the windows launch, below) share, each stated once.  A window
// is (a, m): m frames from frame a of the fragment; k_leaf_osc3filtpan's only window is the fragment, (0, n). ----

// Lane = voice: a voice of the workgroup as every wavefront reads it - its five units, its output bus, its filter's three
// gains, its run's bounds (with_run only) - and whether it is this launch's to render (ok): the ONE statement of the
// class's rule.  with_run: the launch of the voices that HAVE a run this batch (k_leaf_osc3filtpan_win), or of those that
// have none.  A voice that fails is left untouched: every word 0, no bus.
struct O3Voice { int uo0, uo1, uo2, uf, up, off, nch, lp, bp, hp, rfirst, rend; bool ok; };

DEV O3Voice o3_voice(bool with_run, bool listed, const int *list, int at, const A2DVoice *voices, const A2DRun *runs, const int *ustate)
{
	O3Voice V = { 0, 0, 0, 0, 0, -1, 2, 0, 0, 0, 0, 0, false };
	if(listed) {
		const int slot = list[at];
		const A2DRun run = runs[slot];
		if((run.count != 0) == with_run) {
			const A2DVoice &vc = voices[slot];
			V.uo0 = vc.unit[0]; V.uo1 = vc.unit[1]; V.uo2 = vc.unit[2];
			V.uf = vc.unit[3];
			V.up = vc.unit[4];
			V.off = vc.out_off;
			V.nch = vc.out_nch;
			const int m0 = ustate[(size_t)V.uo0 * A2D_USTATE + OW_MODE], m1 = ustate[(size_t)V.uo1 * A2D_USTATE + OW_MODE],
					m2 = ustate[(size_t)V.uo2 * A2D_USTATE + OW_MODE];
			const int *wf = ustate + (size_t)V.uf * A2D_USTATE;
			V.lp = wf[FW_LP]; V.bp = wf[FW_BP]; V.hp = wf[FW_HP];
			V.ok = vc.nunits == 5 && V.off >= 0 && V.nch >= 2 && !wf[FW_RAMP] &&
					(m0 == A2D_OSC_MIPWAVE || m0 == A2D_OSC_OFF) && (m1 == A2D_OSC_MIPWAVE || m1 == A2D_OSC_OFF) &&
					(m2 == A2D_OSC_MIPWAVE || m2 == A2D_OSC_OFF);
			if(with_run && V.ok) {
				V.rfirst = run.first;
				V.rend = run.first + run.count;
			}
		}
	}
	return V;
}

// The filter wavefront's state, lane = voice: the q ramper, f12_process's f and the two delays
struct O3Filt { Ramp q; int ff, d1, d2; };

DEV O3Filt o3_filt_load(const O3Voice &V, const int *ustate)
{
	O3Filt F = { { 0, 0, 0, 0 }, 0, 0, 0 };
	if(V.ok) {
		const int *wf = ustate + (size_t)V.uf * A2D_USTATE;
		F.q = ramp_load(wf + FW_Q);
		F.ff = wf[FW_F1] >> 12;		// f12_process's f, filter12.c:99 (no coefficient ramp: df = 0)
		F.d1 = wf[FW_D1A];
		F.d2 = wf[FW_D2A];
	}
	return F;
}

// state out: the filter's words as f12_process / ctl_store leave them
DEV void o3_filt_store(const O3Voice &V, int *ustate, const O3Filt &F)
{
	if(V.ok) {
		int *wf = ustate + (size_t)V.uf * A2D_USTATE;
		ramp_store(wf + FW_Q, F.q);
		wf[FW_D1A] = F.d1;
		wf[FW_D2A] = F.d2;
	}
}

// A worker's state, lane = voice, its own voices only (mylane): the three oscillators as ctl_load loads them, the
// panmix's rampers.  (Five objects, not one struct of them: as members of one the compiler pairs the oscillators' words
// differently, and the kernels come out 5 - 9 VGPRs larger - profiles/osc3_shared_stages.md.)
DEV void o3_work_load(OscV &o0, OscV &o1, OscV &o2, Ramp &vol, Ramp &pan, const O3Voice &V, const int *ustate, bool mylane)
{
	oscv_clear(o0);
	oscv_clear(o1);
	oscv_clear(o2);
	vol = pan = Ramp{ 0, 0, 0, 0 };
	if(mylane) {
		oscv_load(o0, ustate + (size_t)V.uo0 * A2D_USTATE);
		oscv_load(o1, ustate + (size_t)V.uo1 * A2D_USTATE);
		oscv_load(o2, ustate + (size_t)V.uo2 * A2D_USTATE);
		const int *wp = ustate + (size_t)V.up * A2D_USTATE;
		vol = ramp_load(wp + PW_VOL);
		pan = ramp_load(wp + PW_PAN);
	}
}

// state out: ctl_store's words of the oscillators and the panmix
DEV void o3_work_store(const O3Voice &V, int *ustate, const OscV &o0, const OscV &o1, const OscV &o2, const Ramp &vol, const Ramp &pan, bool mylane)
{
	if(mylane) {
		oscv_store(ustate + (size_t)V.uo0 * A2D_USTATE, o0);
		oscv_store(ustate + (size_t)V.uo1 * A2D_USTATE, o1);
		oscv_store(ustate + (size_t)V.uo2 * A2D_USTATE, o2);
		int *wp = ustate + (size_t)V.up * A2D_USTATE;
		ramp_store(wp + PW_VOL, vol);
		ramp_store(wp + PW_PAN, pan);
	}
}

// Stage C (the header comment), one pass: a window (a, m) of each voice of mk (lane = voice: has, a, m; mk: the voices
// that have one), summed into the buses of fragment f.  Lane = voice: panmix_process12's head for the window, the rampers
// stepped over it.  Lane = frame: the voices whose window holds this frame, at frame lane - a of it.  WIN: (a, m) are
// read out of the voices' lanes; else they are the same in every lane - the fragment, (0, n) - and cost no lane read.
template<bool WIN>
DEV void o3_pan_pass(const int *tile, const O3Voice &V, Ramp &vol, Ramp &pan, bool has, int a, int m, unsigned long long mk, bool lpraw,
		const QuietOut &out, int f, int lane)
{
	int pv = 0, pdv = 0, ppn = 0, pdp = 0, g0 = 0, g1 = 0;
	bool pcl = false;
	if(has) {
		// panmix.c:84-95: the clamp variant chosen in front of a2_PrepareRamper
		pcl = a2s_pan_over(pan.target) || a2s_pan_over(pan.value);
		ramp_prepare_v(vol, m);
		ramp_prepare_v(pan, m);
		pv = vol.value; pdv = vol.delta;
		ppn = pan.value; pdp = pan.delta;
		a2s_pan_gains(pv, ppn, pcl, &g0, &g1);	// (volume and pan at rest: the window's two gains)
		ramp_run(vol, m);
		ramp_run(pan, m);
	}
	const unsigned long long mramp = __ballot((pdv | pdp) != 0), mclamp = __ballot(pcl);
	BusRun run = busrun_begin();
	for(unsigned long long rest = mk; rest; rest &= rest - 1) {
		const int v = (int)__builtin_ctzll(rest);
		busrun_voice(run, out, f, V.off, V.nch, v);
		const int wk = lane - (WIN ? rdl(a, v) : a);
		const bool in = wk >= 0 && wk < (WIN ? rdl(m, v) : m);
		const int y = quiet_row(tile, v, lane, lpraw, V.lp);
		int v0 = rdl(g0, v), v1 = rdl(g1, v);
		if((mramp >> v) & 1ull) {
			// win_pan's arithmetic for a window in which volume or pan moves
			const int vk = wadd(rdl(pv, v), wmul(rdl(pdv, v), wk));
			const int pk = wadd(rdl(ppn, v), wmul(rdl(pdp, v), wk));
			const int vp = mul64s(pk, vk, 24);
			v0 = wsub(vk, vp);
			v1 = wadd(vk, vp);
			if((mclamp >> v) & 1ull) {
				const int lim = wshl(vk, 1);
				if(v0 > lim) v0 = lim;
				if(v1 > lim) v1 = lim;
			}
		}
		if(in) {
			run.acc0 = wadd(run.acc0, mul64s(y, v0, 24));
			run.acc1 = wadd(run.acc1, mul64s(y, v1, 24));
		}
	}
	busrun_end(run, out, f);
}

__global__ __launch_bounds__(64 * QUIET_WAVES)
void k_leaf_osc3filtpan(const A2DParams *__restrict__ pp, const int *__restrict__ list, int nlist, int vpg,
		const A2DVoice *__restrict__ voices, const A2DRun *__restrict__ runs, int *ustate,
		const A2DWave *__restrict__ waves, const uint32_t *__restrict__ ptab, const int *__restrict__ wavecoef,
		int nfrags, int *__restrict__ busmem)
{
	extern __shared__ __attribute__((aligned(16))) int o3_tiles[];	// 3 x [vpg][QUIET_PITCH]
	// the pitch table: read in every window of a gliding voice, from LDS (as k_win_ctl)
	__shared__ PTab s_ptab;
	// the workgroup's share of its bus, fragment by fragment, where it has one bus (stage D)
	__shared__ QuietBus o3_acc;
	for(int k = (int)threadIdx.x; k < 128; k += 64 * QUIET_WAVES)
		s_ptab[k] = ptab[k];
	quiet_bus_clear(o3_acc, (int)threadIdx.x, 64 * QUIET_WAVES);
	__syncthreads();
	const int wv = rfl((int)(threadIdx.x >> 6));
	const int lane = threadIdx.x & 63;
	const int first = (int)blockIdx.x * vpg;
	const int nv = min(vpg, nlist - first);
	if(nv <= 0)
		return;		// (the whole workgroup: the grid has none such)
	const int tsize = vpg * QUIET_PITCH;

	// lane v: voice v of this workgroup, in every wavefront
	const O3Voice V = o3_voice(false, lane < nv, list, first + lane, voices, runs, ustate);
	const QuietWg wg = quiet_wg(V.ok, V.bp, V.hp, V.off, V.nch);
	if(!wg.todo)
		return;		// (the whole workgroup)
	const bool lpraw = wg.lpraw, wgbus = wg.wgbus;
	const int nsteps = nfrags + 3;

	if(wv == 0) {
		// ================= the filter wavefront: lane = voice =================
		O3Filt F = o3_filt_load(V, ustate);
		__builtin_amdgcn_s_setprio(3);
		for(int st = 0; st < nsteps; ++st) {
			const int f = st - 1;
			if(f >= 0 && f < nfrags) {
				const int n = min((int)pp->fragframes[f], A2D_FRAG);
				if(n > 0) {
					// f12_process's head, filter12.c:86-96
					if(V.ok)
						ramp_prepare_v(F.q, n);
					const bool qrest = __all(!V.ok || F.q.delta == 0);
					if(V.ok) {
						int *row = o3_tiles + (f % 3) * tsize + lane * QUIET_PITCH;
						int qv = F.q.value;
						filt_row_pick(lpraw, qrest, row, n, F.ff, V.lp, V.bp, V.hp, F.d1, F.d2, qv, F.q.delta);
						ramp_run(F.q, n);
					}
				}
			}
			filt_barrier();
		}
		o3_filt_store(V, ustate, F);
		return;
	}

	// ================= workers: a range of the workgroup's voices each =================
	const unsigned long long mine = quiet_worker_voices(wv, nv, wg.todo);	// (wavefront 4: none)
	const bool mylane = (mine >> lane) & 1ull;
	OscV o0, o1, o2;
	Ramp vol, pan;
	o3_work_load(o0, o1, o2, vol, pan, V, ustate, mylane);
	const CoefRsrc rs = coef_rsrc(wavecoef);

	const QuietOut out = { busmem, &o3_acc, wgbus, lane };

	for(int st = 0; st < nsteps; ++st) {
		// ---- D(st - 3): the workgroup's sum of a fragment, complete since the last barrier ----
		if(wv == 4 && wgbus && st >= 3) {
			const int f = st - 3;
			if((int)pp->fragframes[f] > 0)
				quiet_bus_flush(o3_acc, busmem, wg.wg_off, f, lane);
		}
		// ---- K/A(st) ----
		if(st < nfrags && mine) {
			const int f = st;
			const int n = min((int)pp->fragframes[f], A2D_FRAG);
			if(n > 0) {
				// control, lane = voice: the window's words of each oscillator and what its frames are made of
				int w0[6] = { 0, 0, 0, 0, 0, 0 }, w1[6] = { 0, 0, 0, 0, 0, 0 }, w2[6] = { 0, 0, 0, 0, 0, 0 };
				int md0 = WM_SILENT, md1 = WM_SILENT, md2 = WM_SILENT;
				if(mylane) {
					md0 = osc_window_v(waves, s_ptab, o0, n, w0);
					md1 = osc_window_v(waves, s_ptab, o1, n, w1);
					md2 = osc_window_v(waves, s_ptab, o2, n, w2);
				}
				const unsigned long long t0 = __ballot(md0 == WM_TAPS), t1 = __ballot(md1 == WM_TAPS), t2 = __ballot(md2 == WM_TAPS);
				// render, lane = frame.  (lanes beyond the fragment's frames: the last frame's address, stored as 0)
				int *tile = o3_tiles + (f % 3) * tsize;
				const unsigned fl = (unsigned)min(lane, n - 1);
				const bool in = lane < n;
				auto issue = [&](int v, OscTaps &A, OscTaps &B, OscTaps &C) __attribute__((always_inline)) {
					if((t0 >> v) & 1ull) osctaps_issue(w0, v, rs, fl, A); else osctaps_clear(A);
					if((t1 >> v) & 1ull) osctaps_issue(w1, v, rs, fl, B); else osctaps_clear(B);
					if((t2 >> v) & 1ull) osctaps_issue(w2, v, rs, fl, C); else osctaps_clear(C);
				};
				unsigned long long m = mine;
				int k = (int)__builtin_ctzll(m);
				m &= m - 1;
				OscTaps A0, B0, C0;
				issue(k, A0, B0, C0);
				for(;;) {
					const int kn = m ? (int)__builtin_ctzll(m) : -1;
					OscTaps A1, B1, C1;
					if(kn >= 0)
						issue(kn, A1, B1, C1);
					// wtosc_do_fragment replacing, then twice adding (A2_PROCADD: wrapping)
					const int x = wadd(wadd(osctaps_finish(A0, fl), osctaps_finish(B0, fl)), osctaps_finish(C0, fl));
					tile[k * QUIET_PITCH + lane] = in ? x >> 5 : 0;
					if(kn < 0)
						break;
					m &= m - 1;
					k = kn;
					A0 = A1; B0 = B1; C0 = C1;
				}
			}
		}
		// ---- C(st - 2): one pass, every voice's window the fragment ----
		if(st >= 2 && st - 2 < nfrags && mine) {
			const int f = st - 2;
			const int n = min((int)pp->fragframes[f], A2D_FRAG);
			if(n > 0)
				o3_pan_pass<false>(o3_tiles + (f % 3) * tsize, V, vol, pan, mylane, 0, n, mine, lpraw, out, f, lane);
		}
		filt_barrier();
	}
	o3_work_store(V, ustate, o0, o1, o2, vol, pan, mylane);
}

int a2d_launch_leaf_osc3filtpan(const A2DParams *dparams, const A2DParams &hp, const int *dlist, int nlist, int vpg, void *stream)
{
	return quiet_launch(k_leaf_osc3filtpan, dparams, dlist, nlist, vpg, stream, hp.voices, hp.runs, hp.ustate, hp.waves, hp.ptab,
			hp.wavecoef, hp.nfrags, hp.busmem);
}

// ---------------------------------------------------------------------------
// k_leaf_osc3filtpan_win: the windows launch.  The same voices in the batches in which their only records are R_SEG windows
// that tile the fragments (a parent's VM woke inside a fragment: include/a2amd_osc3win.h) - every ramper stepped window by
// window, as the reference's Process(offset, frames) calls would.  Workgroup, tiles and stages are k_leaf_osc3filtpan's,
// and so is every piece above; what differs:
//   The voices.  Those of its list that HAVE a run (runs[slot].count != 0): the host lists a voice here only where
//             seg_rows() (a2amd_sched.cpp) has found the run windows only and a tiling, and on no other list.
//   The windows.  Read in place: lane = voice keeps a cursor into its run per stage, and a fragment's windows are a mask over
//             its frames - bit a: a window starts at frame a; it ends where the next one starts, or at the fragment's end (the
//             tiling).  A fragment without a record is the default window (0, n): bit 0.  No table, so no cap on the windows of
//             a voice.  Every wavefront reads the same words and comes to the same windows.
//   K/A(f)    over the window index k, up to the most windows a voice of the wavefront has in the fragment (wave-uniform: a
//             ballot): lane = voice, osc_window_v() on the three oscillators of the voices that have a k-th window (a, m);
//             lane = frame, for each such voice lanes a <= lane < a + m render frame lane - a of that window's words.  The
//             row ends up holding the whole fragment; lanes beyond n hold 0.
//   B(f - 1)  the q ramper prepared and run once per window.  Lanes have different windows: the wavefront walks the segments
//             between the union of its voices' cut frames, filt_row over each (d1 / d2 and the running q carry across), and a
//             lane re-prepares q where one of its own windows starts.  Where every voice's q is at rest - timer == 0 - the
//             fragment is filtered whole, as in k_leaf_osc3filtpan: a2_PrepareRamper without a timer (a2_dsp.h:130-134) sets
//             value = target and delta = 0 whatever 'frames' is and leaves the timer 0, and a2_RunRamper (:152-155) then adds
//             0 - the same q in every frame and the same words left, however the fragment is cut.
//   C(f - 2)  over k likewise, an o3_pan_pass() each: the head per window, the clamp flag chosen per window in front of the
//             prepare (as k_bus_fbdpan_win does).  A pass has bus runs of its own (the sums are wrapping adds: their order
//             is free).
// D and the state stores are k_leaf_osc3filtpan's: either kernel of the class, or k_voices, takes the voice up next batch.
// A listed voice that failed 'ok' - o3_voice(), the rule both launches share - would be rendered by nobody, so the host
// must list none.  What excludes each case there (upload(), a2amd_sched.cpp):
//   - five units, a bus of two channels or more: only voices classified CLS_OSC3FILTPAN (is_osc3filtpan_chain(), the classes
//     fresh where the list is made) are listed;
//   - an oscillator neither on a mip-mapped wave nor off: noise is not of the class, a 'w' write to noise is a record (the run
//     is then not windows only) and afterwards every window carries its R_NOISESEED record or, in a device-seeded stretch,
//     the voice is marked (noise_run) and not listed; any other wave kind played in the batch sets mode_mix: not listed;
//   - a coefficient ramp pending: a filter12 cutoff ramp leaves R_F1SET / R_F1RAMP records in every window it spans - such a
//     run is not windows only - the filter step that ends a ramp clears the flag, and a voice with a filter in the batch's
//     sweep table is marked (cut_run) and not listed.
// ---------------------------------------------------------------------------

// One fragment's windows of a voice, lane = voice: the records of fragment f at the run's cursor (cur .. end) as a mask of
// the frames at which a window starts, below n; bit 0 is always set (a fragment without a record: the default window).
// The cursor passes every record up to fragment f: it never stalls, whatever the run holds.
DEV unsigned long long o3w_cuts(const A2DRec *__restrict__ recs, int &cur, int end, int f, int n)
{
	unsigned long long m = 1ull;
	while(cur < end) {
		const unsigned head = recs[cur].head;
		if((int)A2D_RFRAG(head) > f)
			break;
		if((int)A2D_RFRAG(head) == f)
			m |= 1ull << (recs[cur].dur & 63u);
		++cur;
	}
	return n >= 64 ? m : m & ((1ull << n) - 1ull);
}

// the next window of a mask of window starts (not empty): its first frame, and - taken off the mask - its frames
DEV void o3w_next(unsigned long long &rem, int n, int &a, int &m)
{
	a = (int)__builtin_ctzll(rem);
	rem &= rem - 1;
	m = (rem ? (int)__builtin_ctzll(rem) : n) - a;
}

__global__ __launch_bounds__(64 * QUIET_WAVES)
void k_leaf_osc3filtpan_win(const A2DParams *__restrict__ pp, const int *__restrict__ list, int nlist, int vpg,
		const A2DVoice *__restrict__ voices, const A2DRun *__restrict__ runs, const A2DRec *__restrict__ recs, int *ustate,
		const A2DWave *__restrict__ waves, const uint32_t *__restrict__ ptab, const int *__restrict__ wavecoef,
		int nfrags, int *__restrict__ busmem)
{
	extern __shared__ __attribute__((aligned(16))) int o3_tiles[];	// 3 x [vpg][QUIET_PITCH]
	__shared__ PTab s_ptab;
	__shared__ QuietBus o3_acc;
	for(int k = (int)threadIdx.x; k < 128; k += 64 * QUIET_WAVES)
		s_ptab[k] = ptab[k];
	quiet_bus_clear(o3_acc, (int)threadIdx.x, 64 * QUIET_WAVES);
	__syncthreads();
	const int wv = rfl((int)(threadIdx.x >> 6));
	const int lane = threadIdx.x & 63;
	const int first = (int)blockIdx.x * vpg;
	const int nv = min(vpg, nlist - first);
	if(nv <= 0)
		return;		// (the whole workgroup: the grid has none such)
	const int tsize = vpg * QUIET_PITCH;

	// lane v: voice v of this workgroup, in every wavefront
	const O3Voice V = o3_voice(true, lane < nv, list, first + lane, voices, runs, ustate);
	const QuietWg wg = quiet_wg(V.ok, V.bp, V.hp, V.off, V.nch);
	if(!wg.todo)
		return;		// (the whole workgroup)
	const bool lpraw = wg.lpraw, wgbus = wg.wgbus;
	const int nsteps = nfrags + 3;

	if(wv == 0) {
		// ================= the filter wavefront: lane = voice =================
		O3Filt F = o3_filt_load(V, ustate);
		int cur = V.rfirst;
		__builtin_amdgcn_s_setprio(3);
		for(int st = 0; st < nsteps; ++st) {
			const int f = st - 1;
			if(f >= 0 && f < nfrags) {
				const int n = min((int)pp->fragframes[f], A2D_FRAG);
				const unsigned long long cuts = o3w_cuts(recs, cur, V.rend, f, n);
				if(n > 0) {
					const unsigned long long mycuts = V.ok ? cuts : 0ull;
					// (q at rest in the whole wavefront: a window changes nothing - the header comment - and the fragment is one
					// segment, one window)
					const bool allrest = __all(!V.ok || F.q.timer == 0);
					unsigned long long u = 1ull;	// the union of the voices' window starts
					if(!allrest)
						for(;;) {
							const unsigned long long more = __ballot((mycuts & ~u) != 0);
							if(!more)
								break;
							const int v = (int)__builtin_ctzll(more);
							u |= (unsigned long long)(unsigned)rdl((int)(unsigned)mycuts, v) |
									((unsigned long long)(unsigned)rdl((int)(unsigned)(mycuts >> 32), v) << 32);
						}
					int *row = o3_tiles + (f % 3) * tsize + lane * QUIET_PITCH;
					int qv = F.q.value, qd = 0;
					while(u) {
						int s0, len;
						o3w_next(u, n, s0, len);
						// f12_process's head, filter12.c:86-96, where a window of this voice starts
						if(V.ok && (allrest || ((mycuts >> s0) & 1ull))) {
							unsigned long long own = allrest ? 1ull : mycuts >> s0;
							int a, m;
							o3w_next(own, n - s0, a, m);
							ramp_prepare_v(F.q, m);
							qv = F.q.value;
							qd = F.q.delta;
							ramp_run(F.q, m);
						}
						const bool qrest = __all(!V.ok || qd == 0);
						if(V.ok)
							filt_row_pick(lpraw, qrest, row + s0, len, F.ff, V.lp, V.bp, V.hp, F.d1, F.d2, qv, qd);
					}
				}
			}
			filt_barrier();
		}
		o3_filt_store(V, ustate, F);
		return;
	}

	// ================= workers: a range of the workgroup's voices each =================
	const unsigned long long mine = quiet_worker_voices(wv, nv, wg.todo);	// (wavefront 4: none)
	const bool mylane = (mine >> lane) & 1ull;
	OscV o0, o1, o2;
	Ramp vol, pan;
	o3_work_load(o0, o1, o2, vol, pan, V, ustate, mylane);
	const CoefRsrc rs = coef_rsrc(wavecoef);
	int curA = V.rfirst, curC = V.rfirst;	// the run's cursor of either stage

	const QuietOut out = { busmem, &o3_acc, wgbus, lane };

	for(int st = 0; st < nsteps; ++st) {
		// ---- D(st - 3): the workgroup's sum of a fragment, complete since the last barrier ----
		if(wv == 4 && wgbus && st >= 3) {
			const int f = st - 3;
			if((int)pp->fragframes[f] > 0)
				quiet_bus_flush(o3_acc, busmem, wg.wg_off, f, lane);
		}
		// ---- K/A(st) ----
		if(st < nfrags && mine) {
			const int f = st;
			const int n = min((int)pp->fragframes[f], A2D_FRAG);
			const unsigned long long cuts = o3w_cuts(recs, curA, V.rend, f, n);
			if(n > 0) {
				unsigned long long rem = mylane ? cuts : 0ull;
				int *tile = o3_tiles + (f % 3) * tsize;
				for(int k = 0;; ++k) {
					// control, lane = voice: the k-th window of the voices that have one - its words of each oscillator
					int w0[6] = { 0, 0, 0, 0, 0, 0 }, w1[6] = { 0, 0, 0, 0, 0, 0 }, w2[6] = { 0, 0, 0, 0, 0, 0 };
					int md0 = WM_SILENT, md1 = WM_SILENT, md2 = WM_SILENT, a_l = 0, m_l = 1;
					const bool has = rem != 0;
					if(has) {
						o3w_next(rem, n, a_l, m_l);
						md0 = osc_window_v(waves, s_ptab, o0, m_l, w0);
						md1 = osc_window_v(waves, s_ptab, o1, m_l, w1);
						md2 = osc_window_v(waves, s_ptab, o2, m_l, w2);
					}
					unsigned long long m = __ballot(has);
					if(!m)
						break;
					const unsigned long long t0 = __ballot(md0 == WM_TAPS), t1 = __ballot(md1 == WM_TAPS), t2 = __ballot(md2 == WM_TAPS);
					// render, lane = frame: frame lane - a of the window (lanes outside it: its nearest frame's address, not stored)
					auto issue = [&](int v, OscTaps &A, OscTaps &B, OscTaps &C, unsigned &fl, bool &in) __attribute__((always_inline)) {
						const int a = rdl(a_l, v), mm = rdl(m_l, v);
						fl = (unsigned)min(max(lane - a, 0), mm - 1);
						in = lane >= a && lane < a + mm;
						if((t0 >> v) & 1ull) osctaps_issue(w0, v, rs, fl, A); else osctaps_clear(A);
						if((t1 >> v) & 1ull) osctaps_issue(w1, v, rs, fl, B); else osctaps_clear(B);
						if((t2 >> v) & 1ull) osctaps_issue(w2, v, rs, fl, C); else osctaps_clear(C);
					};
					// (the fragment's first pass: every voice has a window, and the lanes beyond the fragment store their 0)
					const bool beyond = k == 0 && lane >= n;
					int v = (int)__builtin_ctzll(m);
					m &= m - 1;
					OscTaps A0, B0, C0;
					unsigned fl0;
					bool in0;
					issue(v, A0, B0, C0, fl0, in0);
					for(;;) {
						const int vn = m ? (int)__builtin_ctzll(m) : -1;
						OscTaps A1, B1, C1;
						unsigned fl1 = 0;
						bool in1 = false;
						if(vn >= 0)
							issue(vn, A1, B1, C1, fl1, in1);
						// wtosc_do_fragment replacing, then twice adding (A2_PROCADD: wrapping)
						const int x = wadd(wadd(osctaps_finish(A0, fl0), osctaps_finish(B0, fl0)), osctaps_finish(C0, fl0));
						if(in0 || beyond)
							tile[v * QUIET_PITCH + lane] = in0 ? x >> 5 : 0;
						if(vn < 0)
							break;
						m &= m - 1;
						v = vn;
						A0 = A1; B0 = B1; C0 = C1;
						fl0 = fl1; in0 = in1;
					}
				}
			}
		}
		// ---- C(st - 2): a pass per window index (bus runs of its own: the sums are wrapping adds, their order is free) ----
		if(st >= 2 && st - 2 < nfrags && mine) {
			const int f = st - 2;
			const int n = min((int)pp->fragframes[f], A2D_FRAG);
			const unsigned long long cuts = o3w_cuts(recs, curC, V.rend, f, n);
			if(n > 0) {
				unsigned long long rem = mylane ? cuts : 0ull;
				for(;;) {
					int a_l = 0, m_l = 0;
					const bool has = rem != 0;
					const unsigned long long mk = __ballot(has);
					if(!mk)
						break;
					if(has)
						o3w_next(rem, n, a_l, m_l);
					o3_pan_pass<true>(o3_tiles + (f % 3) * tsize, V, vol, pan, has, a_l, m_l, mk, lpraw, out, f, lane);
				}
			}
		}
		filt_barrier();
	}
	o3_work_store(V, ustate, o0, o1, o2, vol, pan, mylane);
}

// the windows launch: the same shape
int a2d_launch_leaf_osc3filtpan_win(const A2DParams *dparams, const A2DParams &hp, const int *dlist, int nlist, int vpg, void *stream)
{
	return quiet_launch(k_leaf_osc3filtpan_win, dparams, dlist, nlist, vpg, stream, hp.voices, hp.runs, hp.recs, hp.ustate, hp.waves,
			hp.ptab, hp.wavecoef, hp.nfrags, hp.busmem);
}
