// a2amd_sched.cpp - what a recorded batch becomes on the device: the records and lists that go
// up (upload), the launch order - leaf voices first, bus owners by nesting depth, deepest first -
// the launch shapes, hipGraphs of quiet batches, and the end of a batch.  (Split out of
// a2amd_host.cpp in round 3; the design notes are at the top of that file.)
#include "a2amd_host.h"
#include "a2amd_cutsweep.h"
#include <functional>

namespace a2h {




void touch(a2amd_ctx *c, int vi)
{
	HVoice &v = c->voices[vi];
	const long long serial = c->serial_base + rec_tag(c);
	if(v.touched != serial) {
		v.touched = serial;
		v.frag_mark = v.recs.size();
	}
}



// The windows of the open fragment that were left unrecorded so far - the voice's
// default window, noted in HVoice::default_seg or by the host in the default map -
// become records: something else follows in the same fragment after all.
void spell_out_pending(a2amd_ctx *c, int vi)
{
	HVoice &dv = c->voices[vi];
	const bool marked = c->frag_open && c->defmap_used && (size_t)vi < c->defmap.size() && c->defmap[vi];
	if(marked || (c->frag_open && is_held(c, vi))) {
		// (a held voice that gets a record after all - its chain taken down from outside the
		// walk, say - had its default window in this fragment like a marked one; the hold ends)
		if(marked)
			c->defmap[vi] = 0;
		unhold(c, vi);
		dv.default_seg = c->serial_base + c->cur_frag;
		if(dv.walked != c->serial_base + c->cur_frag) {
			dv.walked = c->serial_base + c->cur_frag;
			++c->walked_started;
		}
	}
	if(dv.default_seg == c->serial_base + rec_tag(c)) {
		dv.default_seg = -1;
		A2DRec seg = { A2D_HEAD(rec_tag(c), R_SEG, 0, 0), 0, (unsigned)c->fragframes[rec_tag(c)] << 16, 0 };
		if(!dv.listed_recs) {
			dv.listed_recs = true;
			c->with_recs.push_back(vi);
		}
		dv.recs.push_back(seg);
	}
}

void push_rec(a2amd_ctx *c, int vi, int op, int unit, int reg, int value, unsigned dur, unsigned start)
{
	touch(c, vi);
	spell_out_pending(c, vi);
	A2DRec r;
	r.head = A2D_HEAD(rec_tag(c), op, unit, reg);
	r.value = value;
	r.dur = dur;
	r.start = start;
	HVoice &v = c->voices[vi];
	if(!v.listed_recs) {
		v.listed_recs = true;
		c->with_recs.push_back(vi);
	}
	// A write that reaches a unit which has already rendered the window the
	// voice is in (a control wire from a unit further down the chain, e.g. the
	// engine's env, env.c:135) takes effect after that window: the device
	// executes a window as one SEG record, so the write waits behind it.
	if(op != R_SEG && op != R_INIT && op != R_KILL && unit < v.win_done) {
		v.deferred.push_back(r);
		return;
	}
	v.recs.push_back(r);
	if(op == R_SEG) {
		v.win_done = 0;
		for(A2DRec &d : v.deferred)
			v.recs.push_back(d);
		v.deferred.clear();
	}
}

int bus_alloc(a2amd_ctx *c, int nch)
{
	auto &fl = c->bus_free[nch];
	if(!fl.empty()) {
		int off = fl.back();
		fl.pop_back();
		return off;
	}
	size_t off = c->bus_used;
	c->bus_used += c->bus_stride_frames * (size_t)nch;
	return (int)off;
}

long long now_serial(const a2amd_ctx *c) { return c->serial_base + rec_tag(c); }

// the engine-visible walk found no work for the VMs: close the fragment
int close_fragment(a2amd_ctx *c)
{
	if(!c->frag_open)
		return 0;
	const int f = c->cur_frag;
	const unsigned nframes = c->fragframes[f];
	if(c->defmap_used) {
		size_t n = 0;
		const size_t nv = std::min(c->defmap.size(), c->voices.size());
		for(size_t k = 0; k < nv; ++k)
			n += c->defmap[k];
		c->walked_started += (int)n;
	}
	c->walked_started += (int)c->n_held;
	if(c->walked_started != c->n_started_live) {
		if(c->sw.hosttiming)
			dbg_counters()[2] += 1;
		// a live voice got no Process call this fragment: say so, or
		// the kernel would apply the default
		for(size_t vi = 0; vi < c->voices.size(); ++vi) {
			HVoice &v = c->voices[vi];
			if((c->defmap_used && vi < c->defmap.size() && c->defmap[vi]) || is_held(c, (int)vi))
				continue;	// (walked: the host marked its default window)
			if(v.live && v.started && !v.dying && v.walked != c->serial_base + f &&
					v.touched != c->serial_base + f) {
				if(v.vm >= 0)
					c->vm.unwalked = (int)vi;	// (its VM cannot be told to skip a fragment: a2amd_render fails)
				A2DRec r = { A2D_HEAD(f, R_NOP, 0, 0), 0, 0, 0 };
				if(!v.listed_recs) {
					v.listed_recs = true;
					c->with_recs.push_back((int)vi);
				}
				v.recs.push_back(r);
				v.touched = c->serial_base + f;
				if(c->sw.hosttiming)
					dbg_counters()[3] += 1;
			}
		}
	}
	c->frag_open = false;
	c->walk_time += nframes;
	c->prev_frames = nframes;
	c->defmap_used = false;
	return 0;
}

void resolve_out(a2amd_ctx *c, HVoice &v)
{
	if(v.resolved)
		return;
	v.depth = (int)c->stack.size();
	if(c->stack.empty()) {
		v.out_off = 0;
		v.out_nch = c->cfg.channels;
	} else {
		const HUnit &il = c->units[c->stack.back()];
		const HVoice &pv = c->voices[il.voice];
		if(il.wired) {
			v.out_off = pv.out_off;
			v.out_nch = pv.out_nch;
		} else {
			v.out_off = pv.own_off;
			v.out_nch = pv.own_nch;
		}
	}
	v.resolved = true;
	v.cls_stale = true;
	c->voices_dirty = true;
	c->dirty_voices.push_back((int)(&v - c->voices.data()));
	c->lists_dirty = true;
}

void sync_voice_mirror(a2amd_ctx *c, int vi)
{
	const HVoice &v = c->voices[vi];
	if(c->mvoices.size() <= (size_t)vi)
		c->mvoices.resize(vi + 1);
	A2DVoice &m = c->mvoices[vi];
	memset(&m, 0, sizeof(m));
	m.nunits = v.nunits;
	for(int i = 0; i < v.nunits && i < A2D_CHAIN_INLINE; ++i)
		m.unit[i] = v.unit[i];
	if(v.nunits > A2D_CHAIN_INLINE)
		c->long_chains = true;
	if(c->long_chains) {
		if(c->mvext.size() <= (size_t)vi)
			c->mvext.resize(vi + 1);
		A2DVoiceExt &e = c->mvext[vi];
		memset(&e, 0, sizeof(e));
		for(int i = A2D_CHAIN_INLINE; i < v.nunits; ++i)
			e.unit[i - A2D_CHAIN_INLINE] = v.unit[i];
	}
	m.out_off = v.out_off;
	m.out_nch = v.out_nch;
	m.own_off = v.own_off;
	m.own_nch = v.own_nch;
}

// what the wavetable leaf kernels play: mip-mapped waves, nothing, and - k_leaf_recs / the window kernels, k_leaf_noisepan and
// k_leaf_noisefiltpan only - noise.  The quiet kernels of the wavetable classes never see a noise oscillator: every window the
// engine calls for carries an R_NOISESEED record, and a voice whose noise windows are seeded on the device
// (a2amd_fragment_repeat_noise) is either k_leaf_noisepan's / k_leaf_noisefiltpan's or given a stand-in record run by
// upload() in a batch in which it has no record of its own.

// wtosc (mip-mapped wave playing) -> panmix 1->2 adding into the output bus
bool is_oscpan_chain(const a2amd_ctx *c, const HVoice &v)
{
	if(v.nunits != 2 || v.out_nch < 2)
		return false;
	const HUnit &o = c->units[v.unit[0]], &pm = c->units[v.unit[1]];
	return o.kind == A2AMD_WTOSC && !(o.flags & A2AMD_PROCADD) && !o.wired &&
			leaf_mode(o.mode) &&
			pm.kind == A2AMD_PANMIX && pm.nin == 1 && pm.nout == 2 && pm.wired &&
			(pm.flags & A2AMD_PROCADD);
}

// wtosc (replacing) + wtosc (adding) -> panmix 1->2 adding into the output bus
bool is_osc2pan_chain(const a2amd_ctx *c, const HVoice &v)
{
	if(v.nunits != 3 || v.out_nch < 2)
		return false;
	const HUnit &a = c->units[v.unit[0]], &b = c->units[v.unit[1]], &pm = c->units[v.unit[2]];
	return a.kind == A2AMD_WTOSC && !(a.flags & A2AMD_PROCADD) && !a.wired &&
			leaf_mode(a.mode) &&
			b.kind == A2AMD_WTOSC && (b.flags & A2AMD_PROCADD) && !b.wired &&
			leaf_mode(b.mode) &&
			pm.kind == A2AMD_PANMIX && pm.nin == 1 && pm.nout == 2 && pm.wired &&
			(pm.flags & A2AMD_PROCADD);
}

// wtosc -> filter12 (1 channel, replacing) -> panmix 1->2 adding into the output bus
bool is_oscfiltpan_chain(const a2amd_ctx *c, const HVoice &v)
{
	if(v.nunits != 3 || v.out_nch < 2)
		return false;
	const HUnit &o = c->units[v.unit[0]], &f = c->units[v.unit[1]], &pm = c->units[v.unit[2]];
	return o.kind == A2AMD_WTOSC && !(o.flags & A2AMD_PROCADD) && !o.wired &&
			leaf_mode(o.mode) &&
			f.kind == A2AMD_FILTER12 && f.nin == 1 && !f.wired && !(f.flags & A2AMD_PROCADD) &&
			// (a ramping cutoff means an R_F1RAMP record per window walked by calls, and in a stretch of repeated
			// fragments a column of the batch's sweep table, whose voices upload() gives the stand-in run: such a
			// voice is never without a run, and the quiet kernel skips voices that have one)
			pm.kind == A2AMD_PANMIX && pm.nin == 1 && pm.nout == 2 && pm.wired &&
			(pm.flags & A2AMD_PROCADD);
}

// wtosc (replacing) + wtosc (adding) -> filter12 (1 channel, replacing) -> panmix 1->2 adding into the
// output bus: the usual subtractive-synth note
bool is_osc2filtpan_chain(const a2amd_ctx *c, const HVoice &v)
{
	if(v.nunits != 4 || v.out_nch < 2)
		return false;
	const HUnit &a = c->units[v.unit[0]], &b = c->units[v.unit[1]], &f = c->units[v.unit[2]], &pm = c->units[v.unit[3]];
	return a.kind == A2AMD_WTOSC && !(a.flags & A2AMD_PROCADD) && !a.wired &&
			leaf_mode(a.mode) &&
			b.kind == A2AMD_WTOSC && (b.flags & A2AMD_PROCADD) && !b.wired &&
			leaf_mode(b.mode) &&
			f.kind == A2AMD_FILTER12 && f.nin == 1 && !f.wired && !(f.flags & A2AMD_PROCADD) &&
			pm.kind == A2AMD_PANMIX && pm.nin == 1 && pm.nout == 2 && pm.wired &&
			(pm.flags & A2AMD_PROCADD);
}

// wtosc (replacing) + wtosc (adding) + wtosc (adding) -> filter12 (1 channel, replacing) -> panmix 1->2 adding into the
// output bus: the three-oscillator subtractive lead, k_leaf_osc3filtpan's (a2amd_osc3filtpan.hip).  An oscillator on the
// noise generator is not of the class (no quiet kernel renders noise in this chain): the voice is the general kernel's, as
// before.  A 'w' write to or from noise marks the class stale and - with A2AMD_NOISE_QUIET on - rebuilds the lists; until a
// rebuild such a voice has a run in every batch (its R_NOISESEED records or the noise stand-in), which the kernel skips.
bool is_osc3filtpan_chain(const a2amd_ctx *c, const HVoice &v)
{
	if(v.nunits != 5 || v.out_nch < 2)
		return false;
	const HUnit &a = c->units[v.unit[0]], &b = c->units[v.unit[1]], &d = c->units[v.unit[2]], &f = c->units[v.unit[3]],
			&pm = c->units[v.unit[4]];
	return a.kind == A2AMD_WTOSC && !(a.flags & A2AMD_PROCADD) && !a.wired &&
			leaf_mode(a.mode) && a.mode != A2D_OSC_NOISE &&
			b.kind == A2AMD_WTOSC && (b.flags & A2AMD_PROCADD) && !b.wired &&
			leaf_mode(b.mode) && b.mode != A2D_OSC_NOISE &&
			d.kind == A2AMD_WTOSC && (d.flags & A2AMD_PROCADD) && !d.wired &&
			leaf_mode(d.mode) && d.mode != A2D_OSC_NOISE &&
			f.kind == A2AMD_FILTER12 && f.nin == 1 && !f.wired && !(f.flags & A2AMD_PROCADD) &&
			pm.kind == A2AMD_PANMIX && pm.nin == 1 && pm.nout == 2 && pm.wired &&
			(pm.flags & A2AMD_PROCADD);
}

// fmN -> panmix 1->2 adding into the output bus
bool is_fmpan_chain(const a2amd_ctx *c, const HVoice &v)
{
	if(v.nunits != 2 || v.out_nch < 2)
		return false;
	const HUnit &o = c->units[v.unit[0]], &pm = c->units[v.unit[1]];
	return o.kind >= A2AMD_FM1 && o.kind <= A2AMD_FM4R && !(o.flags & A2AMD_PROCADD) && !o.wired &&
			pm.kind == A2AMD_PANMIX && pm.nin == 1 && pm.nout == 2 && pm.wired &&
			(pm.flags & A2AMD_PROCADD);
}

// wtosc alone, wired and adding into the output bus: `struct { wtosc }` (compiler.c:3085-3106 wires the last unit's
// outputs to the voice's; the engine clamps them to the one a wtosc has, core.c:222-235 - channel 0 of the parent's bus)
bool is_oscbare_chain(const a2amd_ctx *c, const HVoice &v)
{
	if(v.nunits != 1 || v.out_nch < 1 || v.out_nch > 2)
		return false;
	const HUnit &o = c->units[v.unit[0]];
	return o.kind == A2AMD_WTOSC && (o.flags & A2AMD_PROCADD) && o.wired && o.nout == 1 && leaf_mode(o.mode);
}

// inline 0 2; panmix 2 2; xinsert 2 >  (a2_rootdriver / a2_groupdriver), or - a mono group: `struct { inline; panmix }`
// compiles to it - inline 0 1; panmix 1 2 ..., which is the same chain with the one channel read twice (panmix_process12
// against panmix_process22, panmix.c:78-115 / :191-229)
bool is_driver_chain(const a2amd_ctx *c, const HVoice &v)
{
	if((v.nunits != 3 && v.nunits != 2) || (v.own_nch != 2 && v.own_nch != 1) || v.out_nch < 2 || v.own_off < 0)
		return false;
	const HUnit &il = c->units[v.unit[0]], &pm = c->units[v.unit[1]];
	if(!(il.kind == A2AMD_INLINE && !(il.flags & A2AMD_PROCADD) && !il.wired && il.nout == v.own_nch &&
			pm.kind == A2AMD_PANMIX && pm.nin == v.own_nch && pm.nout == 2))
		return false;
	if(v.nunits == 2)
		// inline 0 2; panmix 2 >  - what the drop-in's root voice looks like from here (the root's
		// xinsert stays the engine's): the panmix itself adds into the output bus
		return pm.wired && (pm.flags & A2AMD_PROCADD);
	const HUnit &xi = c->units[v.unit[2]];
	return !pm.wired && !(pm.flags & A2AMD_PROCADD) &&
			xi.kind == A2AMD_XINSERT && xi.nin == 2 && xi.wired && (xi.flags & A2AMD_PROCADD) &&
			!xi.xio_mode;	// (clients: the general kernel serves them)
}

// a tap the frame-parallel delay kernel can take: at least one fragment long, and
// short enough not to wrap onto the frames being written

// what the two delay-chain classes share: a stereo inline in front, then nd = 1 .. 4 two-channel fbdelay units at chain
// positions 1 .. nd, every tap of each at least one fragment long and at most the delay line less one.  Wiring and
// adding mode are the callers' to test.
static bool fbd_units_ok(const a2amd_ctx *c, const HVoice &v, int nd)
{
	if(nd < 1 || nd > 4 || v.own_nch != 2 || v.out_nch < 2 || v.own_off < 0 || v.inline_pos != 0)
		return false;
	const HUnit &il = c->units[v.unit[0]];
	if(il.kind != A2AMD_INLINE || (il.flags & A2AMD_PROCADD) || il.wired || il.nout != 2)
		return false;
	for(int k = 1; k <= nd; ++k) {
		const HUnit &d = c->units[v.unit[k]];
		if(d.kind != A2AMD_FBDELAY || d.nin != 2 || d.nout != 2)
			return false;
		for(int t = 0; t < 3; ++t)
			if(!fbd_tap_ok(d.fbd_taps[t]))
				return false;
	}
	return true;
}

// inline 0 2; fbdelay 2 2 [; fbdelay 2 2 ...]; the last one wired and adding
// (the group voices of benchmark/fmtest4.a2s:83-95), every tap >= one fragment
bool is_fbdchain(const a2amd_ctx *c, const HVoice &v)
{
	const int nd = v.nunits - 1;
	if(!fbd_units_ok(c, v, nd))
		return false;
	for(int k = 1; k <= nd; ++k) {
		const HUnit &d = c->units[v.unit[k]];
		const bool last = k == nd;
		if((d.wired != 0) != last || (last && !(d.flags & A2AMD_PROCADD)))
			return false;
	}
	return true;
}

// "Windows only, and they tile": every record of the run an R_SEG, the run sorted by fragment, and the windows of a
// fragment starting at frame 0, following each other without gap or overlap, none of them empty, and ending at
// fragframes[f] - the fragment is covered exactly once, in order, which is what lets a delay chain ignore the cuts
// (fbdelay.c:69-126 is a loop over frames) and k_bus_fbdpan's windows launch find every frame's window.  Records reach
// the library through the C ABI from outside: this is checked, not assumed.
// Returns the table rows the batch needs - over its fragments, max(1, windows in the fragment): one without a record is
// the default window (0, fragframes[f]) - or 0: not windows only (or no record at all), -1: windows only, but not a tiling.
int seg_rows(const A2DRec *recs, size_t nrecs, const unsigned *fragframes, int nfrags)
{
	if(!nrecs)
		return 0;
	for(size_t i = 0; i < nrecs; ++i)
		if(A2D_ROP(recs[i].head) != R_SEG)
			return 0;
	int rows = nfrags, prev = -1;
	unsigned at = 0;	// the frame the open fragment's next window must start at
	for(size_t i = 0; i < nrecs; ++i) {
		const int f = (int)A2D_RFRAG(recs[i].head);
		const unsigned off = recs[i].dur & 0xffff, n = recs[i].dur >> 16;
		if(f >= nfrags || f < prev)
			return -1;
		if(f != prev) {
			if(prev >= 0 && at != fragframes[prev])
				return -1;
			prev = f;
			at = 0;
		} else
			++rows;		// (a fragment's first window is the row it has anyway)
		if(off != at || !n || n > fragframes[f] - at)
			return -1;
		at += n;
	}
	return at == fragframes[prev] ? rows : -1;
}

// inline 0 2; fbdelay 2 2 [; fbdelay 2 2 ...]; panmix 2 2 wired and adding - no delay wired, any of them adding or not:
// the master section of most songs (k2intro.a2s, fmtest3.a2s: `struct { inline 0 *; fbdelay * *; panmix * > }`)
bool is_fbdpan_chain(const a2amd_ctx *c, const HVoice &v)
{
	const int nd = v.nunits - 2;
	if(!fbd_units_ok(c, v, nd))
		return false;
	for(int k = 1; k <= nd; ++k)
		if(c->units[v.unit[k]].wired)
			return false;
	const HUnit &pm = c->units[v.unit[nd + 1]];
	return pm.kind == A2AMD_PANMIX && pm.nin == 2 && pm.nout == 2 && pm.wired && (pm.flags & A2AMD_PROCADD);
}

// append a launch list to list_all / to the batch's exceptions; the range it takes there
static ListRange append_range(std::vector<int> &to, const std::vector<int> &l)
{
	const ListRange r = { (int)to.size(), (int)l.size() };
	to.insert(to.end(), l.begin(), l.end());
	return r;
}

// Is k_leaf_osc2tame launched in front of k_leaf_osc2pan for a batch of these fragments (include/a2amd_osc2tame_kernel.h):
// where the walk it holds exists at all - the fused steps (bit 18 clear, the 16 byte table there) and the voice-major walk
// (the switch of value 16 clear) on, every super-chunk of every slice whole - the class is large enough to pay for a second
// launch (or bit 20), and neither bit 19 nor a2amd_osc2quiet_hold() says no.  No fragment is longer than A2D_FRAG, so
// "whole" does not depend on the slices: one slice is asked.  The one statement of the rule: launch_depth() launches by it,
// and upload() keeps a captured graph only while it gives the same answer.
static bool osc2_pair_wanted(const a2amd_ctx *c, const unsigned *frames, int nfrags)
{
	const int n = c->leaf[LEAF_OSC2PAN].count;
	return n && !(c->sw.debug & ((1 << 18) | 16 | (1 << 19))) && c->hparams.wavecoef4 && !c->osc2quiet_hold &&
			(n >= A2D_OSC2TAME_MIN || (c->sw.debug & (1 << 20))) && a2d_osc2_all_whole(frames, nfrags, 1);
}

int upload(a2amd_ctx *c)
{
	// (voices the device VM took over during this batch: the host's interpreter carries them to its
	// end - records into their lists - and their states go up, a2amd_vm.cpp)
	// (a batch with cutoff sweeps in repeated fragments: the sweep pass reads the coefficient table the device VM reads -
	// made here for the pitch table as it stands where it is not yet, with or without the device VM in use;
	// vm_prepare_batch sends it up)
	if(!c->cut_st.empty())
		vm_build_f1tab(c);
	if(int r = vm_prepare_batch(c))
		return r;
	c->last_sweeps = a2amd_sweep_batch_info{};
	c->n_cut_standin = 0;
	c->n_noise_standin = c->n_noise_quiet = c->n_noise_filt_quiet = 0;
	// (a2amd_last_batch_buses(): the lists of a quiet batch are the last upload's - nobody ramps, nothing is dropped)
	c->n_bus_windows_dropped = 0;
	c->last_bus.driver_ramping = c->last_bus.driver_windows_dropped = 0;
	c->last_fbdpan.gliding_voices = 0;
	// (a2amd_last_batch_bus_windows(): a quiet batch has no record, so no windows)
	c->last_buswin = a2amd_bus_windows_info{};
	c->last_buswin.window_cap = FBW_MAXWIN;
	// (a2amd_last_batch_osc3filt_windows(): likewise)
	c->last_osc3win = a2amd_osc3filt_windows_info{};
	if(c->sw.hosttiming) {
		// (A2AMD_HOSTTIMING: why a batch did not take the quiet path - first reason that applies)
		const int why = !c->blob_quiet ? 0 : !c->with_recs.empty() ? 1 : !c->prev_with_recs.empty() ? 2 :
				c->voices_dirty ? 3 : c->udesc_dirty ? 4 : c->waves_dirty ? 5 : c->lists_dirty ? 6 : c->ptab_dirty ? 7 :
				!c->dirty_voices.empty() ? 8 : !c->fbd_to_zero.empty() ? 9 : c->nfrags != c->blob_nfrags ? 10 :
				c->bus_used > c->d_busmem.cap ? 11 :
				memcmp(c->fragframes, c->blob_frames, (size_t)c->nfrags * sizeof(unsigned)) ? 10 : 12;
		dbg_why()[why] += 1;
	}
	if(c->blob_quiet && c->with_recs.empty() && c->prev_with_recs.empty() && c->moving.empty() && c->noise_st.empty() && c->cut_st.empty() && !c->voices_dirty &&
			!c->udesc_dirty && !c->waves_dirty && !c->lists_dirty && !c->ptab_dirty && !c->vm.list_dirty &&
			c->dirty_voices.empty() && c->fbd_to_zero.empty() && c->bus_used <= c->d_busmem.cap) {
		bool inject = false;
		for(const XioSlot &x : c->xio)
			if(x.unit >= 0 && (x.inj_used || (c->units[x.unit].xio_mode & A2AMD_XIO_INJECT)))
				inject = true;
		const bool same = c->nfrags == c->blob_nfrags &&
				!memcmp(c->fragframes, c->blob_frames, (size_t)c->nfrags * sizeof(unsigned));
		if(!inject && same) {
			// the same quiet batch again: the device has it all (graphs stay valid)
			if(c->sw.hosttiming)
				dbg_counters()[0] += 1;
			++c->quiet_streak;
			c->uploaded = true;
			return 0;
		}
		if(!inject && c->d_params && c->stream) {
			// A quiet batch again, cut into fragments differently - the engine's root voice woke
			// up in the middle of a fragment, which it does every 3 906 frames while it idles at
			// 'end' (core.c:1195), i.e. once per a2play buffer: nothing per voice has changed, only
			// the fragment table of the parameter block.  That block alone goes up again (a few
			// hundred bytes instead of a pass over every voice); graphs read it on the device and
			// stay valid while the NUMBER of fragments - their launch shapes - is the same.
			A2DParams p = c->hparams;
			p.nfrags = c->nfrags;
			p.nseed = nullptr;	// (no device-seeded noise windows in a quiet batch)
			p.nnoise = 0;
			p.cutf = nullptr;	// (... and no cutoff sweeps)
			p.ncut = 0;
			memset(p.fragframes, 0, sizeof(p.fragframes));
			memset(p.fragstart, 0, sizeof(p.fragstart));
			for(int f = 0, acc = 0; f < c->nfrags; ++f) {
				p.fragframes[f] = (uint8_t)c->fragframes[f];
				p.fragstart[f] = (uint16_t)acc;
				acc += (int)c->fragframes[f];
			}
			const int bi = c->blob_i;
			c->blob_i ^= 1;
			if(c->blob_busy[bi]) {
				HIPCHK(c, hipEventSynchronize(c->blob_ev[bi]));
				c->blob_busy[bi] = false;
			}
			if(c->h_blob[bi] && c->h_blob_cap[bi] >= sizeof(A2DParams) && c->blob_ev[bi]) {
				memcpy(c->h_blob[bi], &p, sizeof(p));
				HIPCHK(c, hipMemcpyAsync(c->d_blob.d, c->h_blob[bi], sizeof(p), hipMemcpyHostToDevice, c->stream));
				HIPCHK(c, hipEventRecord(c->blob_ev[bi], c->stream));
				c->blob_busy[bi] = true;
				c->hparams = p;
				// (... and while k_leaf_osc2tame is, as in the batch before, launched or not: a context whose class of
				// `wtosc; wtosc; panmix` voices is too small for it, or has it switched off, keeps its graphs as before)
				if(c->nfrags != c->blob_nfrags ||
						osc2_pair_wanted(c, c->fragframes, c->nfrags) != osc2_pair_wanted(c, c->blob_frames, c->nfrags)) {
					drop_graphs(c);
					c->quiet_streak = 0;
				} else
					++c->quiet_streak;
				c->blob_nfrags = c->nfrags;
				memcpy(c->blob_frames, c->fragframes, (size_t)c->nfrags * sizeof(unsigned));
				if(c->sw.hosttiming)
					dbg_counters()[0] += 1;
				c->uploaded = true;
				return 0;
			}
		}
	}
	c->blob_quiet = false;
	c->quiet_streak = 0;
	drop_graphs(c);
	const size_t nv = c->voices.size(), nu = c->units.size();
	// capacities
	// (kept: only the entries that changed are re-sent below)
	if(int r = grow(c, c->d_voices, nv, 1, true)) return r;
	if(int r = grow(c, c->d_udesc, nu, 1, false)) return r;
	if(int r = grow(c, c->d_ustate, nu, A2D_USTATE, true)) return r;
	if(int r = grow(c, c->d_ustage, c->d_ustate.cap, A2D_USTATE, false)) return r;
	if(int r = grow(c, c->d_vactive, nv, 1, true)) return r;
	if(int r = grow(c, c->d_runs, nv, 1, true)) return r;
	if(!c->noise_st.empty()) {
		// device-seeded noise windows (a2amd_fragment_repeat_noise): the batch's seed table and the oscillators' columns
		if(int r = grow(c, c->d_nseed, (size_t)c->nfrags * (size_t)c->noise_slots, 1, false)) return r;
		if(int r = grow(c, c->d_nslot, c->d_ustate.cap, 1, false)) return r;
	}
	if(!c->cut_st.empty()) {
		// cutoff sweeps in repeated fragments (a2amd_fragment_repeat[_noise]): the batch's sweep table and the filters' columns
		if(int r = grow(c, c->d_cutf, (size_t)c->nfrags * (size_t)c->cut_slots, 1, false)) return r;
		if(int r = grow(c, c->d_cslot, c->d_ustate.cap, 1, false)) return r;
	}
	{
		const int32_t *before = c->d_busmem.d;
		if(int r = grow(c, c->d_busmem, c->bus_used, 1, false)) return r;
		if(c->d_busmem.d != before)
			c->others_clean = c->root_clean = false;
	}
	if(c->fbd_count)
		if(int r = grow(c, c->d_fbdmem, c->fbd_count, 2 * (size_t)A2D_FBD_BUFSIZE, true)) return r;
	if(!c->xio.empty()) {
		if(int r = grow(c, c->d_xio, c->xio.size(), A2D_XIO_SLOT, true)) return r;
		// what the WRITE clients produced for this batch's fragments
		const size_t n = (size_t)c->nfrags * A2AMD_MAXCHANNELS * A2D_FRAG;
		for(size_t k = 0; k < c->xio.size(); ++k) {
			XioSlot &x = c->xio[k];
			// (also when the clients left in the middle of the batch, and zeros
			// over last batch's when they produced nothing)
			if(x.unit < 0 || !(x.inj_used || (c->units[x.unit].xio_mode & A2AMD_XIO_INJECT)))
				continue;
			HIPCHK(c, hipMemcpyAsync(c->d_xio.d + k * A2D_XIO_SLOT + A2D_XIO_HALF, x.inj.data(),
					n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
			HIPCHK(c, hipStreamSynchronize(c->stream));
			if(x.inj_used)
				std::fill(x.inj.begin(), x.inj.begin() + n, 0);
			x.inj_used = false;
		}
	}
	if(c->fm_count) {
		if(int r = grow(c, c->d_fmstate, c->fm_count, A2D_FMSTATE, true)) return r;
		if(!c->d_fmsine) {
			// fm_OpenState, fm.c:493-501: one period of sine and one pad
			// sample, computed here with the reference's own expression
			// (libm on the host) and shipped as {s[i], s[i+1] - s[i]} pairs
			int16_t sine[2049];
			uint32_t pairs[2048];
			for(int k = 0; k < 2049; ++k)
				sine[k] = (int16_t)(sin(k * 2.0f * M_PI / 2048) * 32767.0f);
			for(int k = 0; k < 2048; ++k)
				pairs[k] = (uint32_t)(uint16_t)sine[k] | ((uint32_t)(sine[k + 1] - sine[k]) << 16);
			HIPCHK(c, hipMalloc((void **)&c->d_fmsine, sizeof(pairs)));
			HIPCHK(c, hipMemcpy(c->d_fmsine, pairs, sizeof(pairs), hipMemcpyHostToDevice));
		}
	}

	if(c->voices_dirty && nv) {
		// re-upload the span of voice table entries that changed
		if(c->mvoices.size() < nv)
			c->mvoices.resize(nv);
		int lo = (int)nv, hi = -1;
		for(int vi : c->dirty_voices)
			if(vi < (int)nv) {
				sync_voice_mirror(c, vi);
				lo = std::min(lo, vi);
				hi = std::max(hi, vi);
			}
		c->dirty_voices.clear();
		if(hi >= lo)
			HIPCHK(c, hipMemcpyAsync(c->d_voices.d + lo, c->mvoices.data() + lo,
					(size_t)(hi - lo + 1) * sizeof(A2DVoice), hipMemcpyHostToDevice, c->stream));
		if(c->long_chains) {
			// (the first chain of more than 8 units: the side array comes into being, whole; from then on it follows the
			// voice table's dirty span)
			const bool fresh = c->d_vext.cap < c->d_voices.cap;
			if(int r = grow(c, c->d_vext, c->d_voices.cap, 1, true)) return r;
			if(c->mvext.size() < nv)
				c->mvext.resize(nv);
			const int elo = fresh ? 0 : lo, ehi = fresh ? (int)nv - 1 : hi;
			if(ehi >= elo)
				HIPCHK(c, hipMemcpyAsync(c->d_vext.d + elo, c->mvext.data() + elo,
						(size_t)(ehi - elo + 1) * sizeof(A2DVoiceExt), hipMemcpyHostToDevice, c->stream));
		}
		c->voices_dirty = false;
	}
	if(c->udesc_dirty && nu) {
		HIPCHK(c, hipMemcpyAsync(c->d_udesc.d, c->mudesc.data(), nu * sizeof(uint32_t),
				hipMemcpyHostToDevice, c->stream));
		c->udesc_dirty = false;
	}
	if(c->waves_dirty && !c->mwaves.empty()) {
		if(int r = grow(c, c->d_waves, c->mwaves.size(), 1, false)) return r;
		HIPCHK(c, hipMemcpyAsync(c->d_waves.d, c->mwaves.data(), c->mwaves.size() * sizeof(A2DWave),
				hipMemcpyHostToDevice, c->stream));
		c->waves_dirty = false;
	}
	if(c->ptab_dirty) {
		HIPCHK(c, hipMemcpyAsync(c->d_ptab, c->ptab, sizeof(c->ptab), hipMemcpyHostToDevice, c->stream));
		c->ptab_dirty = false;
	}
	for(int b : c->fbd_to_zero)
		HIPCHK(c, hipMemsetAsync(c->d_fbdmem.d + (size_t)b * 2 * A2D_FBD_BUFSIZE, 0,
				2 * (size_t)A2D_FBD_BUFSIZE * sizeof(int32_t), c->stream));
	c->fbd_to_zero.clear();

	// Records: one contiguous run per voice that has any.  The device keeps a
	// dense runs[slot] table (zero = quiet voice); only the entries that change
	// are written, by a scatter kernel: this batch's runs, and zeros for the
	// voices that carried records last batch but not now.
	std::vector<A2DRec> &recs = c->up_recs;
	std::vector<int> &sc_idx = c->up_idx, &now = c->up_now;
	std::vector<A2DRun> &sc_val = c->up_val;
	recs.clear();
	now.clear();
	{
		const size_t nsc = c->with_recs.size() + c->prev_with_recs.size();
		sc_idx.resize(nsc);
		sc_val.resize(nsc);
		now.resize(c->with_recs.size());
	}
	size_t nsc_used = 0, nnow = 0;
	for(int vi : c->with_recs) {
		HVoice &v = c->voices[vi];
		if(v.recs.empty()) {
			v.listed_recs = false;
			continue;
		}
		// A group voice with the stateless chain inline -> panmix -> xinsert whose records are windows only - its own VM
		// woke inside a fragment (a sequencer that spawns notes), or its parent's did - and whose volume and pan are at
		// rest: the windows change nothing (a2_PrepareRamper with no ramp under way sets the same gains for every window,
		// a2_dsp.h:128-133; inline, panmix and xinsert keep no state from frame to frame), so it stays with the bus
		// kernel of its depth instead of going to the general kernel - one wavefront that is as long as the batch.
		if(!c->sw.bus_windows && v.inline_pos >= 0 && v.vm < 0 && v.moving_until <= c->vm.batch_time && !(c->sw.no_fast & 4) &&
				v.resolved && is_driver_chain(c, v)) {
			bool only_windows = true;
			for(const A2DRec &r : v.recs)
				if(A2D_ROP(r.head) != R_SEG) {
					only_windows = false;
					break;
				}
			if(only_windows) {
				++c->n_bus_windows_dropped;
				v.recs.clear();
				v.listed_recs = false;
				continue;
			}
		}
		// ... and a group voice `inline; fbdelay [; fbdelay ...]` with the last delay wired (k_bus_fbdchain's), whatever its
		// delays hold: fbdelay has no ramper and never sees a window - fbdelay_process (fbdelay.c:69-126) is a loop over
		// frames that reads its parameters as plain integers and advances bufpos once per frame - so windows that cover
		// each fragment exactly once, in order, leave the same delay lines, outputs and bufpos as the whole fragment, and
		// inline picks its children's sum out of a bus they have filled independently.  seg_rows() checks the covering;
		// a run that fails it stays: the general kernel's.  (is_fbdchain() itself, not v.cls: the class may be stale in
		// front of the list rebuild below.  The pan-tailed chains keep their runs: the exception lists below.)
		else if(!c->sw.bus_windows && v.inline_pos >= 0 && v.vm < 0 && v.resolved && v.depth > 0 && !(c->sw.no_fast & 32) &&
				is_fbdchain(c, v)) {
			const int rows = seg_rows(v.recs.data(), v.recs.size(), c->fragframes, c->nfrags);
			if(rows > 0) {
				++c->last_buswin.fbd_dropped;
				v.recs.clear();
				v.listed_recs = false;
				continue;
			}
			c->last_buswin.refused_tiling += rows < 0;
		}
		A2DRun r = { (int)recs.size(), (int)v.recs.size() };
		recs.insert(recs.end(), v.recs.begin(), v.recs.end());
		sc_idx[nsc_used] = vi;
		sc_val[nsc_used++] = r;
		now[nnow++] = vi;
	}
	// Voices without records whose controls are still gliding (HVoice::moving_until): the quiet kernels take an
	// unsettled voice fragment by fragment on the scalar unit for the whole batch; the window kernels resolve its
	// rampers in closed form.  They are given ONE shared stand-in record that belongs to no fragment - a run the
	// quiet kernels skip and the control pass never consumes: default windows throughout.
	c->n_moving_listed = 0;
	int nop_at = -1;
	// the stand-in run for voice vi (no records of its own this batch): used for gliding voices here and for
	// device-seeded noise voices below
	auto give_stand_in = [&](int vi) {
		HVoice &v = c->voices[vi];
		if(nop_at < 0) {
			nop_at = (int)recs.size();
			A2DRec nop = { A2D_HEAD(0xffff, R_NOP, 0, 0), 0, 0, 0 };
			recs.push_back(nop);
		}
		const A2DRun r = { nop_at, 1 };
		sc_idx.resize(nsc_used + 1 + c->prev_with_recs.size());
		sc_val.resize(sc_idx.size());
		sc_idx[nsc_used] = vi;
		sc_val[nsc_used++] = r;
		now.resize(nnow + 1);
		now[nnow++] = vi;
		v.moving_run = c->serial_base;
		v.listed_recs = true;
		++c->n_moving_listed;
	};
	if(!c->moving.empty()) {
		const uint64_t t0 = c->vm.batch_time;	// walk_time when this batch began
		for(size_t i = 0; i < c->moving.size();) {
			const int vi = c->moving[i];
			HVoice &v = c->voices[vi];
			if(!(v.live || v.dying) || v.moving_until <= t0) {
				v.listed_moving = false;
				v.moving_until = 0;
				c->moving[i] = c->moving.back();
				c->moving.pop_back();
				continue;
			}
			++i;
			// (a voice slot that was recycled while it stood in the list stands in it twice)
			if(v.moving_run == c->serial_base)
				continue;
			if(c->sw.no_moving || !v.recs.empty() || v.vm >= 0 || c->lists_dirty || v.mode_mix || !v.resolved ||
					!(v.cls == CLS_OSCPAN || v.cls == CLS_OSC2PAN || v.cls == CLS_OSCFILTPAN || v.cls == CLS_OSC2FILTPAN))
				continue;
			give_stand_in(vi);
		}
	}
	// Voices with a filter in this batch's sweep table (a2amd_fragment_repeat[_noise] with a cutoff sweeping) and no record
	// in the whole batch: the same stand-in run keeps them with the kernels that read the table - the window kernels /
	// k_leaf_recs for the wavetable classes, the general kernel (which takes its voices with or without records) for any
	// other chain.  The quiet kernels render settled filters only and skip a voice that has a run: they never see one,
	// whatever its class (as for noise below, the run is given whether or not the class is known for sure).
	for(const A2DCutSweep &e : c->cut_list) {
		const int vi = c->units[e.unit].voice;
		HVoice &v = c->voices[vi];
		if(v.cut_run == c->serial_base)
			continue;	// (a voice with two sweeping filters, a filter listed by two stretches)
		v.cut_run = c->serial_base;
		if(!v.recs.empty() || !(v.live || v.dying))
			continue;
		if(v.moving_run != c->serial_base)
			give_stand_in(vi);
		++c->n_cut_standin;
	}
	// Voices with a noise oscillator in a device-seeded stretch (a2amd_fragment_repeat_noise) and no record in the whole
	// batch: the same stand-in run keeps them with the kernels that regenerate a window's draws from a seed - the window
	// kernels / k_leaf_recs for the four wavetable classes, the general kernel (which takes its voices with or without
	// records) for any other chain.  The quiet kernels of the wavetable classes know no noise.
	// (unlike a gliding voice, which the quiet kernels can take the slow way when its class is not known for sure -
	// lists_dirty, mode_mix - a noise voice gets the run whatever its class: those kernels must never see one)
	// The exceptions are the two classes with a quiet kernel of their own, wtosc (noise) -> panmix (k_leaf_noisepan, round 7)
	// and wtosc (noise) -> filter12 -> panmix (k_leaf_noisefiltpan): a voice is left WITHOUT the run when its remembered class
	// is CLS_NOISEPAN / CLS_NOISEFILTPAN and still stands (a stale one may be any class once the lists are rebuilt below; one
	// that stands comes out of a rebuild as it went in), its amplitude, q, volume and pan are at rest (moving_until, the test
	// of the list above: the kernels render settled voices only), no filter of it has a column of this batch's sweep table
	// (cut_run: a cutoff sweeping in a device-seeded stretch - such a voice has taken the run above) and A2AMD_NOISE_QUIET
	// is not 0.
	// The filter class moreover only from nzf_min such voices IN THIS BATCH on (A2AMD_NZF_MIN, a2amd_host.h): they are
	// counted first - from the remembered classes, so the count is the same whether or not the lists are rebuilt below -
	// and below the threshold every one of them takes the run, as before the class had a kernel.
	// Invariant, for both classes: a noise oscillator never stands in k_leaf_oscpan's / k_leaf_oscfiltpan's list without a
	// record - a noise-mode voice is classified CLS_NOISEPAN / CLS_NOISEFILTPAN, never CLS_OSCPAN / CLS_OSCFILTPAN, and while
	// a remembered CLS_OSCPAN / CLS_OSCFILTPAN is stale (a 'w' write to noise) it has the run - and a recordless noise voice
	// is rendered by exactly one kernel, whether or not the lists are rebuilt in this upload(): runs[v].count == 0 <=> the
	// quiet kernel of its segment - k_leaf_noisepan and k_leaf_noisefiltpan take the voices of their segments whose run is
	// empty, every other kernel those whose run is not.
	{
		const uint64_t t0 = c->vm.batch_time;
		// a voice a quiet noise kernel may take: which of the two classes (0: neither)
		auto quiet_cls = [&](const HVoice &v) {
			return c->sw.noise_quiet && (v.cls == CLS_NOISEPAN || v.cls == CLS_NOISEFILTPAN) && !v.cls_stale && v.resolved &&
					v.vm < 0 && v.recs.empty() && (v.live || v.dying) && v.moving_until <= t0 && v.cut_run != c->serial_base ?
					v.cls : 0;
		};
		// (a voice of either class has one oscillator: it is met once)
		int nfilt = 0;
		for(const A2DNoiseOsc &o : c->noise_osc) {
			const HVoice &v = c->voices[c->units[o.unit].voice];
			nfilt += v.noise_run != c->serial_base && v.moving_run != c->serial_base && quiet_cls(v) == CLS_NOISEFILTPAN;
		}
		const bool filt_quiet = nfilt >= c->sw.nzf_min;
		for(const A2DNoiseOsc &o : c->noise_osc) {
			const int vi = c->units[o.unit].voice;
			HVoice &v = c->voices[vi];
			if(v.noise_run == c->serial_base)
				continue;	// (a voice with two noise oscillators)
			v.noise_run = c->serial_base;
			if(!v.recs.empty() || !(v.live || v.dying))
				continue;
			const int qc = quiet_cls(v);
			const bool quiet = qc == CLS_NOISEPAN || (qc == CLS_NOISEFILTPAN && filt_quiet);
			if(v.moving_run != c->serial_base && !quiet)
				give_stand_in(vi);
			if(v.moving_run == c->serial_base)
				++c->n_noise_standin;
			else if(qc == CLS_NOISEFILTPAN)
				++c->n_noise_filt_quiet;
			else
				++c->n_noise_quiet;
		}
	}
	now.resize(nnow);
	c->with_recs.swap(now);
	if(sc_idx.size() < nsc_used + c->prev_with_recs.size()) {
		sc_idx.resize(nsc_used + c->prev_with_recs.size());
		sc_val.resize(sc_idx.size());
	}
	for(int vi : c->prev_with_recs)
		if(vi < (int)nv && c->voices[vi].recs.empty() && c->voices[vi].moving_run != c->serial_base) {
			A2DRun z = { 0, 0 };
			sc_idx[nsc_used] = vi;
			sc_val[nsc_used++] = z;
		}
	sc_idx.resize(nsc_used);
	sc_val.resize(nsc_used);
	c->prev_with_recs.clear();
	c->stats.records += recs.size();
	if(c->sw.hosttiming) {
		dbg_counters()[1] += (double)recs.size();
		dbg_counters()[4] += (double)c->with_recs.size();
	}

	// Launch lists (a2amd_host.h: ListRange).  Static part, rebuilt when the voice tree changes: every listed voice by class.
	if(c->lists_dirty) {
		const bool cls_check = c->sw.cls_check;
		bool owners_ok = !c->sw.no_selfclean, root_driver = false;
		std::vector<int> leaf[LEAF_N];
		std::map<int, std::pair<std::vector<int>, std::vector<int>>> bydepth;
		std::map<int, std::vector<int>> fbd_bydepth, fbdpan_bydepth;
		int maxdepth = -1;
		for(size_t vi = 0; vi < nv; ++vi) {
			HVoice &v = c->voices[vi];
			// voices that died during this batch still render up to their
			// R_KILL record
			if(!(v.live || v.dying) || !v.resolved) {
				v.cls = -1;
				continue;
			}
			// (what a voice's class is made of - its units' kinds, wiring and modes, its place in the tree, clients on its
			// xinsert, delay taps, mode_mix - changes at a handful of places, each of which says so: cls_stale.  A rebuild -
			// one per batch in which a note is born or ends - classifies only those voices; A2AMD_CLS_CHECK=1, the test
			// suite's setting, classifies all and fails if a remembered class is not what comes out)
			const bool classify = v.cls_stale || v.cls < 0 || cls_check;
			const int was_cls = v.cls;
			if(v.inline_pos >= 0) {
				auto &d = bydepth[v.depth];
				if(classify)
					v.cls = !(c->sw.no_fast & 4) && is_driver_chain(c, v) ? CLS_BUSDRIVER :
							!(c->sw.no_fast & 32) && v.depth > 0 && is_fbdchain(c, v) ? CLS_FBDCHAIN :
							// (a root of this shape stays general: the master bus is the root driver's to store)
							!(c->sw.no_fast & 512) && v.depth > 0 && is_fbdpan_chain(c, v) ? CLS_FBDPAN : CLS_BUSGENERIC;
				// (the master bus at offset 0 is the root's alone)
				if(v.cls == CLS_BUSGENERIC || (v.out_off == 0) != (v.depth == 0))
					owners_ok = false;
				else if(v.depth == 0)
					root_driver = true;
				(v.cls == CLS_BUSDRIVER ? d.first : v.cls == CLS_FBDCHAIN ? fbd_bydepth[v.depth] :
						v.cls == CLS_FBDPAN ? fbdpan_bydepth[v.depth] : d.second).push_back((int)vi);
				maxdepth = std::max(maxdepth, v.depth);
			} else {
				if(classify)
					v.cls = !(c->sw.no_fast & 1) && is_oscpan_chain(c, v) ?
								// (the noise generator: a class of its own, k_leaf_noisepan - a 'w' write marks the class stale)
								(c->sw.noise_quiet && c->units[v.unit[0]].mode == A2D_OSC_NOISE ? CLS_NOISEPAN : CLS_OSCPAN) :
							!(c->sw.no_fast & 8) && is_osc2pan_chain(c, v) ? CLS_OSC2PAN :
							!(c->sw.no_fast & 2) && is_oscfiltpan_chain(c, v) ?
								// (likewise: k_leaf_noisefiltpan's, whatever their number - upload() counts them batch by batch)
								(c->sw.noise_quiet && c->units[v.unit[0]].mode == A2D_OSC_NOISE ? CLS_NOISEFILTPAN : CLS_OSCFILTPAN) :
							// (no quiet kernel of its own: k_leaf_recs renders it, records or not - unless an
							// oscillator leaves the mip-mapped waves somewhere in this batch)
							!(c->sw.no_fast & 128) && !v.mode_mix && is_osc2filtpan_chain(c, v) ? CLS_OSC2FILTPAN :
							!(c->sw.no_fast & 16) && is_fmpan_chain(c, v) ? CLS_FMPAN :
							// (a voice the device VM runs stays with the general kernel: the host cannot tell in which
							// batches the VM writes it records - adoption and recall mark the class stale, a2amd_vm.cpp)
							!(c->sw.no_fast & 256) && v.vm < 0 && is_oscbare_chain(c, v) ? CLS_OSCBARE :
							// (likewise, and - as for the two-oscillator note - not while an oscillator leaves the mip-mapped
							// waves somewhere in this batch)
							!(c->sw.no_fast & 1024) && v.vm < 0 && !v.mode_mix && is_osc3filtpan_chain(c, v) ? CLS_OSC3FILTPAN :
							CLS_GENERIC;
				if(v.out_off == 0)
					owners_ok = false;	// adds straight into the master bus
				leaf[cls_lists[v.cls].leaf].push_back((int)vi);
			}
			if(cls_check && !v.cls_stale && was_cls >= 0 && was_cls != v.cls)
				return c->fail(A2AMD_ESTATE, "voice %zu: remembered launch class %d, classified %d (a change nobody reported)",
						vi, was_cls, v.cls);
			v.cls_stale = false;
		}
		auto by_bus = [&](int a, int b) { return c->voices[a].out_off < c->voices[b].out_off; };
		// (slots follow the order of birth, births the walk: a class is usually grouped by bus already - one pass
		// says so, where a sort of 16 384 voices by a key two loads away was most of a rebuild; a scene with a note
		// born or ended in most batches rebuilds in most batches)
		for(int k = 0; k < LEAF_N; ++k)
			if(k != LEAF_FMPAN && !std::is_sorted(leaf[k].begin(), leaf[k].end(), by_bus))
				std::stable_sort(leaf[k].begin(), leaf[k].end(), by_bus);
		// fm voices, grouped by unit kind: one launch per kind present
		std::stable_sort(leaf[LEAF_FMPAN].begin(), leaf[LEAF_FMPAN].end(), [&](int a, int b) {
			const int ka = c->units[c->voices[a].unit[0]].kind, kb = c->units[c->voices[b].unit[0]].kind;
			return ka != kb ? ka < kb : c->voices[a].out_off < c->voices[b].out_off;
		});
		for(int k = 0; k < 8; ++k)
			c->fm_kind_count[k] = 0;
		for(int vi : leaf[LEAF_FMPAN])
			++c->fm_kind_count[c->units[c->voices[vi].unit[0]].kind - A2AMD_FM1];
		c->list_all.clear();
		for(int k = 0; k < LEAF_N; ++k)
			c->leaf[k] = append_range(c->list_all, leaf[k]);
		c->depth_ranges.assign(maxdepth + 1, DepthRange());
		for(int d = 0; d <= maxdepth; ++d) {
			DepthRange &r = c->depth_ranges[d];
			r.driver = append_range(c->list_all, bydepth[d].first);
			r.fbd = append_range(c->list_all, fbd_bydepth[d]);
			r.fbdpan = append_range(c->list_all, fbdpan_bydepth[d]);
			r.generic = append_range(c->list_all, bydepth[d].second);
		}
		if(int r = grow(c, c->d_list, c->list_all.size() + 64, 1, false)) return r;
		if(int r = grow(c, c->d_staged, c->d_list.cap, 1, false)) return r;	// (one marker per list entry)
		if(int r = grow(c, c->d_osc2_taken, c->d_list.cap, 1, false)) return r;	// (one per wavefront of a list: no more than its entries)
		if(!c->list_all.empty())
			HIPCHK(c, hipMemcpyAsync(c->d_list.d, c->list_all.data(), c->list_all.size() * sizeof(int),
					hipMemcpyHostToDevice, c->stream));
		c->lists_dirty = false;
		c->owners_all_driver = owners_ok && root_driver;
		if(!c->vm.list.empty() || c->vm.stats.live)
			c->vm.list_dirty = true;	// (launch classes may have moved)
	}
	if(int r = vm_build_lists(c))
		return r;
	std::vector<int> dyn_all;
	{
		// this batch's exceptions (shipped in the blob)
		// Voices of the wtosc[+wtosc]->panmix classes whose records are what
		// k_leaf_recs executes (windows, writes, births, deaths; oscillators on
		// mip-mapped waves throughout the batch) go first, by class; the rest -
		// filter voices, a wave of another kind somewhere in the batch - to the
		// general kernel.
		std::vector<int> dyn[DYN_N];
		std::vector<std::vector<int>> dyn_bus(c->depth_ranges.size()), fbdpan_win(c->depth_ranges.size());
		const bool no_recs_kernel = (c->sw.no_fast & 64) != 0;
		for(int vi : c->with_recs) {
			HVoice &v = c->voices[vi];
			if(c->sw.vm_dump)	// (debugging aid: the records of a batch, host-made ...)
				for(const A2DRec &r : v.recs)
					fprintf(stderr, "REC %lld v%d f%u op%u u%u r%u val %d dur %u start %u\n", c->serial_base, vi,
							A2D_RFRAG(r.head), A2D_ROP(r.head), A2D_RUNIT(r.head), A2D_RREG(r.head), r.value, r.dur, r.start);
			// (fm-panmix voices execute their own records in k_leaf_fmpan)
			if(v.cls == CLS_OSCPAN || v.cls == CLS_NOISEPAN || v.cls == CLS_OSCFILTPAN || v.cls == CLS_NOISEFILTPAN || v.cls == CLS_OSC2PAN ||
					v.cls == CLS_OSC2FILTPAN) {
				// (close_fragment's R_NOP is the one other record k_leaf_recs takes - as nothing)
				const bool ok = !no_recs_kernel && !v.mode_mix && !v.fancy_recs;
				// (on a list already, whichever: a voice the general kernel takes - DYN_REST - must not be put on DYN_FILT2 as
				// well by the small-scene rule below and rendered twice)
				if(v.cls == CLS_OSC2FILTPAN)
					v.dynf2_run = c->serial_base;
				dyn[ok ? cls_lists[v.cls].dyn : DYN_REST].push_back(vi);
			} else if(v.cls == CLS_OSCBARE || v.cls == CLS_OSC3FILTPAN) {
				// (a bare wtosc with records - or the stand-in run of a noise oscillator in a device-seeded stretch: the general
				// kernel's, which renders the voices on its exception list; k_leaf_oscbare skips a voice that has a run.
				// 3 x wtosc-filter12-panmix likewise: records of its own, the stand-in of a cutoff in the batch's sweep table or of
				// a noise oscillator - k_leaf_osc3filtpan skips it)
				// But for a lead whose run is windows only and tiles its fragments (seg_rows(); the classes are fresh here): it
				// keeps the run and its class - k_leaf_osc3filtpan's windows launch steps every ramper window by window
				// (include/a2amd_osc3win.h).  It stands on no other list: the whole-fragment launch skips it for its run, the
				// general kernel never sees it.  What the kernel's own test of the voice relies on (a2amd_osc3filtpan.hip):
				// mode_mix - no oscillator off the mip-mapped waves in this batch; a filter with a column of the batch's sweep
				// table or a noise oscillator in a device-seeded stretch (cut_run / noise_run, marked above) is the general
				// kernel's as before; a cutoff ramp leaves R_F1* records, so such a run is not windows only.
				if(v.cls == CLS_OSC3FILTPAN && !(c->sw.no_fast & 2048) && v.vm < 0 && v.resolved && !v.mode_mix &&
						v.cut_run != c->serial_base && v.noise_run != c->serial_base) {
					const int rows = seg_rows(v.recs.data(), v.recs.size(), c->fragframes, c->nfrags);
					a2amd_osc3filt_windows_info &ow = c->last_osc3win;
					if(rows > 0) {
						dyn[DYN_OSC3WIN].push_back(vi);
						++ow.window_voices;
						ow.gliding_voices += v.moving_until > c->vm.batch_time;
						ow.windows += (uint32_t)rows;
						continue;
					}
					ow.refused_tiling += rows < 0;
				}
				dyn[DYN_REST].push_back(vi);
			} else if((v.cls == CLS_BUSDRIVER || v.cls == CLS_FBDCHAIN || v.cls == CLS_FBDPAN) && v.depth < (int)dyn_bus.size()) {
				// A pan-tailed delay chain whose run is windows only and tiles its fragments (seg_rows(); the classes are fresh
				// here) keeps the run and its kernel: k_bus_fbdpan's windows launch of the depth, which steps volume and pan
				// window by window as panmix_process22 would (a2_PrepareRamper once per window, a2_dsp.h:128-149) and ignores
				// the run where they are at rest - its thread 0 decides that from the ramper words, not the host; the delays
				// and inline never see a window.  It is on no other exception list - the general kernel never sees it, the
				// launch over r.fbdpan skips it for its run - and is no reason to give up the self-cleaning buses.
				if(v.cls == CLS_FBDPAN && !c->sw.bus_windows && !(c->sw.no_fast & 512) && v.depth > 0 && v.vm < 0 && v.resolved) {
					const int rows = seg_rows(v.recs.data(), v.recs.size(), c->fragframes, c->nfrags);
					a2amd_bus_windows_info &bw = c->last_buswin;
					if(rows > 0 && rows <= FBW_MAXWIN) {
						fbdpan_win[v.depth].push_back(vi);
						++bw.fbdpan_voices;
						bw.fbdpan_gliding += v.moving_until > c->vm.batch_time;
						bw.fbdpan_windows += (uint32_t)rows;
						continue;
					}
					bw.refused_tiling += rows < 0;
					bw.refused_cap += rows > FBW_MAXWIN;
				}
				dyn_bus[v.depth].push_back(vi);
				if(c->sw.hosttiming_level >= 3 && !v.recs.empty())
					fprintf(stderr, "a2amd: bus voice %d (depth %d, class %d) carries %zu records, first: frag %u op %u unit %u reg %u value %d\n",
							vi, v.depth, v.cls, v.recs.size(), A2D_RFRAG(v.recs[0].head), A2D_ROP(v.recs[0].head),
							A2D_RUNIT(v.recs[0].head), A2D_RREG(v.recs[0].head), v.recs[0].value);
			}
		}
		// Round 6: 2 x wtosc-filter12-panmix has a quiet kernel of its own (k_leaf_osc2filtpan) and rounds 2-5's "the records
		// kernels render every voice of the class" is over: like the other three classes, a voice is the quiet kernel's
		// in a batch in which its run is empty and the records / window kernels' otherwise.  Whose records the DEVICE VM
		// writes (k_vm_emit, after this list is made) the host cannot tell which it will be: the class's adopted voices
		// stand on the list in every batch, and the list is taken with skip_empty - the one rule "runs[v].count == 0 <=>
		// the quiet kernel's" decides for every voice, whoever wrote its records.
		for(int vi : c->vm.o2f_voices) {
			HVoice &v = c->voices[vi];
			if(v.dynf2_run == c->serial_base || v.cls != CLS_OSC2FILTPAN || !(v.live || v.dying) || v.vm < 0)
				continue;
			v.dynf2_run = c->serial_base;
			dyn[DYN_FILT2].push_back(vi);
		}
		// ... but not in a small scene.  A launch of k_leaf_osc2filtpan takes as long as its filter wavefront's chain
		// through the batch whatever its voice count - and on the context's one stream it runs BEHIND the records kernel,
		// which renders a song's few such voices inside the launch that renders the song's other record voices
		// (measured: the 60-voice song, 500 s, 2.94 s in round 5 -> 3.53 s with the quiet kernel for its handful of notes,
		// profiles/r06_song_timing.jsonl).  Below A2AMD_O2F_MIN voices of the class (default 512) every voice of it is the
		// records / window kernels', as in rounds 2 - 5.
		const ListRange o2f = c->leaf[LEAF_OSC2FILTPAN];
		c->o2f_quiet = o2f.count >= c->sw.o2f_min;
		if(!c->o2f_quiet)
			for(int k = 0; k < o2f.count; ++k) {
				const int vi = c->list_all[o2f.first + k];
				HVoice &v = c->voices[vi];
				if(v.dynf2_run == c->serial_base || v.mode_mix)
					continue;
				v.dynf2_run = c->serial_base;
				dyn[DYN_FILT2].push_back(vi);
			}
		// (the walk order usually has them grouped by bus already)
		auto by_bus_dyn = [&](int a, int b) { return c->voices[a].out_off < c->voices[b].out_off; };
		for(int k = 0; k < DYN_N; ++k) {
			if(!std::is_sorted(dyn[k].begin(), dyn[k].end(), by_bus_dyn))
				std::stable_sort(dyn[k].begin(), dyn[k].end(), by_bus_dyn);
			c->dyn[k] = append_range(dyn_all, dyn[k]);
		}
		c->consume_ok = c->owners_all_driver;
		for(size_t d = 0; d < dyn_bus.size(); ++d) {
			c->depth_ranges[d].dyn = append_range(dyn_all, dyn_bus[d]);
			if(!dyn_bus[d].empty())
				c->consume_ok = false;	// a bus owner carries records: the general kernel renders it
			// (... but for those whose run k_bus_fbdpan's windows launch takes: a fast owner still)
			c->depth_ranges[d].fbdpan_win = append_range(dyn_all, fbdpan_win[d]);
		}
		// a2amd_last_batch_buses(): the bus owners by the kernel that renders them this batch.  k_bus_driver,
		// k_bus_fbdchain and k_bus_fbdpan leave a listed voice whose run is not empty to the general kernel (the depth's
		// exception list) - or, a pan-tailed chain with a windows-only run, to k_bus_fbdpan's windows launch (fbdpan_win above:
		// not in generic_voices; a2amd_last_batch_bus_windows() counts it).
		a2amd_bus_info &bi = c->last_bus;
		bi = a2amd_bus_info{};
		bi.driver_windows_dropped = c->n_bus_windows_dropped;
		// The drivers among them whose rampers may not be at rest (HVoice::moving_until: a2amd_unit_write sets it for every
		// write to a bus owner's panmix, gliding or not - nothing else leaves these rampers unsettled: the host's records
		// alone write them, the device VM adopts no bus owner) are listed once more, for k_bus_driver's launch of one
		// workgroup a voice: the launch over all drivers leaves an unsettled one alone.
		std::vector<int> ramp;
		c->n_mono_drivers = 0;
		for(size_t d = 0; d < c->depth_ranges.size(); ++d) {
			DepthRange &r = c->depth_ranges[d];
			ramp.clear();
			for(int k = 0; k < r.driver.count; ++k) {
				const int vi = c->list_all[r.driver.first + k];
				const HVoice &v = c->voices[vi];
				c->n_mono_drivers += v.own_nch == 1;
				if(!v.recs.empty())
					continue;
				++bi.driver_voices;
				if(v.moving_until > c->vm.batch_time)
					ramp.push_back(vi);
			}
			bi.driver_ramping += (uint32_t)ramp.size();
			r.ramp = append_range(dyn_all, ramp);
			for(int k = 0; k < r.fbd.count; ++k)
				bi.fbd_voices += c->voices[c->list_all[r.fbd.first + k]].recs.empty();
			bi.generic_voices += (uint32_t)(r.generic.count + r.dyn.count);
		}
		// a2amd_last_batch_fbdpan(): the pan-tailed delay chains by who renders them this batch.  One with records stands on
		// its depth's exception list above (record_voices: the general kernel's, less those of the windows launch,
		// a2amd_bus_windows_info.fbdpan_voices); the others are k_bus_fbdpan's, those whose volume or pan may not be at rest by
		// the host's bound (moving_until, as for the drivers) included: the class has no list of its own for them, the
		// voice's one workgroup steps the rampers itself.
		a2amd_fbdpan_batch_info &fp = c->last_fbdpan;
		fp = a2amd_fbdpan_batch_info{};
		for(const DepthRange &r : c->depth_ranges)
			for(int k = 0; k < r.fbdpan.count; ++k) {
				const HVoice &v = c->voices[c->list_all[r.fbdpan.first + k]];
				++fp.class_voices;
				fp.max_delays = std::max(fp.max_delays, (uint32_t)(v.nunits - 2));
				if(!v.recs.empty()) {
					++fp.record_voices;
					continue;
				}
				++fp.quiet_voices;
				fp.gliding_voices += v.moving_until > c->vm.batch_time;
			}
		// a2amd_last_batch_bare(): the bare wtosc voices by who renders them this batch.  One with a run - records of its
		// own, or the stand-in run of a noise oscillator in a device-seeded stretch - stands on the general kernel's list
		// above; the others are k_leaf_oscbare's, those still gliding by the host's bound (moving_until) included: the class
		// is given no stand-in run for a glide, the kernel steps the rampers itself.
		c->n_bare_quiet = c->n_bare_gliding = c->n_bare_records = 0;
		const ListRange bare = c->leaf[LEAF_OSCBARE];
		for(int k = 0; k < bare.count; ++k) {
			const HVoice &v = c->voices[c->list_all[bare.first + k]];
			if(!v.recs.empty() || v.moving_run == c->serial_base) {
				++c->n_bare_records;
				continue;
			}
			++c->n_bare_quiet;
			c->n_bare_gliding += v.moving_until > c->vm.batch_time;
		}
		// a2amd_last_batch_osc3filt(): the 3 x wtosc-filter12-panmix voices, the same way.  One with a run - records of its own,
		// the stand-in of a cutoff in the batch's sweep table or of a noise oscillator - stands on the general kernel's list
		// above; the others are k_leaf_osc3filtpan's, gliding ones included: runs[v].count == 0 <=> rendered by that kernel.
		c->n_o3f_quiet = c->n_o3f_gliding = c->n_o3f_records = 0;
		const ListRange o3f = c->leaf[LEAF_OSC3FILTPAN];
		for(int k = 0; k < o3f.count; ++k) {
			const HVoice &v = c->voices[c->list_all[o3f.first + k]];
			if(!v.recs.empty() || v.moving_run == c->serial_base) {
				++c->n_o3f_records;
				continue;
			}
			++c->n_o3f_quiet;
			c->n_o3f_gliding += v.moving_until > c->vm.batch_time;
		}
	}

	A2DParams p;
	memset(&p, 0, sizeof(p));
	p.voices = c->d_voices.d;
	p.vext = c->long_chains ? c->d_vext.d : nullptr;
	p.udesc = c->d_udesc.d;
	p.ustate = c->d_ustate.d;
	p.vactive = c->d_vactive.d;
	p.runs = c->d_runs.d;
	p.waves = c->d_waves.d;
	p.wavepool = c->d_wavepool.d;
	p.wavecoef = c->d_wavecoef.d;
	p.wavecoef4 = c->d_wavecoef4.d;
	p.busmem = c->d_busmem.d;
	p.fbdmem = c->d_fbdmem.d;
	p.ptab = c->d_ptab;
	p.fmstate = c->d_fmstate.d;
	p.xio = c->d_xio.d;
	p.fmsine = c->d_fmsine;
	if(!c->noise_st.empty()) {
		p.nseed = c->d_nseed.d;
		p.nslot = c->d_nslot.d;
		p.nnoise = c->noise_slots;
	}
	if(!c->cut_st.empty()) {
		p.cutf = c->d_cutf.d;
		p.cslot = c->d_cslot.d;
		p.ncut = c->cut_slots;
	}
	p.nfrags = c->nfrags;
	p.samplerate = c->cfg.samplerate;
	p.debug = c->sw.debug;
	for(int f = 0, acc = 0; f < c->nfrags; ++f) {
		p.fragframes[f] = (uint8_t)c->fragframes[f];
		p.fragstart[f] = (uint16_t)acc;
		acc += (int)c->fragframes[f];
	}

	// the blob: [params | records | scatter indices | scatter runs | exception lists | noise oscillators of the seed pass |
	// filters of the sweep pass]
	auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
	const size_t nsc = sc_idx.size();
	const size_t o_recs = up256(sizeof(A2DParams));
	const size_t o_idx = o_recs + up256((recs.size() + 1) * sizeof(A2DRec));
	const size_t o_val = o_idx + up256(nsc * sizeof(int));
	const size_t o_dyn = o_val + up256(nsc * sizeof(A2DRun));
	// ... and behind what the host makes, room for the records the device VM writes (a2amd_vm.cpp)
	const size_t o_noise = o_dyn + up256(dyn_all.size() * sizeof(int));
	const size_t o_cut = o_noise + up256(c->noise_osc.size() * sizeof(A2DNoiseOsc));
	const size_t host_total = o_cut + up256(c->cut_list.size() * sizeof(A2DCutSweep));
	const size_t vm_room = (size_t)vm_blob_room(c);
	const size_t total = host_total;
	if(int r = grow(c, c->d_blob, host_total + vm_room * sizeof(A2DRec), 1, false)) return r;
	c->vm.rec_off = host_total;
	c->vm.rec_cap = (uint32_t)((c->d_blob.cap - host_total) / sizeof(A2DRec));
	const int bi = c->blob_i;
	c->blob_i ^= 1;
	if(c->blob_busy[bi]) {		// the copy that last read this staging buffer must have run
		HIPCHK(c, hipEventSynchronize(c->blob_ev[bi]));
		c->blob_busy[bi] = false;
	}
	if(total > c->h_blob_cap[bi]) {
		if(c->h_blob[bi])
			HIPCHK(c, hipHostFree(c->h_blob[bi]));
		c->h_blob_cap[bi] = std::max(total * 2, (size_t)65536);
		HIPCHK(c, hipHostMalloc((void **)&c->h_blob[bi], c->h_blob_cap[bi], hipHostMallocDefault));
	}
	if(!c->blob_ev[bi])
		HIPCHK(c, hipEventCreateWithFlags(&c->blob_ev[bi], hipEventDisableTiming));
	char *hb = c->h_blob[bi];
	p.recs = (const A2DRec *)(c->d_blob.d + o_recs);
	c->hparams = p;
	memcpy(hb, &p, sizeof(p));
	if(!recs.empty())
		memcpy(hb + o_recs, recs.data(), recs.size() * sizeof(A2DRec));
	if(nsc) {
		memcpy(hb + o_idx, sc_idx.data(), nsc * sizeof(int));
		memcpy(hb + o_val, sc_val.data(), nsc * sizeof(A2DRun));
	}
	if(!dyn_all.empty())
		memcpy(hb + o_dyn, dyn_all.data(), dyn_all.size() * sizeof(int));
	if(!c->noise_osc.empty())
		memcpy(hb + o_noise, c->noise_osc.data(), c->noise_osc.size() * sizeof(A2DNoiseOsc));
	if(!c->cut_list.empty())
		memcpy(hb + o_cut, c->cut_list.data(), c->cut_list.size() * sizeof(A2DCutSweep));
	HIPCHK(c, hipMemcpyAsync(c->d_blob.d, hb, total, hipMemcpyHostToDevice, c->stream));
	HIPCHK(c, hipEventRecord(c->blob_ev[bi], c->stream));
	c->blob_busy[bi] = true;
	c->d_params = (A2DParams *)c->d_blob.d;
	c->d_dyn = (const int *)(c->d_blob.d + o_dyn);
	if(nsc)
		if(a2d_launch_scatter_runs((const int *)(c->d_blob.d + o_idx), (const A2DRun *)(c->d_blob.d + o_val),
				(int)nsc, c->d_runs.d, c->stream))
			return c->fail(A2AMD_EHIP, "scatter launch failed");
	// the seed pass: every device-seeded stretch's generator words, in front of the kernels that render its windows
	// (the columns are this batch's: an oscillator no stretch of it lists has none - a2d_noise_seed)
	if(!c->noise_st.empty())
		HIPCHK(c, hipMemsetAsync(c->d_nslot.d, 0, c->d_nslot.cap * sizeof(int32_t), c->stream));
	for(const a2amd_ctx::NoiseStretch &st : c->noise_st)
		if(const int e = a2d_launch_noise_seeds((const A2DNoiseOsc *)(c->d_blob.d + o_noise) + st.first, (int)st.n, st.start, st.f0,
				st.count, st.frames, c->d_nseed.d, c->noise_slots, c->d_nseed.cap, c->d_nslot.d, (int)c->d_nslot.cap, c->stream))
			return c->fail(A2AMD_EHIP, "noise seed launch failed: %s", hipGetErrorString((hipError_t)e));
	// the sweep pass: every cell of the batch's table says "no ramp" and no filter has a column (a2d_cut_coeff), then each
	// stretch's rampers are stepped over it (k_cut_sweep) and, once for the batch, what they left is looked up in the
	// coefficient table (k_cut_resolve) - in front of the kernels that render the windows
	if(!c->cut_st.empty()) {
		const size_t words = (size_t)c->nfrags * (size_t)c->cut_slots;
		if(!c->vm.d_f1tab || !c->vm.f1tab_up)
			return c->fail(A2AMD_ESTATE, "cutoff sweep: the coefficient table is not on the device");
		HIPCHK(c, hipMemsetAsync(c->d_cutf.d, A2CS_NONE_BYTE, words * sizeof(int32_t), c->stream));
		HIPCHK(c, hipMemsetAsync(c->d_cslot.d, 0, c->d_cslot.cap * sizeof(int32_t), c->stream));
		for(const a2amd_ctx::CutStretch &st : c->cut_st)
			if(const int e = a2d_launch_cut_sweep((const A2DCutSweep *)(c->d_blob.d + o_cut) + st.first, (int)st.n, st.f0, st.count,
					st.frames, c->d_cutf.d, c->cut_slots, words, c->d_cslot.d, (int)c->d_cslot.cap, c->stream))
				return c->fail(A2AMD_EHIP, "cutoff sweep launch failed: %s", hipGetErrorString((hipError_t)e));
		if(const int e = a2d_launch_cut_resolve(c->d_cutf.d, words, c->vm.d_f1tab, c->stream))
			return c->fail(A2AMD_EHIP, "cutoff sweep launch failed: %s", hipGetErrorString((hipError_t)e));
		c->last_sweeps.pass_launched = 1;
		c->last_sweeps.filters = (uint32_t)c->cut_slots;
		c->last_sweeps.ramp_windows = c->n_cut_windows;
		c->last_sweeps.standin_voices = c->n_cut_standin;
	}
	c->uploaded = true;
	c->blob_quiet = recs.empty() && dyn_all.empty();
	c->blob_nfrags = c->nfrags;
	memcpy(c->blob_frames, c->fragframes, (size_t)c->nfrags * sizeof(unsigned));
	return 0;
}

// Shape of the fast leaf launch, from sweeps on MI355X (DESIGN.md "Launch
// shape"): cut the batch into as many time slices as it has 8-fragment chunks
// (up to 8), then give a wavefront enough voices that about 4096 wavefronts
// (one resident round of 256 CUs x 16) share the work; at least 4 voices, so
// that their sum reaches the bus in one atomic instead of four, at most 32.
void pick_fast_shape(const A2Switches &sw, int n, int nfrags, int *vpw, int *ysplit, int ymax = 32)
{
	const int nchunks = (nfrags + A2D_FAST_FCH - 1) / A2D_FAST_FCH;
	int y = sw.ysplit_set ? sw.ysplit : ymax;
	y = std::min(std::max(y, 1), nchunks);
	int v = sw.vpw_set ? sw.vpw :
			std::min(std::max((int)(((long long)n * y + 4095) / 4096), 4), 32);
	*vpw = std::min(std::max(v, 1), 64);
	*ysplit = y;
}

int launch_depth(a2amd_ctx *c, int d, int consume, A2DCommitSet *pend)	// consume: 1 zero what is read, 2 root stores the master bus
{
	const DepthRange &r = c->depth_ranges[d];
	c->last_bus.consume = (uint32_t)consume;	// (a2amd_last_batch_buses(): the last launch is the one nearest the root)
	if(r.driver.count) {
		// (state commits the time-sliced leaf kernels left behind ride along)
		// (the root, a plain driver chain that stores the master bus: into the host's buffer where asked)
		// (... and only if nothing else adds into the master bus at depth 0: no voice with records there this
		// batch, no leaf voice mixing straight into it - owners_all_driver says so for the static lists)
		const bool direct = d == 0 && (consume & 2) && c->master_dst && r.driver.count == 1 && !r.generic.count && !r.fbd.count && !r.fbdpan.count &&
				!r.dyn.count && c->owners_all_driver && !c->capture.on;	// (a capture reads the bus memory)
		if(direct)
			c->master_direct = true;
		if(a2d_launch_bus_driver(c->d_params, c->d_list.d + r.driver.first, r.driver.count, c->nfrags, consume,
				pend, c->stream, direct ? c->master_dst : nullptr))
			return c->fail(A2AMD_EHIP, "bus driver launch failed: %s", hipGetErrorString(hipGetLastError()));
		pend->n = 0;
		++c->stats.launches;
		// ... and those of them that may still glide, one workgroup each (upload(): DepthRange::ramp)
		if(r.ramp.count) {
			if(a2d_launch_bus_driver(c->d_params, c->d_dyn + r.ramp.first, r.ramp.count, c->nfrags, consume,
					nullptr, c->stream, direct ? c->master_dst : nullptr, 1))
				return c->fail(A2AMD_EHIP, "bus driver launch failed: %s", hipGetErrorString(hipGetLastError()));
			++c->stats.launches;
		}
	}
	if(r.fbd.count) {
		if(a2d_launch_bus_fbdchain(c->d_params, c->d_list.d + r.fbd.first, r.fbd.count, consume & 1, c->stream))
			return c->fail(A2AMD_EHIP, "delay chain launch failed: %s", hipGetErrorString(hipGetLastError()));
		++c->stats.launches;
	}
	if(r.fbdpan.count) {
		if(a2d_launch_bus_fbdpan(c->d_params, c->d_list.d + r.fbdpan.first, r.fbdpan.count, consume & 1, c->stream))
			return c->fail(A2AMD_EHIP, "pan-tailed delay chain launch failed: %s", hipGetErrorString(hipGetLastError()));
		c->last_fbdpan.launched = 1;
		++c->stats.launches;
	}
	// ... and those of the class whose run is windows only (upload(): DepthRange::fbdpan_win): the same kernel in its
	// windows mode, which reads the run the launch above skipped the voice for
	if(r.fbdpan_win.count) {
		if(a2d_launch_bus_fbdpan(c->d_params, c->d_dyn + r.fbdpan_win.first, r.fbdpan_win.count, consume & 1, c->stream, 1))
			return c->fail(A2AMD_EHIP, "pan-tailed delay chain windows launch failed: %s", hipGetErrorString(hipGetLastError()));
		c->last_fbdpan.launched = c->last_buswin.launched = 1;
		++c->stats.launches;
	}
	if(r.generic.count) {
		if(a2d_launch_voices(c->d_params, c->d_list.d + r.generic.first, r.generic.count, 1, c->stream))
			return c->fail(A2AMD_EHIP, "bus launch failed: %s", hipGetErrorString(hipGetLastError()));
		++c->stats.launches;
	}
	if(r.dyn.count) {
		if(a2d_launch_voices(c->d_params, c->d_dyn + r.dyn.first, r.dyn.count, 1, c->stream))
			return c->fail(A2AMD_EHIP, "bus launch failed: %s", hipGetErrorString(hipGetLastError()));
		++c->stats.launches;
	}
	return 0;
}

int pick_vpw(int n)
{
	int v = n / 4096;
	return std::min(std::max(v, 1), (int)A2D_MAXVPW);
}

// give a region of the wave pool back: kept sorted by offset, neighbours merged
void wavepool_release(a2amd_ctx *c, size_t off, size_t len)
{
	if(!len)
		return;
	auto &fl = c->wavepool_free;
	auto it = std::lower_bound(fl.begin(), fl.end(), std::make_pair(off, (size_t)0));
	it = fl.insert(it, std::make_pair(off, len));
	if(it + 1 != fl.end() && it->first + it->second == (it + 1)->first) {
		it->second += (it + 1)->second;
		it = fl.erase(it + 1) - 1;
	}
	if(it != fl.begin() && (it - 1)->first + (it - 1)->second == it->first) {
		(it - 1)->second += it->second;
		it = fl.erase(it) - 1;
	}
	// the tail of the pool grows back into unused space
	if(it->first + it->second == c->wavepool_used) {
		c->wavepool_used = it->first;
		fl.erase(it);
	}
}

void end_batch(a2amd_ctx *c)
{
	// (graphs survive: upload() drops them unless the next batch is the same quiet one)
	// Records made after the last fragment of the batch was closed belong to
	// the first fragment of the next batch: carry them over.
	const int done = c->nfrags;
	c->serial_base += done;
	std::vector<int> carry;
	c->prev_with_recs.clear();
	for(int vi : c->with_recs) {
		HVoice &v = c->voices[vi];
		c->prev_with_recs.push_back(vi);
		size_t keep = 0;
		// (a voice that was set up but not walked yet keeps everything)
		const bool unborn = v.live && !v.resolved;
		// (the records are in fragment order: nothing to carry over unless the last one is)
		if(unborn || (!v.recs.empty() && (int)A2D_RFRAG(v.recs.back().head) >= done))
			for(size_t i = 0; i < v.recs.size(); ++i)
				if(unborn || (int)A2D_RFRAG(v.recs[i].head) >= done) {
					A2DRec r = v.recs[i];
					int f = (int)A2D_RFRAG(r.head) - done;
					r.head = (r.head & 0xffff0000u) | (uint32_t)(f < 0 ? 0 : f);
					v.recs[keep++] = r;
				}
		v.recs.resize(keep);
		v.frag_mark = 0;
		if(keep) {
			v.touched = c->serial_base;
			carry.push_back(vi);
		} else {
			v.touched = -1;
			v.listed_recs = false;
			if(v.mode_mix) {
				c->lists_dirty = true;	// (it may have its leaf class back)
				v.cls_stale = true;
			}
			v.mode_mix = false;
			v.fancy_recs = false;
		}
	}
	c->with_recs = carry;
	for(int vi : c->deferred_free_voices) {
		c->voices[vi] = HVoice();
		c->free_voices.push_back(vi);
		c->lists_dirty = true;
	}
	c->deferred_free_voices.clear();
	for(int ui : c->deferred_free_units)
		c->free_units.push_back(ui);
	c->deferred_free_units.clear();
	for(auto &b : c->deferred_bus_free)
		c->bus_free[b.second].push_back(b.first);
	c->deferred_bus_free.clear();
	for(int b : c->fbd_deferred_free)
		c->fbd_free.push_back(b);
	c->fbd_deferred_free.clear();
	for(int b : c->fm_deferred_free)
		c->fm_free.push_back(b);
	c->fm_deferred_free.clear();
	for(int b : c->xio_deferred_free) {
		c->xio[b].unit = -1;
		c->xio_free.push_back(b);
	}
	c->xio_deferred_free.clear();
	for(auto &r : c->deferred_wavepool_free)
		wavepool_release(c, r.first, r.second);
	c->deferred_wavepool_free.clear();
	for(int w : c->deferred_wave_slots)
		c->free_wave_slots.push_back(w);
	c->deferred_wave_slots.clear();
	c->noise_st.clear();
	c->noise_osc.clear();
	c->noise_slots = 0;
	c->cut_st.clear();
	c->cut_list.clear();
	c->cut_slots = 0;
	c->n_cut_windows = 0;
	c->nfrags = 0;
	c->cur_frag = 0;
	c->frag_open = false;
	c->uploaded = false;
	c->sub_resume = -1;
	c->paused_at = 0;
	vm_end_batch(c);
}

// does a voice at nesting depth d hold an xinsert in A2AMD_XIO_MUTE mode (insert clients)?
bool depth_has_mutes(const a2amd_ctx *c, int d)
{
	for(const XioSlot &x : c->xio)
		if(x.last_unit >= 0 && x.last_unit < (int)c->units.size() && (c->units[x.last_unit].xio_mode & A2AMD_XIO_MUTE) &&
				c->units[x.last_unit].voice >= 0 && c->voices[c->units[x.last_unit].voice].depth == d)
			return true;
	return false;
}

// The wavetable leaf voices that carry records this batch - the four host-made class lists (wtosc |
// 2 x wtosc [-> filter12] -> panmix; the last one with its quiet voices) and the three lists of voices
// whose records the device VM has just written - through the window kernels (a2amd_win.hip): per slab
// of the batch the control pass of every list, then the render pass of every list.  A slot per fragment
// and voice, a pool of further windows sized by the bound the control pass allocates by (one per record);
// a batch whose slots would not fit A2AMD_WIN_MB (1 024) is cut into slabs of fragments.
static int issue_windows(a2amd_ctx *c, const int *d_dyn, const ListRange *dyn, const std::function<int()> &mid)
{
	const int sset = c->vm.spec_set;	// (the speculative slot set a taken pass wrote: mid() may launch the next pass)
	// vmk >= 0: a class of VM voices run by k_vm_win; spec: ... that a speculative pass has already run for this batch
	// (vm_issue took it): its entries stand in the pass's own slot set and pool, at (sat, satw) - no control pass, no
	// room in this batch's slot memory, k_vm_commit in k_vm_win's place
	struct Job { int nosc, filt, n, skip; const int *list; int vmk; bool spec; size_t sat, satw; };
	static const int nosc[4] = { 1, 2, 1, 2 }, filt[4] = { 0, 0, 1, 1 };
	Job jobs[7];
	int nj = 0;
	size_t nvoices = 0;		// ... of the jobs that take slots here
	const bool spec = c->vm.fused && c->vm.spec_use;
	for(int k = 0; k < 4; ++k)
		if(dyn[k].count) {
			jobs[nj++] = Job{ nosc[k], filt[k], dyn[k].count, k == DYN_FILT2 && c->o2f_quiet, d_dyn + dyn[k].first, -1, false, 0, 0 };	// (DYN_FILT2: see upload())
			nvoices += (size_t)dyn[k].count;
		}
	// (the control pass takes room in the pool by the length of a voice's record run: every gliding voice's run is
	// the ONE shared stand-in record)
	size_t nrec = c->up_recs.size() + c->n_moving_listed;
	size_t nfusedv = 0;
	if(!c->vm.list.empty()) {
		const int *l = c->vm.d_list.d + c->vm.list.size();
		size_t sat = 0, satw = 0;	// (the speculative pass's layout: the three classes one after the other, vm_speculate)
		for(int k = 0; k < 3; l += c->vm.n_cls[k++])
			if(c->vm.n_cls[k]) {
				jobs[nj++] = Job{ nosc[k], filt[k], c->vm.n_cls[k], 1, l, c->vm.fused ? k : -1, spec, sat, satw };
				if(!spec)
					nvoices += (size_t)c->vm.n_cls[k];
				if(c->vm.fused && !spec)
					nfusedv += (size_t)c->vm.n_cls[k];
				sat += (size_t)c->vm.n_cls[k] * (size_t)c->nfrags;
				satw += (size_t)c->vm.n_cls[k] * (size_t)c->nfrags * A2D_WIN_SLOTWORDS(nosc[k], filt[k]);
			}
		nrec += c->vm.last_total;
	}
	// (k_vm_win takes pool room as its voices' VMs make further windows: how much was counted ahead, by k_vm_pool
	// behind the last batch - vm_issue, a2amd_vm.cpp - for exactly this batch)
	if(nfusedv)
		nrec += c->vm.pred_entries + 64;
	if(nfusedv || spec)
		++c->vm.fused_batches;
	if(!nj)
		return 0;
	// (a batch whose every list took a speculative pass takes nothing from THIS pool and has no control pass of its own:
	// its counter is neither cleared nor read back - two calls in front of the commit, two behind the render pass, of a
	// buffer whose time is the engine thread's as much as the GPU's)
	bool plain_jobs = false;
	for(int j = 0; j < nj; ++j)
		plain_jobs = plain_jobs || !jobs[j].spec;
	if(c->wtop_pending) {
		// (the copy sits behind the batch before this one: done, or nearly - waited for rather than polled, because this
		// batch's memset and copy overwrite d_wtop / h_wtop and an overflow flag not read here would be lost)
		HIPCHK(c, hipEventSynchronize(c->wtop_ev));
		c->wtop_pending = false;
		c->vm.pool_used = std::max(c->h_wtop[0], c->h_wtop[2]);
		if(c->h_wtop[1] || c->h_wtop[3]) {
			// (a bound that did not hold - the control pass's record count, k_vm_pool's prediction: never)
			c->vm.fused_off = true;
			return c->fail(A2AMD_ESTATE, "window pool overflow in an earlier batch (%u / %u entries taken of %zu): voices lost windows",
					c->h_wtop[0], c->h_wtop[2], c->d_wext.cap);
		}
	}
	const size_t budget = (size_t)c->sw.win_mb * (1u << 20) / (A2D_WIN_WORDS * sizeof(int)) / 2;
	// Slabs: the control pass (lane = voice: a few hundred wavefronts, each as long as its voices' walk) of slab
	// k + 1 runs on a stream of its own beside the render pass of slab k - two sets of slots and pools.  A batch
	// of 16 fragments or more is cut into four slabs (A2AMD_WIN_SLABS), a shorter one is one slab.
	// (measured, 16 384 scripted voices x 64 fragments: 0.50 ms as one slab, 0.76 as four - the control pass is as
	// long as ONE wavefront's walk, and a wavefront that shares its SIMD with seven render wavefronts walks at a
	// fraction of its pace - so slabs are what the memory bound asks for, not the default)
	const int nfrags = c->nfrags;
	// (a taken speculative pass covers the batch in one piece: with it, the lists that do take slots here are not cut
	// into slabs for the asking - A2AMD_WIN_SLABS - only where the memory bound demands it)
	int per = nfrags >= 16 && !spec ? (nfrags + c->sw.win_slabs - 1) / c->sw.win_slabs : nfrags;
	if(nvoices && nvoices * (size_t)per > budget)
		per = (int)std::max<size_t>(1, budget / nvoices);
	const int nslabs = (nfrags + per - 1) / per;
	const bool two = nslabs > 1;
	c->last_batch.win_slabs = (uint32_t)nslabs;
	for(int j = 0; j < nj; ++j)
		c->last_batch.win_voices += (uint32_t)jobs[j].n;
	const size_t nslots = nvoices * (size_t)per, cap = std::max<size_t>(nrec, 1);
	size_t slotwords = 0;		// of a slab: every list's slots at its class's size
	for(int j = 0; j < nj; ++j)
		if(!jobs[j].spec)
			slotwords += (size_t)jobs[j].n * (size_t)per * A2D_WIN_SLOTWORDS(jobs[j].nosc, jobs[j].filt);
	if(cap >= ((size_t)1 << 32))
		return c->fail(A2AMD_EUNSUPPORTED, "a batch of %zu records", cap);
	const size_t sets = two ? 2 : 1;
	if(sets * slotwords > c->d_win.cap || sets * cap > c->d_wext.cap || sets * nslots > c->d_widx.cap || nvoices > c->d_wrc.cap ||
			nfusedv * A2D_VMW_ROW > c->d_wscr.cap ||
			!c->d_wtop || (two && !c->win_stream)) {
		if(c->capturing)
			return c->fail(A2AMD_ESTATE, "window pool too small inside a graph capture");
		if(int r = grow(c, c->d_win, sets * slotwords, 1, false)) return r;
		if(int r = grow(c, c->d_wext, sets * cap, A2D_WIN_WORDS, false)) return r;
		if(int r = grow(c, c->d_widx, sets * nslots, 1, false)) return r;
		if(int r = grow(c, c->d_wrc, nvoices, 1, false)) return r;
		if(int r = grow(c, c->d_wscr, nfusedv * A2D_VMW_ROW, A2D_WIN_WORDS, false)) return r;
		if(!c->d_wtop) {
			HIPCHK(c, hipMalloc((void **)&c->d_wtop, 4 * sizeof(unsigned)));
			HIPCHK(c, hipMemsetAsync(c->d_wtop, 0, 4 * sizeof(unsigned), c->stream));
		}
		if(two && !c->win_stream) {
			HIPCHK(c, hipStreamCreateWithFlags(&c->win_stream, hipStreamNonBlocking));
			for(int k = 0; k < 5; ++k)
				HIPCHK(c, hipEventCreateWithFlags(&c->win_ev[k], hipEventDisableTiming));
		}
	}
	// (the sets are laid out by the CURRENT capacities: a graph captured earlier was dropped when they grew)
	const size_t half_win = c->d_win.cap / 2, half_ext = c->d_wext.cap / 2, half_idx = c->d_widx.cap / 2;
	hipStream_t sc = two ? c->win_stream : c->stream;		// the control passes' stream
	if(two) {
		// everything issued so far (uploads, the device VM's records, the quiet kernels) comes first
		HIPCHK(c, hipEventRecord(c->win_ev[4], c->stream));
		HIPCHK(c, hipStreamWaitEvent(sc, c->win_ev[4], 0));
	}
	// a list's control pass over fragments [fa, fb): k_win_ctl over its records, or - VM voices of a fused batch - k_vm_win
	uint32_t frames_to[A2D_MAXBATCH + 1];
	frames_to[0] = 0;
	for(int f = 0; f < nfrags; ++f)
		frames_to[f + 1] = frames_to[f] + (uint32_t)c->fragframes[f];
	auto control = [&](const Job &b, int fa, int fb, int *wslot, int *wext, unsigned *widx, unsigned *wtop, unsigned wcap, int *wrc,
			hipStream_t st) -> int {
		int r;
		if(b.spec) {
			// the speculative pass has done this job's control work: its results become the state (once: the first slab)
			if(fa != 0)
				return 0;
			A2DVmParams vp;
			vm_class_params(c, b.vmk, &vp);
			VmHost &m = c->vm;
			const A2DVmwOut from = { m.d_vmv_sh.d, m.d_ustate_sh.d, m.d_vactive_sh.d, m.d_runs_sh.d, m.d_stotal, nullptr };
			r = a2d_launch_vm_commit(vp, c->hparams, b.nosc, b.filt, from, st);
		} else if(b.vmk >= 0) {
			A2DVmParams vp;
			vm_class_params(c, b.vmk, &vp);
			size_t before = 0;	// (voices of the classes in front of this one: their rows of d_wscr)
			for(int q = 0; q < b.vmk; ++q)
				before += (size_t)c->vm.n_cls[q];
			int *const wscr = c->d_wscr.d + before * A2D_VMW_ROW * A2D_WIN_WORDS;
			r = a2d_launch_vm_win(vp, c->hparams, b.nosc, b.filt, fa, fb, vp.now + (frames_to[fa] << 8), vp.now + (frames_to[nfrags] << 8),
					wslot, wext, wscr, widx, wtop, wcap, st);
		} else
			r = a2d_launch_win_ctl(c->d_params, c->hparams, b.nosc, b.filt, b.list, b.n, b.skip, fa, fb, wslot, wext, widx, wtop, wcap, wrc, st);
		if(c->sw.win_sync && !r && !c->capturing) {
			const hipError_t e = hipStreamSynchronize(st);
			fprintf(stderr, "a2amd windows: control pass <%d,%d> %s of %d voices, fragments [%d, %d): %s\n", b.nosc, b.filt,
					b.spec ? "k_vm_commit (speculative pass taken)" : b.vmk >= 0 ? "k_vm_win" : "k_win_ctl", b.n, fa, fb,
					hipGetErrorString(e));
		}
		return r;
	};
	const bool wtiming = c->sw.win_timing;
	static hipEvent_t tev[3] = { nullptr, nullptr, nullptr };
	// Several lists, one slab (a song: a few dozen voices of four classes): each list's control pass and render
	// pass are kernels of a few wavefronts that take as long as one voice's walk / one filter chain - on one stream
	// they would run back to back; here every list gets a stream of its own between a fork and a join (the render
	// passes only ever ADD to the buses).  A2AMD_WIN_FORK=0: one stream.
	bool forked = false;
	if(nj > 1 && nslabs == 1 && c->sw.win_fork && !wtiming) {
		if(!c->win_fork[0]) {
			if(c->capturing)
				return c->fail(A2AMD_ESTATE, "window streams missing inside a graph capture");
			for(int j = 0; j < 7; ++j) {
				HIPCHK(c, hipStreamCreateWithFlags(&c->win_fork[j], hipStreamNonBlocking));
				HIPCHK(c, hipEventCreateWithFlags(&c->win_fev[j], hipEventDisableTiming));
			}
			HIPCHK(c, hipEventCreateWithFlags(&c->win_fev[7], hipEventDisableTiming));
		}
		if(plain_jobs)
			HIPCHK(c, hipMemsetAsync(c->d_wtop, 0, 2 * sizeof(unsigned), c->stream));
		HIPCHK(c, hipEventRecord(c->win_fev[7], c->stream));
		size_t at = 0, atw = 0, atv = 0;
		for(int j = 0; j < nj; ++j) {
			const Job &b = jobs[j];
			hipStream_t sj = c->win_fork[j];
			HIPCHK(c, hipStreamWaitEvent(sj, c->win_fev[7], 0));
			if(control(b, 0, nfrags, c->d_win.d + atw, c->d_wext.d, c->d_widx.d + at, c->d_wtop,
					(unsigned)std::min<size_t>(c->d_wext.cap, 0xffffffffu), c->d_wrc.d + atv, sj))
				return c->fail(A2AMD_EHIP, "window control launch failed: %s", hipGetErrorString(hipGetLastError()));
			if(b.spec ? a2d_launch_win_render(c->sw, c->hparams, b.nosc, b.filt, b.list, b.n, 0, nfrags, c->vm.d_swin[sset].d + b.satw,
						c->vm.d_swext[sset].d, c->vm.d_swidx[sset].d + b.sat, sj) :
					a2d_launch_win_render(c->sw, c->hparams, b.nosc, b.filt, b.list, b.n, 0, nfrags, c->d_win.d + atw,
						c->d_wext.d, c->d_widx.d + at, sj))
				return c->fail(A2AMD_EHIP, "window render launch failed: %s", hipGetErrorString(hipGetLastError()));
			HIPCHK(c, hipEventRecord(c->win_fev[j], sj));
			HIPCHK(c, hipStreamWaitEvent(c->stream, c->win_fev[j], 0));
			if(!b.spec) {
				at += (size_t)b.n * (size_t)nfrags;
				atw += (size_t)b.n * (size_t)nfrags * A2D_WIN_SLOTWORDS(b.nosc, b.filt);
				atv += (size_t)b.n;
			}
			c->stats.launches += 2;
		}
		forked = true;
	}
	int k = 0;
	for(int fa = 0; fa < nfrags && !forked; fa += per, ++k) {
		const int fb = std::min(nfrags, fa + per), set = two ? (k & 1) : 0;
		int *const wslot = c->d_win.d + (size_t)set * half_win;
		int *const wext = c->d_wext.d + (size_t)set * half_ext * A2D_WIN_WORDS;
		unsigned *const widx = c->d_widx.d + (size_t)set * half_idx;
		unsigned *const wtop = c->d_wtop + 2 * set;
		if(two && k >= 2)	// (the render pass that read this set has to be done with it)
			HIPCHK(c, hipStreamWaitEvent(sc, c->win_ev[2 + set], 0));
		if(wtiming && !two && !c->capturing) {
			for(int q = 0; q < 3; ++q)
				if(!tev[q])
					HIPCHK(c, hipEventCreate(&tev[q]));
			HIPCHK(c, hipEventRecord(tev[0], c->stream));
		}
		if(plain_jobs)
			HIPCHK(c, hipMemsetAsync(wtop, 0, 2 * sizeof(unsigned), sc));
		size_t at = 0, atw = 0, atv = 0;
		for(int j = 0; j < nj; ++j) {
			const Job &b = jobs[j];
			if(control(b, fa, fb, wslot + atw, wext, widx + at, wtop,
					(unsigned)std::min<size_t>(two ? half_ext : c->d_wext.cap, 0xffffffffu), c->d_wrc.d + atv, sc))
				return c->fail(A2AMD_EHIP, "window control launch failed: %s", hipGetErrorString(hipGetLastError()));
			if(b.spec)
				continue;	// (no slots of this batch's: the speculative pass's own)
			at += (size_t)b.n * (size_t)(fb - fa);
			atw += (size_t)b.n * (size_t)(fb - fa) * A2D_WIN_SLOTWORDS(b.nosc, b.filt);
			atv += (size_t)b.n;
			++c->stats.launches;
		}
		if(two) {
			HIPCHK(c, hipEventRecord(c->win_ev[set], sc));
			HIPCHK(c, hipStreamWaitEvent(c->stream, c->win_ev[set], 0));
		}
		if(wtiming && !two && !c->capturing)
			HIPCHK(c, hipEventRecord(tev[1], c->stream));
		// (one slab, one stream: the batch's other leaf kernels and the speculative pass for the next batch go here, the
		// render passes behind them - issue_kernels)
		if(nslabs == 1 && !wtiming) {
			if(int r = mid())
				return r;
			if(c->vm.spec_go_pending) {	// (the pass first, then the render pass: vm_speculate)
				HIPCHK(c, hipStreamWaitEvent(c->stream, c->vm.spec_go, 0));
				c->vm.spec_go_pending = false;
			}
		}
		at = atw = 0;
		for(int j = 0; j < nj; ++j) {
			const Job &b = jobs[j];
			if(b.spec) {
				// (the whole batch at once, behind the first slab's control passes - the commit among them)
				if(fa == 0 && a2d_launch_win_render(c->sw, c->hparams, b.nosc, b.filt, b.list, b.n, 0, nfrags, c->vm.d_swin[sset].d + b.satw,
						c->vm.d_swext[sset].d, c->vm.d_swidx[sset].d + b.sat, c->stream))
					return c->fail(A2AMD_EHIP, "window render launch failed: %s", hipGetErrorString(hipGetLastError()));
				if(fa == 0)
					++c->stats.launches;
				continue;
			}
			if(a2d_launch_win_render(c->sw, c->hparams, b.nosc, b.filt, b.list, b.n, fa, fb, wslot + atw,
					wext, widx + at, c->stream))
				return c->fail(A2AMD_EHIP, "window render launch failed: %s", hipGetErrorString(hipGetLastError()));
			at += (size_t)b.n * (size_t)(fb - fa);
			atw += (size_t)b.n * (size_t)(fb - fa) * A2D_WIN_SLOTWORDS(b.nosc, b.filt);
			++c->stats.launches;
		}
		if(two)
			HIPCHK(c, hipEventRecord(c->win_ev[2 + set], c->stream));
		if(wtiming && !two && !c->capturing) {
			// (A2AMD_WIN_TIMING=1: the two passes' times per slab on stderr - a measurement aid that waits for the GPU)
			float t_ctl = 0, t_ren = 0;
			HIPCHK(c, hipEventRecord(tev[2], c->stream));
			HIPCHK(c, hipEventSynchronize(tev[2]));
			hipEventElapsedTime(&t_ctl, tev[0], tev[1]);
			hipEventElapsedTime(&t_ren, tev[1], tev[2]);
			fprintf(stderr, "a2amd windows: fragments [%d, %d), %zu voices in %d list(s), %zu records: control pass %.1f us, render pass %.1f us\n",
					fa, fb, nvoices, nj, nrec, t_ctl * 1e3, t_ren * 1e3);
		}
	}
	// The pool's overflow flag (a bound the host got wrong: voices would lose windows) is never left unread: it is
	// copied back behind the batch and looked at before the next one's windows are issued - a batch late, but loud
	// (A2AMD_WIN_CHECK=1, the test suite's setting: at once, with a wait).
	if(!c->capturing && plain_jobs) {
		if(!c->h_wtop) {
			HIPCHK(c, hipHostMalloc((void **)&c->h_wtop, 4 * sizeof(unsigned), hipHostMallocDefault));
			memset(c->h_wtop, 0, 4 * sizeof(unsigned));
			HIPCHK(c, hipEventCreateWithFlags(&c->wtop_ev, hipEventDisableTiming));
		}
		HIPCHK(c, hipMemcpyAsync(c->h_wtop, c->d_wtop, 4 * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(c, hipEventRecord(c->wtop_ev, c->stream));
		c->wtop_pending = true;
	}
	if(c->vm.fused && !c->vm.spec_use)	// (a pass that met a fault is not taken: vm_issue)
		if(int r = vm_fused_done(c))
			return r;
	if(c->sw.win_check && !c->capturing && plain_jobs) {
		unsigned top[4] = { 0, 0, 0, 0 };
		HIPCHK(c, hipMemcpyAsync(top, c->d_wtop, sizeof(top), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(c, hipStreamSynchronize(c->stream));
		if(top[1] || (two && top[3])) {
			if(c->vm.fused)
				c->vm.fused_off = true;
			return c->fail(A2AMD_ESTATE, "window pool overflow (%u / %u of %zu entries)", top[0], top[2], c->d_wext.cap);
		}
	}
	return 0;
}

static void flush_commits(a2amd_ctx *c, A2DCommitSet *pend)
{
	for(int k = 0; k < pend->n; ++k)
		a2d_launch_commit(c->hparams, pend->c[k], c->stream);
	pend->n = 0;
}

// k_leaf_recs over one list of a class
// (a wavefront walks its voices one after the other, fragment by fragment: as many
// wavefronts as the chip holds before a wavefront gets a second voice)
static int launch_recs(a2amd_ctx *c, int nosc, int filt, const int *list, int n, int skip_empty)
{
	if(!n)
		return 0;
	const int vpw = c->sw.rvpw_set ? c->sw.rvpw : (n + 8191) / 8192;
	if(a2d_launch_leaf_recs(c->sw, c->d_params, c->hparams, nosc, filt, list, n, vpw, c->stream, skip_empty))
		return c->fail(A2AMD_EHIP, "leaf records launch failed: %s", hipGetErrorString(hipGetLastError()));
	++c->stats.launches;
	return 0;
}

// k_leaf_oscpan is the batch's only leaf kernel: no voice in any other leaf segment, no exceptions
static bool oscpan_alone(const a2amd_ctx *c)
{
	for(int k = 0; k < LEAF_N; ++k)
		if((c->leaf[k].count != 0) != (k == LEAF_OSCPAN))
			return false;
	return c->dyn[DYN_REST].first + c->dyn[DYN_REST].count == 0;
}

// The batch's leaf kernels other than the window kernels (issue_leaf_phase says when they run): what the block needs of
// its caller, and whether it has run
struct LeafPass {
	A2DCommitSet *pend;	// state commits the time-sliced quiet kernels leave for a later launch
	hipEvent_t e1;
	bool use_win;		// the window kernels render the voices with records (else: the records kernels, here)
	bool solo;		// oscpan_alone()
	bool done;
};

static int launch_leaves(a2amd_ctx *c, LeafPass &lp)
{
	if(lp.done)
		return 0;
	lp.done = true;
	A2DCommitSet &pend = *lp.pend;
	const int *const list = c->d_list.d;
	// A class whose quiet voices are ALL the device VM's, none of them left alone this batch - the speculative pass
	// that was taken for it counted (A2DVmwOut::idle) - has nothing for its quiet kernel to do, and a launch that
	// finds that out voice by voice is 10 us (k_leaf_oscpan + commit) to 80 us (k_leaf_oscfiltpan: sixteen
	// wavefronts per workgroup through the batch's fragments, barriers and all) in front of the next pass
	// (profiles/r06_timeline_before.txt).  The launch classes contain the VM's (every live voice of the class is in
	// the list, classify above): equal counts are equal sets.
	// Not for the filter class: there the 80 us happen to keep the order that is best for it - the render pass onto
	// the CUs first, the next pass behind it (vm_speculate) - and without them the two start together: 16 384 voices,
	// a2_Run(4096) 1 398 -> 1 416 us per buffer, a2_Run(1024) 399 -> 416; with the pass held back behind the render
	// pass instead 1 370 and 408 (profiles/r06_go_skip_ab.txt).  A2AMD_VMSKIP: bit 0 the classes without filter12,
	// bit 1 the one with.
	auto none_quiet = [&](int k, int nleaf) {
		return (c->sw.vmskip & (k == 2 ? 2 : 1)) && c->vm.spec_use && !c->vm.list.empty() && c->vm.n_cls[k] == nleaf && c->vm.spec_idle[k] == 0;
	};
	// e1 right behind the main kernel when it is the only leaf kernel
	// of the batch (lp.solo): "leaf" time is then that kernel alone
	const ListRange oscpan = c->leaf[LEAF_OSCPAN];
	if(oscpan.count && none_quiet(0, oscpan.count)) {
		if(lp.solo && lp.e1)
			HIPCHK(c, hipEventRecord(lp.e1, c->stream));
		++c->vm.quiet_skipped;
	} else if(oscpan.count) {
		int vpw, ysplit;
		pick_fast_shape(c->sw, oscpan.count, c->nfrags, &vpw, &ysplit);
		if(a2d_launch_leaf_oscpan(c->d_params, c->hparams, list + oscpan.first, oscpan.count,
				vpw, ysplit, c->d_ustage.d, c->d_staged.d + oscpan.first, c->stream, lp.solo ? (void *)lp.e1 : nullptr,
				&pend.c[pend.n]))
			return c->fail(A2AMD_EHIP, "fast leaf launch failed: %s", hipGetErrorString(hipGetLastError()));
		if(pend.c[pend.n].nlist)
			++pend.n;
		++c->stats.launches;
		c->vm.last.quiet_launched[0] = 1;	// (a2amd_last_batch_vm)
	}
	// wtosc (noise) -> panmix without records: only a batch with device-seeded windows has such voices (in any other every
	// window of a noise oscillator carries its R_NOISESEED record).  A wavefront keeps its voices for the whole batch - no
	// time slices, the held sample travels - so the voices are spread like k_leaf_fmpan's: one wavefront per SIMD first
	// (1 024), then the lanes fill up.
	// (n_noise_quiet: the voices upload() left without the stand-in run - none, and every voice of the segment has records)
	const ListRange noisepan = c->leaf[LEAF_NOISEPAN];
	if(noisepan.count && !c->noise_st.empty() && c->n_noise_quiet) {
		const int vpw = c->sw.nzvpw_set ? c->sw.nzvpw : (noisepan.count + 1023) / 1024;
		if(a2d_launch_leaf_noisepan(c->d_params, c->hparams, list + noisepan.first, noisepan.count, vpw, c->stream))
			return c->fail(A2AMD_EHIP, "noise leaf launch failed: %s", hipGetErrorString(hipGetLastError()));
		++c->stats.launches;
		c->last_noise.quiet_launched = 1;
	}
	// wtosc (noise) -> filter12 -> panmix without records, likewise.  A workgroup keeps its voices - at most 64, the lanes of
	// its filter wavefront - for the whole batch: spread first (one workgroup per CU, 256), then fill.
	const ListRange noisefilt = c->leaf[LEAF_NOISEFILTPAN];
	if(noisefilt.count && !c->noise_st.empty() && c->n_noise_filt_quiet) {
		const int vpg = c->sw.nzfvpg_set ? c->sw.nzfvpg : (noisefilt.count + 255) / 256;
		if(a2d_launch_leaf_noisefiltpan(c->d_params, c->hparams, list + noisefilt.first, noisefilt.count, vpg, c->stream))
			return c->fail(A2AMD_EHIP, "noise filter leaf launch failed: %s", hipGetErrorString(hipGetLastError()));
		++c->stats.launches;
		c->last_noise_filter.quiet_launched = 1;
	}
	// bare wtosc voices without a run this batch, settled or gliding (upload() counted them: none, and the segment's voices
	// are all the general kernel's - no launch).  A wavefront keeps its voices for the whole batch, as k_leaf_noisepan's
	// does: one wavefront per SIMD first (1 024), then the lanes fill up.  A2AMD_VPW forces the voices per wavefront.
	const ListRange bare = c->leaf[LEAF_OSCBARE];
	if(bare.count && c->n_bare_quiet) {
		const int vpw = std::min(std::max(c->sw.vpw_set ? c->sw.vpw : (bare.count + 1023) / 1024, 1), 64);
		if(a2d_launch_leaf_oscbare(c->d_params, c->hparams, list + bare.first, bare.count, vpw, c->stream))
			return c->fail(A2AMD_EHIP, "bare oscillator leaf launch failed: %s", hipGetErrorString(hipGetLastError()));
		++c->stats.launches;
		c->last_bare.launched = 1;
		c->last_bare.vpw = (uint32_t)vpw;
	}
	// 3 x wtosc-filter12-panmix voices without a run this batch, settled or gliding (upload() counted them: none, and the
	// segment's voices are all the general kernel's - no launch).  A workgroup keeps its voices - at most 64, the lanes of
	// its filter wavefront - for the whole batch, as k_leaf_noisefiltpan's does: spread first (one workgroup per CU, 256),
	// then fill.  A2AMD_F2VPW forces the voices per workgroup.
	auto o3_vpg = [&](int count) { return std::min(std::max(c->sw.f2vpw ? c->sw.f2vpw : (count + 255) / 256, 1), 64); };
	auto o3_launched = [&](auto &info, int count, int vpg) {	// (either launch's info struct)
		++c->stats.launches;
		info.launched = 1;
		info.vpg = (uint32_t)vpg;
		info.workgroups = (uint32_t)((count + vpg - 1) / vpg);
	};
	const ListRange o3f = c->leaf[LEAF_OSC3FILTPAN];
	if(o3f.count && c->n_o3f_quiet) {
		const int vpg = o3_vpg(o3f.count);
		if(a2d_launch_leaf_osc3filtpan(c->d_params, c->hparams, list + o3f.first, o3f.count, vpg, c->stream))
			return c->fail(A2AMD_EHIP, "3-osc filter leaf launch failed: %s", hipGetErrorString(hipGetLastError()));
		o3_launched(c->last_osc3filt, o3f.count, vpg);
	}
	// ... and those of the class whose run is windows only (upload(): dyn[DYN_OSC3WIN]): the windows launch, the same
	// workgroup and the same rule for its size, over this batch's list of them
	const ListRange o3w = c->dyn[DYN_OSC3WIN];
	if(o3w.count) {
		const int vpg = o3_vpg(o3w.count);
		if(a2d_launch_leaf_osc3filtpan_win(c->d_params, c->hparams, c->d_dyn + o3w.first, o3w.count, vpg, c->stream))
			return c->fail(A2AMD_EHIP, "3-osc filter leaf windows launch failed: %s", hipGetErrorString(hipGetLastError()));
		o3_launched(c->last_osc3win, o3w.count, vpg);
	}
	const ListRange osc2pan = c->leaf[LEAF_OSC2PAN];
	if(osc2pan.count && none_quiet(1, osc2pan.count))
		++c->vm.quiet_skipped;
	else if(osc2pan.count) {
		int vpw, ysplit;
		// (its own chunk length; 16 time slices: 2.19 ms against 2.25 with 32 at configs[3], round 3)
		pick_fast_shape(c->sw, osc2pan.count, c->nfrags * A2D_FAST_FCH / A2D_OSC2_FCH, &vpw, &ysplit, 16);
		// (A2AMD_DEBUG bit 16: no voice-major walk, every super-chunk chunk by chunk - A/B and tests)
		const int voice_major = !(c->sw.debug & 16);
		// (... bit 17: that walk stages no level in LDS, every tap is a gather - include/a2amd_osc2lds.h)
		const int lds_taps = !(c->sw.debug & (1 << 17));
		// (... bit 18: no voice takes the fused steps of tame levels - include/a2amd_osc2tame.h)
		const int tame = !(c->sw.debug & (1 << 18));
		// Whole wavefronts of settled, tame voices are k_leaf_osc2tame's, launched in front with the same shape
		// (osc2_pair_wanted; the shape is fixed here so that both launches count the same wavefronts)
		a2d_osc2_shape(&vpw, &ysplit, c->d_ustage.d && c->d_staged.d);
		const bool pair = osc2_pair_wanted(c, c->fragframes, c->nfrags);
		if(pair) {
			if(a2d_launch_leaf_osc2tame(c->d_params, c->hparams, list + osc2pan.first, osc2pan.count, vpw, ysplit, c->d_ustage.d,
					c->d_staged.d + osc2pan.first, c->stream, lds_taps, c->d_tame_count, c->d_osc2_taken.d, c->d_taken_count))
				return c->fail(A2AMD_EHIP, "2-osc tame leaf launch failed: %s", hipGetErrorString(hipGetLastError()));
			++c->stats.launches;
			c->last_osc2quiet.launched = 1;
			c->last_osc2quiet.wavefronts = (uint32_t)((osc2pan.count + vpw - 1) / vpw);
		}
		if(a2d_launch_leaf_osc2pan(c->d_params, c->hparams, list + osc2pan.first, osc2pan.count,
				vpw, ysplit, c->d_ustage.d, c->d_staged.d + osc2pan.first, c->stream, &pend.c[pend.n], voice_major, lds_taps, tame, c->d_tame_count, &ysplit,
				pair ? c->d_osc2_taken.d : nullptr))
			return c->fail(A2AMD_EHIP, "2-osc leaf launch failed: %s", hipGetErrorString(hipGetLastError()));
		// (a2amd_last_batch_osc2(): the launch as it went out; the walks follow from it and the batch's fragment lengths)
		c->last_osc2.launched = 1;
		c->last_osc2.voices = (uint32_t)osc2pan.count;
		c->last_osc2.vpw = (uint32_t)vpw;
		c->last_osc2.ysplit = (uint32_t)ysplit;
		c->last_osc2.voice_major = (uint32_t)voice_major;
		if(pend.c[pend.n].nlist)
			++pend.n;
		++c->stats.launches;
		c->vm.last.quiet_launched[1] = 1;	// (a2amd_last_batch_vm)
	}
	const ListRange oscfilt = c->leaf[LEAF_OSCFILTPAN];
	if(oscfilt.count && none_quiet(2, oscfilt.count))
		++c->vm.quiet_skipped;
	else if(oscfilt.count) {
		// voices per workgroup = lanes of its filter wavefront: all 64 once there
		// are enough voices for a workgroup on every CU (one 16-wavefront workgroup
		// per CU), else spread out (a workgroup takes as long as its filter chain,
		// whatever its voice count)
		const int nf = oscfilt.count;
		int vpw = c->sw.fvpw_set ? c->sw.fvpw : std::min(std::max((nf + 255) / 256, 1), 64);
		if(a2d_launch_leaf_oscfiltpan(c->d_params, c->hparams, list + oscfilt.first, nf, vpw, c->stream))
			return c->fail(A2AMD_EHIP, "filter leaf launch failed: %s", hipGetErrorString(hipGetLastError()));
		++c->stats.launches;
		c->vm.last.quiet_launched[2] = 1;	// (a2amd_last_batch_vm)
	}
	const ListRange o2f = c->leaf[LEAF_OSC2FILTPAN];
	if(o2f.count && c->o2f_quiet) {
		// 2 x wtosc-filter12-panmix without records (round 6).  A workgroup (16 wavefronts, 128 registers: one per CU)
		// takes as long as its filter wavefront's chain whatever its voice count, as long as every oscillator
		// wavefront stays in its all-settled loop (a2d_osc2filtpan_max_vpg voices): the voices are dealt over the
		// fewest whole rounds of 256 workgroups that allows (16 384 voices: 2 rounds of 32 - measured 1.09 ms per 256
		// fragments against 3.83 with 48 and 1.50 with 64 voices per workgroup)
		const int nf = o2f.count;
		const int maxv = a2d_osc2filtpan_max_vpg();
		const int rounds = std::max(1, (nf + 256 * maxv - 1) / (256 * maxv));
		const int vpg = c->sw.f2vpw ? c->sw.f2vpw : std::min(std::max((nf + 256 * rounds - 1) / (256 * rounds), 1), maxv);
		if(a2d_launch_leaf_osc2filtpan(c->d_params, c->hparams, list + o2f.first, nf, vpg, c->stream))
			return c->fail(A2AMD_EHIP, "2-osc filter leaf launch failed: %s", hipGetErrorString(hipGetLastError()));
		++c->stats.launches;
		c->last_batch.o2f_launched = 1;
		c->last_batch.o2f_voices = (uint32_t)nf;
		c->last_batch.o2f_max_vpg = (uint32_t)maxv;
		c->last_batch.o2f_vpg = (uint32_t)std::min(std::max(vpg, 1), 64);	// (the launcher's clamp: a filter wavefront's lanes)
	}
	const ListRange fm = c->leaf[LEAF_FMPAN];
	int fm_kinds = 0;
	for(int k = 0; k < 8; ++k)
		fm_kinds += c->fm_kind_count[k] != 0;
	if(fm_kinds > 1 && fm.count <= 16384 && !c->sw.fmvpw_set) {
		// several kinds, few voices: one launch for all of them (the
		// per-kind launches below would run back to back, each as long
		// as a voice's serial chain)
		if(a2d_launch_leaf_fmpan_all(c->d_params, c->hparams, list + fm.first, c->fm_kind_count, (fm.count + 1023) / 1024, c->stream))
			return c->fail(A2AMD_EHIP, "fm leaf launch failed: %s", hipGetErrorString(hipGetLastError()));
		++c->stats.launches;
	} else {
		for(int k = 0, at = fm.first; k < 8; at += c->fm_kind_count[k++]) {
			const int n = c->fm_kind_count[k];
			if(!n)
				continue;
			// A voice is a serial recurrence: a launch takes as long as its longest
			// lane, so few voices are spread over many wavefronts (idle lanes of a
			// wavefront shadow its voices, see fmpan_body) until there is one
			// wavefront per SIMD (1 024), then the lanes fill up
			// (profiles/r01_fm_vpw_sweep.txt).
			int vpw = c->sw.fmvpw_set ? c->sw.fmvpw : (n + 1023) / 1024;
			vpw = std::min(std::max(vpw, 1), 64);
			if(a2d_launch_leaf_fmpan(c->d_params, c->hparams, A2AMD_FM1 + k, list + at, n, vpw, c->stream))
				return c->fail(A2AMD_EHIP, "fm leaf launch failed: %s", hipGetErrorString(hipGetLastError()));
			++c->stats.launches;
		}
	}
	const ListRange gen = c->leaf[LEAF_GENERIC];
	if(gen.count) {
		if(a2d_launch_voices(c->d_params, list + gen.first, gen.count, pick_vpw(gen.count), c->stream))
			return c->fail(A2AMD_EHIP, "leaf launch failed: %s", hipGetErrorString(hipGetLastError()));
		++c->stats.launches;
	}
	if(!lp.use_win) {
		// the records kernels: the four host-made lists ...
		// (the fourth list: this batch's record-carrying 2 x wtosc-filter12-panmix voices and the device VM's voices of that
		// class, taken with skip_empty - upload())
		static const int nosc[4] = { 1, 2, 1, 2 }, filt[4] = { 0, 0, 1, 1 };
		const int *lists[4];
		int counts[4], total = 0, kinds = 0;
		for(int k = 0; k < 4; ++k) {
			lists[k] = c->d_dyn + c->dyn[k].first;
			counts[k] = c->dyn[k].count;
			total += counts[k];
			kinds += counts[k] != 0;
		}
		c->last_batch.recs_voices = (uint32_t)total;
		if(!c->vm.list.empty())
			c->last_batch.recs_voices += (uint32_t)(c->vm.n_cls[0] + c->vm.n_cls[1] + c->vm.n_cls[2]);
		if(kinds > 1 && total <= 4096 && !c->sw.rvpw_set) {
			// few voices of several kinds (a song): one launch - on one stream the per-kind
			// launches would run back to back, each as long as one voice's walk through the batch
			if(a2d_launch_leaf_recs_all(c->sw, c->d_params, c->hparams, lists, counts, 1, c->stream, c->o2f_quiet ? 8 : 0))
				return c->fail(A2AMD_EHIP, "leaf records launch failed: %s", hipGetErrorString(hipGetLastError()));
			++c->stats.launches;
		} else {
			for(int k = 0; k < 4; ++k)
				if(int r = launch_recs(c, nosc[k], filt[k], lists[k], counts[k], k == DYN_FILT2 && c->o2f_quiet))
					return r;
		}
		// ... and the voices whose records the device VM has just written, by class (those it
		// left without records this batch were rendered by their quiet kernels above)
		if(!c->vm.list.empty()) {
			const int *l = c->vm.d_list.d + c->vm.list.size();
			for(int k = 0; k < 3; l += c->vm.n_cls[k++])
				if(int r = launch_recs(c, nosc[k], filt[k], l, c->vm.n_cls[k], 1))
					return r;
		}
	}
	const ListRange rest = c->dyn[DYN_REST];
	if(rest.count > 0) {
		if(a2d_launch_voices(c->d_params, c->d_dyn + rest.first, rest.count, pick_vpw(rest.count), c->stream))
			return c->fail(A2AMD_EHIP, "leaf launch failed: %s", hipGetErrorString(hipGetLastError()));
		++c->stats.launches;
	}
	return 0;
}

// The SUBTREES phase from its start (not: resumed behind insert clients) up to the bus owners: the buses cleared, the
// device VM, the leaf kernels
static int issue_leaf_phase(a2amd_ctx *c, bool consume, bool consume_sub, hipEvent_t e0, hipEvent_t e1, A2DCommitSet *pend)
{
	// (a graph of a self-cleaning batch holds no memset: whoever launches it
	// clears the buses first if they are not known to be clean, ensure_clean())
	const bool selfclean = consume || consume_sub;
	if(c->capturing ? !selfclean : !(selfclean && c->others_clean && c->root_clean))
		HIPCHK(c, hipMemsetAsync(c->d_busmem.d, 0, c->bus_used * sizeof(int32_t), c->stream));
	c->others_clean = selfclean;
	c->root_clean = consume;
	if(e0)
		HIPCHK(c, hipEventRecord(e0, c->stream));
	// the scripted voices the device runs itself: their VMs first - the records of this batch,
	// runs[] pointing at them (a2amd_vm.cpp / a2amd_vm.hip) - then the kernels as for host records
	// The voices that carry records this batch: the 2 x wtosc-filter12-panmix leaves, with and without
	// records, and - of the classes that have quiet kernels of their own - this batch's voices with records.
	// Round 5: the record stream resolved by a lane = voice control pass, the windows rendered
	// from closed-form entries (a2amd_win.hip).  A2AMD_WIN=0: k_leaf_recs, the kernels of rounds
	// 2-4 that interpret the records on the scalar unit of the rendering wavefront (A/B).
	// Which one: the window kernels' two passes are each as long as ONE voice's walk through the batch (the
	// control pass) / one filter chain (the render pass) whatever the voice count - 0.4 to 1 ms per 64 fragments -
	// where k_leaf_recs, one wavefront per voice, takes 0.3 ms for a song's few dozen voices and 0.4 - 0.7 ms for a
	// thousand; from a few thousand voices on it is k_leaf_recs that queues up (16 384: 1.1 - 3.9 ms against
	// 0.5 - 1.8).  A2AMD_WIN=0 / 1 forces (the parity tests run both), A2AMD_WIN_MIN moves the threshold.
	bool use_win;
	{
		int nwinv = 0;
		for(int k = DYN_OSC1; k <= DYN_FILT2; ++k)
			nwinv += c->dyn[k].count;
		for(int k = 0; k < 3; ++k)
			nwinv += c->vm.list.empty() ? 0 : c->vm.n_cls[k];
		use_win = c->sw.win >= 0 ? c->sw.win != 0 : nwinv >= c->sw.win_min;
	}
	// (A2AMD_VMWIN=0: the device VM's voices through records - k_vm_count / k_vm_emit - whatever renders them)
	const bool vmwin_ok = c->sw.vmwin;
	if(int r = vm_issue(c, use_win && vmwin_ok && !c->vm.fused_off))
		return r;
	// a2amd_last_batch(): the lists as upload() made them; the launches below fill in the rest
	c->last_batch = a2amd_batch_info{};
	c->last_batch.o2f_class = (uint32_t)c->leaf[LEAF_OSC2FILTPAN].count;
	c->last_batch.o2f_listed = (uint32_t)c->dyn[DYN_FILT2].count;
	c->last_batch.n_moving_listed = (uint32_t)c->n_moving_listed;
	c->last_batch.general_voices = (uint32_t)c->dyn[DYN_REST].count;
	c->last_noise = a2amd_noise_batch_info{};
	c->last_noise.class_voices = (uint32_t)c->leaf[LEAF_NOISEPAN].count;
	c->last_noise.standin_voices = c->n_noise_standin;
	c->last_noise.quiet_voices = c->n_noise_quiet;
	c->last_noise_filter = a2amd_noise_filter_batch_info{};
	c->last_noise_filter.class_voices = (uint32_t)c->leaf[LEAF_NOISEFILTPAN].count;
	c->last_noise_filter.quiet_voices = c->n_noise_filt_quiet;
	c->last_noise_filter.min_voices = (uint32_t)c->sw.nzf_min;
	c->last_bare = a2amd_bare_batch_info{};
	c->last_bare.class_voices = (uint32_t)c->leaf[LEAF_OSCBARE].count;
	c->last_bare.quiet_voices = c->n_bare_quiet;
	c->last_bare.gliding_voices = c->n_bare_gliding;
	c->last_bare.record_voices = c->n_bare_records;
	c->last_bare.mono_drivers = c->n_mono_drivers;
	c->last_osc3filt = a2amd_osc3filt_batch_info{};
	c->last_osc3filt.class_voices = (uint32_t)c->leaf[LEAF_OSC3FILTPAN].count;
	c->last_osc3filt.quiet_voices = c->n_o3f_quiet;
	c->last_osc3filt.gliding_voices = c->n_o3f_gliding;
	c->last_osc3filt.record_voices = c->n_o3f_records;
	c->last_osc2 = a2amd_osc2_batch_info{};
	c->last_osc2quiet = a2amd_osc2quiet_batch_info{};
	// The batch's other leaf kernels - the quiet kernels of the classes, the records kernels where the window kernels
	// are not in use, the general kernel - as a block that runs once: normally behind the window kernels, and
	// (round 6) from INSIDE issue_windows, between its control passes and its render passes, when a speculative VM
	// pass is to follow: that pass may start as soon as the control passes (k_vm_win / k_vm_commit: the stepped state
	// of the VM voices that are live this batch) and the quiet kernels (the phases of those that are idle) are done,
	// and then has the render pass - the long one - beside it, not in front of it.  All of these kernels only ever
	// ADD to the buses, and runs[] is written by the control passes: their order among themselves is free.
	LeafPass lp = { pend, e1, use_win, oscpan_alone(c), false };
	const std::function<int()> mid = [&]() -> int {
		if(!c->sw.vmspec_early || !vmwin_ok || !vm_spec_wanted(c))
			return 0;	// (no pass to follow: the old order)
		if(int r = launch_leaves(c, lp))
			return r;
		// (a time-sliced quiet kernel leaves its voices' end state in the staging array until a commit that rides
		// along with a later launch: the pass reads the unit state of the class voices that were idle this batch)
		flush_commits(c, pend);
		return vm_speculate(c);
	};
	// ... the window kernels first: k_vm_win says in runs[] which of the VM's voices are the quiet kernels' this batch
	if(use_win) {
		if(int r = issue_windows(c, c->d_dyn, c->dyn, mid))
			return r;
		if(vmwin_ok)
			if(int r = vm_predict(c))
				return r;
	}
	if(int r = launch_leaves(c, lp))
		return r;
	if(e1 && !lp.solo)
		HIPCHK(c, hipEventRecord(e1, c->stream));
	// Round 6: behind the leaf kernels (the quiet ones have moved the phases of the VM voices that were idle this
	// batch), on a stream of its own beside the bus kernels, the readback and the engine thread's next walk:
	// the class voices' VM + control pass for the batch expected next (vm_speculate, a2amd_vm.cpp)
	if(use_win && vmwin_ok && !c->vm.spec_launched_now && vm_spec_wanted(c)) {
		flush_commits(c, pend);	// (see mid(): the pass reads what the quiet kernels have staged)
		if(int r = vm_speculate(c))
			return r;
	}
	vm_note_batch(c, use_win && vmwin_ok);
	return 0;
}

// the kernels of one batch, in stream order; e* may be null
int issue_kernels(a2amd_ctx *c, unsigned phases, hipEvent_t e0, hipEvent_t e1, hipEvent_t e2)
{
	// (self-cleaning buses need both phases in one go: the root's bus is read in ROOT)
	const bool has_sub = (phases & A2AMD_RENDER_SUBTREES) != 0, has_root = (phases & A2AMD_RENDER_ROOT) != 0;
	const bool consume = c->consume_ok && has_sub && has_root;
	// Split phases (multi-GPU steps): the group buses are read - and zeroed - in the
	// SUBTREES phase; the root's bus by the ROOT phase on the rank that runs it, or
	// by a2amd_rootbus_copy() when the partials are parked (shard.GroupedRootReduce).
	const bool consume_sub = c->consume_ok && has_sub && !has_root;
	A2DCommitSet pend;
	pend.n = 0;
	pend.c[0].nlist = pend.c[1].nlist = 0;
	if(phases & A2AMD_RENDER_SUBTREES) {
		if(c->sub_resume < 0)
			if(int r = issue_leaf_phase(c, consume, consume_sub, e0, e1, &pend))
				return r;
		// the voices that own a bus, deepest first.  With A2AMD_RENDER_TAPS the walk stops behind a
		// depth that holds a muted xinsert (insert clients: a2amd_unit_insertable): the host serves
		// them and calls again.
		const int dstart = c->sub_resume >= 0 ? c->sub_resume : (int)c->depth_ranges.size() - 1;
		c->sub_resume = -1;
		c->paused_at = 0;
		for(int d = dstart; d >= 1; --d) {
			if(int r = launch_depth(c, d, consume ? 3 : consume_sub ? 1 : 0, &pend))
				return r;
			if((phases & A2AMD_RENDER_TAPS) && depth_has_mutes(c, d)) {
				c->paused_at = d;
				c->sub_resume = d > 1 ? d - 1 : -1;
				break;
			}
		}
		// (the ROOT phase may run elsewhere, or later: nothing stays pending across calls)
		if(!(phases & A2AMD_RENDER_ROOT))
			flush_commits(c, &pend);
	}
	if(phases & A2AMD_RENDER_ROOT) {
		// The root chain adds into the master bus.  When its phase runs on its own
		// (multi-GPU steps: several SUBTREES phases may have gone by since the
		// last one, audiality2_amd/shard.py) the master bus is cleared here.
		// (... unless the root is a plain driver chain: then it stores the master bus)
		const bool root_stores = consume || c->consume_ok;
		if(!has_sub && !root_stores)
			HIPCHK(c, hipMemsetAsync(c->d_busmem.d, 0,
					(size_t)c->nfrags * c->cfg.channels * A2D_FRAG * sizeof(int32_t), c->stream));
		// (on its own the phase also leaves the root's bus zeroed behind it)
		if(!c->depth_ranges.empty())
			if(int r = launch_depth(c, 0, root_stores ? 3 : 0, &pend))
				return r;
		if(!has_sub && root_stores)
			c->root_clean = true;
		flush_commits(c, &pend);
		if(e2)
			HIPCHK(c, hipEventRecord(e2, c->stream));
		c->stats.fragments += c->nfrags;
		c->stats.voice_fragments += (uint64_t)c->nfrags * (uint64_t)c->list_all.size();
	}
	return 0;
}

void drop_graphs(a2amd_ctx *c)
{
	for(int i = 0; i < 12; ++i) {
		if(c->gexec[i]) {
			hipGraphExecDestroy(c->gexec[i]);
			c->gexec[i] = nullptr;
		}
		if(c->graph[i]) {
			hipGraphDestroy(c->graph[i]);
			c->graph[i] = nullptr;
		}
	}
}

// before a graph of a self-cleaning batch (it holds no memset) is launched
int ensure_clean(a2amd_ctx *c)
{
	if(c->consume_ok && !(c->others_clean && c->root_clean)) {
		HIPCHK(c, hipMemsetAsync(c->d_busmem.d, 0, c->bus_used * sizeof(int32_t), c->stream));
		c->others_clean = c->root_clean = true;
	}
	return 0;
}

// capture 'steps' consecutive runs of the uploaded batch into one graph
int build_graph(a2amd_ctx *c, int slot, int steps, unsigned phases)
{
	if(c->gexec[slot]) {		// (built for another destination of the master bus)
		hipGraphExecDestroy(c->gexec[slot]);
		c->gexec[slot] = nullptr;
	}
	if(c->graph[slot]) {
		hipGraphDestroy(c->graph[slot]);
		c->graph[slot] = nullptr;
	}
	hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
	if(e != hipSuccess)
		return c->fail(A2AMD_EHIP, "hipStreamBeginCapture: %s", hipGetErrorString(e));
	int r = 0;
	// (a captured run does not happen now: every graph starts from buses of
	// unknown state, and what it leaves behind is noted when it is launched)
	const bool oc = c->others_clean, rc = c->root_clean;
	c->master_direct = false;
	c->capturing = true;
	for(int i = 0; i < steps && !r; ++i)
		r = issue_kernels(c, phases, nullptr, nullptr, nullptr);
	c->capturing = false;
	c->others_clean = oc;
	c->root_clean = rc;
	e = hipStreamEndCapture(c->stream, &c->graph[slot]);
	if(r)
		return r;
	if(e != hipSuccess)
		return c->fail(A2AMD_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
	e = hipGraphInstantiate(&c->gexec[slot], c->graph[slot], nullptr, nullptr, 0);
	if(e != hipSuccess)
		return c->fail(A2AMD_EHIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
	c->gdst[slot] = c->master_dst;
	c->gdirect[slot] = c->master_direct;
	c->gconsume[slot] = c->last_bus.consume;
	return 0;
}

} // namespace a2h
