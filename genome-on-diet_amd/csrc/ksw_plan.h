// The planner of a batch of ksw_extd2 alignments: which kernel takes each one, the layout of the backtrace arena, the order and grouping
// of the id lists the kernels are launched over.  Host arithmetic only -- no device call, no environment, no context -- so that
// tests/emul/dp_plan_test.cpp can run it on the CPU; the caller (gd_ksw_batch_dev) uploads and launches what it returns.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <unordered_map>
#include <vector>
#include "ksw_common.h"
#include "ksw_wave_core.h"
#include "ksw_pipe_core.h"

// number of cells the generic kernel's LDS ring must hold for this geometry (see the generic kernel)
static int gd_generic_cap(int qlen, int tlen, int w)
{
	if (w < 0) w = tlen > qlen ? tlen : qlen;
	int n = std::min(std::min(qlen, tlen), w + 1);
	int need = n + 64, cap = 256;
	while (cap < need) cap <<= 1;
	return cap;
}

static inline size_t gd_align256(size_t x) { return (x + 255) & ~(size_t)255; }

// what the planner takes from the context and the environment of its caller
struct GdPlanOpt {
	int kernel_mode = 0;          // 0: by geometry, 1: every alignment on the generic kernel, 2: wave kernels only (anything else is an error)
	bool wave_scoring_ok = true;  // gd_wave_scoring_ok of the batch's scoring
	bool single_affine = false;   // the single-affine kernel forms run (and q == q2, e == e2): no checkpointed wide-band form
	int wide_ckpt = -1;           // 1 / 0 force / forbid the checkpointed wide-band kernel, default by batch size
	int wave_slots = 5120;        // wavefront slots of the 64-lane DP kernel on the device
	bool lane = false;            // the context is a lane of one with batches in flight: longer pipelines (see np below)
	int group_lanes = 0;          // 16: always four alignments per wavefront
	bool use_pipe = true;         // false: no skewed pipelines, short alignments on the grouped kernels only
	// The compact arena.  true: the launch offers the narrow band with the fused walk (the condition under which the 64-lane kernel looks at
	// the mark), so a GD_NARROW_TRY box gets a slot for the half-block rows only and claims full-band rows if its certificate fails at both
	// rungs (GDIET_BT_COMPACT=0 and a context with the narrow band off: false, every slot is sized for the full-band rows)
	bool compact = false;
	int64_t overflow_bytes = -1;  // size of the overflow pool behind the last slot; < 0: GD_POOL_SHARE of the slots' total (GDIET_BT_OVERFLOW_MB)
};
// the overflow pool's default share of the compact total: about 16 of the 9 400 boxes of a HiFi batch of 5 120 reads need their full-band
// rows (profiles/r06_quarter_band.md); a sixteenth of the arena holds a few hundred such boxes
#define GD_POOL_DIV 16
#define GD_POOL_MIN (64 << 20) // ... but at least 64 MiB, or all the full-size slots together if that is less
// bytes per anti-diagonal a GD_NARROW_TRY box's slot holds in the compact layout: the half-block rows (the quarter-block rows use its first half)
#define GD_COMPACT_ROW 512

// decide kernel + backtrace geometry of one alignment
static void gd_plan_one(const GdPlanOpt &O, int qlen, int tlen, int w, int32_t &kind, int32_t &row_bytes)
{
	const int ncol = gd_ncol16(qlen, tlen, w);
	kind = GD_KIND_GENERIC, row_bytes = ncol * 16;
	if (O.kernel_mode == 1 || !O.wave_scoring_ok) return;
	if (gd_wave_supported(qlen, tlen, w, 64)) {
		if (gd_wave_supported(qlen, tlen, w, 16)) {
			// short alignments: several per wavefront.  Targets of <= 128 / 160 bases keep every block in a lane of its own: groups of
			// 8 / 10 lanes (8 / 6 alignments per wavefront) instead of one DPP row of 16 each
			// (the reference's n_col_ counts one block more -- the spill of the score row above the window -- but beyond the target's
			// last block that spill is never read)
			const int g = O.group_lanes == 16 ? 16 : tlen <= 128 ? 8 : tlen <= 160 ? 10 : 16;
			kind = GD_KIND_WAVE16, row_bytes = g * 16;
		}
		else if (O.use_pipe && gd_pipe_geometry_ok(qlen, tlen, w)) kind = GD_KIND_WAVE16, row_bytes = 16 * 16; // 241..256 bases, full matrix: one block more than the 16-lane groups hold -- the pipelines take it (every run, however short)
		else kind = GD_KIND_WAVE64, row_bytes = 64 * 16;
	} else if (gd_wave_supported(qlen, tlen, w, 128)) kind = GD_KIND_WAVE128; // row_bytes stays n_col_*16
}

// The plan of one batch.  The context keeps one and reuses its vectors from batch to batch.
struct GdPlan {
	int err = 0;                   // 0, or the first of: 1 empty sequence, 2 no wave kernel takes an alignment (kernel_mode 2), 4 band beyond the generic kernel's LDS window
	int mask = 0;                  // kernels of the batch: 1 64-lane, 2 generic, 4 short-alignment, 8 wide-band, 16 pipelines
	uint64_t cells = 0, alg_bytes = 0; // roofline accounting
	int max_cap = 0;               // largest gd_generic_cap of the generic kernel's alignments
	size_t bt = 0;                 // bytes of backtrace arena
	// the compact layout (GdPlanOpt::compact, and the batch has GD_NARROW_TRY boxes; else pool_bytes = n_drain = 0 and n_compact = 0):
	// [pool_off, pool_off + pool_bytes) behind the last slot is the overflow pool, bt their sum; n_drain launches of the 64-lane kernel
	// behind the main one serve every box that found no room there, whatever the order of the claims (gd_drain_launches) -- the worst
	// case, for which the claim counters are allocated; a caller that knows how many boxes are pending enqueues gd_drain_rounds of them
	size_t pool_off = 0, pool_bytes = 0, n_compact = 0, full_total = 0, full_max = 0; // n_compact boxes with a half-size slot; their full-size slots in all, the largest
	int n_drain = 0;
	bool wide_ck = false;         // the wide-band alignments run checkpointed ...
	size_t n_ring96 = 0;           // ... and the first n_ring96 of their list on the 96-block ring
	// the id lists of the four kinds back to back, ids[id_off[k]] the first of kind k (n_kind[k] alignments).  Inside the short-alignment
	// kind: three lists of groups of 4 / 6 / 8 ids (16 / 10 / 8 lanes; n_group[g] entries from group_off[g], -1 pads a group), then the
	// n_pipe_ids ids of the pipeline runs
	std::vector<int32_t> ids;
	size_t id_off[4] = {0, 0, 0, 0}, n_kind[4] = {0, 0, 0, 0}, group_off[3] = {0, 0, 0}, n_group[3] = {0, 0, 0}, n_pipe_ids = 0;
	std::vector<PipeWave> pipes;
	std::vector<PipeRun> pipe_runs;
};

// How many launches whose claims go to `arena` bytes serve n_boxes boxes that need full_total bytes of full-size slots in all (each a
// multiple of 256, the largest full_max), in whatever order the claims arrive.  A claim is one atomic add on the launch's counter and is
// served iff the counter, before and after, is inside the arena: a launch serves the claims in the order of their arrival up to the first
// that does not fit -- at least one box (arena >= full_max), and more than arena - full_max bytes unless it serves all that are left.
// -1: the arena is smaller than the largest slot.
static inline int gd_drain_launches(size_t n_boxes, size_t full_total, size_t full_max, size_t arena)
{
	if (n_boxes == 0) return 0;
	if (arena < full_max) return -1;
	const size_t per = arena - full_max + 256;
	return (int)std::min(n_boxes, (full_total + per - 1) / per);
}

// The drain launches over a PENDING LIST (ksw_wave.hip.h): n_pending boxes of the batch found no room in the overflow pool.  All the host
// knows of them when it decides is how many they are and what the planner summed over every box that could have been among them
// (full_total, full_max), so it bounds their bytes by both: n_pending boxes need at most min(full_total, n_pending * full_max).
// gd_drain_launches of that set is the number of rounds -- 0 for an empty list, never more than the planner's n_drain for the whole
// batch (the bound grows with the count and with the bytes), so the claim counters the batch allocated suffice.
struct GdDrainSet { size_t n_pending, full_total, full_max; };
static inline int gd_drain_rounds(const GdDrainSet &S, size_t arena)
{
	return gd_drain_launches(S.n_pending, std::min(S.full_total, S.n_pending * S.full_max), S.full_max, arena);
}
// The claims of those rounds, replayed: the boxes arrive in the order of `units` (their full-size slots in units of 256 bytes) in every
// round, each adds its size to the round's counter, and the ones gd_claim_fits admits -- the kernel's own test -- have their rows at
// the counter's old value; the others go on to the next round.  round[i] (1-based; 0: not served within n_rounds) and off_units[i] of
// every box; returns the number of boxes left without rows, which gd_drain_rounds rules out.  tests/emul/drain_rounds_test.cpp checks
// that against brute force for whatever order the boxes arrive in.
static inline size_t gd_drain_replay(const std::vector<uint32_t> &units, size_t arena, int n_rounds, std::vector<int32_t> &round, std::vector<uint32_t> &off_units)
{
	round.assign(units.size(), 0), off_units.assign(units.size(), 0);
	size_t left = units.size();
	for (int k = 1; k <= n_rounds && left; ++k) {
		uint32_t counter = 0; // (the device's is 32 bits wide as well: every box of a batch together stays below 2^32 units)
		for (size_t i = 0; i < units.size(); ++i) {
			if (round[i]) continue;
			const uint32_t at = counter;
			counter += units[i];
			if (gd_claim_fits(at, units[i], (int64_t)(arena >> 8))) round[i] = k, off_units[i] = at, --left;
		}
	}
	return left;
}

// Fills tasks[0..n) and P.  run_slices(n_sl, f) calls f(sl) for every sl in [0, n_sl), in any order and on any threads; mark(name) is
// told when a step is done (the caller's stage trace).  With P.err set, only err, mask and the tasks' own fields are defined.
template <class RunSlices, class Mark>
static void gd_plan_batch(GdPlan &P, const GdPlanOpt &O, int n, const int64_t *h_qoff, const int64_t *h_toff, const int32_t *h_w, const int64_t *h_cig,
                          const int32_t *h_ex /* exact-match scores, or nullptr */, KswTask *h_tasks, RunSlices &&run_slices, Mark &&mark)
{
	size_t bt = 0;
	uint64_t cells_sum = 0, alg_sum = 0;
	std::vector<int32_t> ids[4];
	int max_cap = 0;
	P.err = 0, P.mask = 0;
	// kernel + backtrace geometry of every alignment first, on the host threads: the admission test of the wave kernels walks the blocks
	// of the band (~1 000 steps for a 15 kbp alignment: 4-5 ms for the 9 400 alignments of a HiFi batch on one thread -- time that sat
	// between the gather kernel and the DP kernel whenever a batch was not ready early).  Slices with a memo each: a short-read
	// batch repeats a few geometries.
	// (the same pass fills every other field of the descriptor, checks it, adds up the roofline accounting and lists the alignments by
	// kind -- per slice, joined in slice order afterwards: done by one thread this was 3-5 ms per 262 144 short alignments, most of a
	// short-read batch's planning)
	struct PlanSlice { uint64_t cells = 0, alg = 0; int max_cap = 0, err = 0; uint32_t mask = 0; std::vector<int32_t> ids[4]; };
	const int n_sl = std::max(1, std::min(64, n / 256));
	std::vector<PlanSlice> slices((size_t)n_sl);
	{
		run_slices(n_sl, [&](int sl) {
			struct { int qlen = -1, tlen = -1, w = 0; int32_t kind = 0, row_bytes = 0, narrow = 0; } memo;
			PlanSlice &S = slices[sl];
			const int i0 = (int)((int64_t)n * sl / n_sl), i1 = (int)((int64_t)n * (sl + 1) / n_sl);
			for (int k = 0; k < 4; ++k) S.ids[k].reserve((size_t)(i1 - i0));
			for (int i = i0; i < i1; ++i) {
				KswTask &T = h_tasks[i];
				T.qlen = (int)(h_qoff[i + 1] - h_qoff[i]), T.tlen = (int)(h_toff[i + 1] - h_toff[i]), T.w = h_w[i];
				T.kind = GD_KIND_GENERIC, T.row_bytes = 0;
				T.qoff = h_qoff[i], T.toff = h_toff[i];
				T.cig_off = h_cig[i], T.cig_cap = (int32_t)std::min<int64_t>(h_cig[i + 1] - h_cig[i], 0x7fffffff);
				T.exact_score = h_ex ? h_ex[i] : GD_NEG_INF;
				T.pad = 0, T.bt_off = 0;
				if (T.qlen <= 0 || T.tlen <= 0) { S.err |= 1; continue; } // (refused below)
				if (T.qlen == memo.qlen && T.tlen == memo.tlen && T.w == memo.w) T.kind = memo.kind, T.row_bytes = memo.row_bytes, T.pad = memo.narrow;
				else {
					gd_plan_one(O, T.qlen, T.tlen, T.w, T.kind, T.row_bytes);
					// the 64-lane kernel's boxes that try the band GD_W_NARROW first, or run their own narrow band on the half-block rows (the
					// kernel's argument decides whether it looks at the mark; O.compact says so here, and sizes the slot below)
					T.pad = T.kind == GD_KIND_WAVE64 && !O.single_affine ? gd_narrow_mode(T.qlen, T.tlen, T.w) : GD_NARROW_NO;
					memo.qlen = T.qlen, memo.tlen = T.tlen, memo.w = T.w, memo.kind = T.kind, memo.row_bytes = T.row_bytes, memo.narrow = T.pad;
				}
				if (O.kernel_mode == 2 && T.kind == GD_KIND_GENERIC) S.err |= 2;
				if (T.kind == GD_KIND_GENERIC) {
					const int cap = gd_generic_cap(T.qlen, T.tlen, T.w);
					if (cap * 7 > 160 * 1024 - 1024) S.err |= 4;
					S.max_cap = std::max(S.max_cap, cap);
				}
				{ // accounting for the roofline: SURVEY.md 8d's per-alignment figure
					const uint64_t wb = (uint64_t)(T.w < 0 ? std::max(T.qlen, T.tlen) : T.w) + 1;
					const uint64_t band = std::min<uint64_t>(wb, (uint64_t)std::min(T.qlen, T.tlen));
					const uint64_t cells = (uint64_t)(T.qlen + T.tlen - 1) * band;
					S.cells += cells;
					S.alg += cells + (uint64_t)(T.qlen + T.tlen) + (uint64_t)T.qlen + (uint64_t)(T.tlen + 1) / 2;
				}
				S.ids[T.kind].push_back(i);
				S.mask |= T.kind == GD_KIND_GENERIC ? 2 : T.kind == GD_KIND_WAVE16 ? 4 : T.kind == GD_KIND_WAVE128 ? 8 : 1;
			}
		});
	}
	mark("kinds");
	{
		int err = 0;
		size_t cnt[4] = {0, 0, 0, 0};
		for (const PlanSlice &S : slices) {
			err |= S.err, cells_sum += S.cells, alg_sum += S.alg, max_cap = std::max(max_cap, S.max_cap), P.mask |= (int)S.mask;
			for (int k = 0; k < 4; ++k) cnt[k] += S.ids[k].size();
		}
		// (the first failure in the order the sequential form reported them)
		if (err) { P.err = err & 1 ? 1 : err & 2 ? 2 : 4; return; }
		for (int k = 0; k < 4; ++k) {
			ids[k].resize(cnt[k]);
			size_t at = 0;
			for (const PlanSlice &S : slices) {
				if (!S.ids[k].empty()) memcpy(ids[k].data() + at, S.ids[k].data(), S.ids[k].size() * sizeof(int32_t));
				at += S.ids[k].size();
			}
		}
	}
	mark("fields");
	bool wide_ck = false;
	if (!ids[GD_KIND_WAVE128].empty() && !O.single_affine) {
		size_t full = 0;
		for (int32_t id : ids[GD_KIND_WAVE128]) full += (size_t)(h_tasks[id].qlen + h_tasks[id].tlen - 1) * (size_t)h_tasks[id].row_bytes;
		wide_ck = O.wide_ckpt == 1 || (O.wide_ckpt < 0 && ((int)ids[GD_KIND_WAVE128].size() >= O.wave_slots / 5 || full > ((size_t)100 << 30)));
	}
	P.pool_off = P.pool_bytes = P.n_compact = P.full_total = P.full_max = 0, P.n_drain = 0;
	for (int i = 0; i < n; ++i) {
		KswTask &T = h_tasks[i];
		T.bt_off = (int64_t)bt;
		const size_t full = gd_align256((size_t)(T.qlen + T.tlen - 1) * (size_t)T.row_bytes + 64);
		if (wide_ck && T.kind == GD_KIND_WAVE128) bt += gd_align256(gd_ck_bytes(T.qlen, T.tlen, T.row_bytes) + 64);
		else if (O.compact && T.kind == GD_KIND_WAVE64 && T.pad == GD_NARROW_TRY) {
			bt += gd_align256((size_t)(T.qlen + T.tlen - 1) * GD_COMPACT_ROW + 64);
			++P.n_compact, P.full_total += full, P.full_max = std::max(P.full_max, full);
		} else bt += full;
	}
	if (P.n_compact) {
		P.pool_off = bt;
		// (the floor: in a batch of a few dozen boxes a sixteenth of the slots holds not one full-size box, and a lone fall-back served by
		// a drain launch is a second serial alignment behind the first -- nothing the arena of such a batch needs to save)
		P.pool_bytes = O.overflow_bytes >= 0 ? gd_align256((size_t)O.overflow_bytes) : std::max(gd_align256(bt / GD_POOL_DIV), std::min(P.full_total, (size_t)GD_POOL_MIN));
		if (P.pool_off + P.pool_bytes < P.full_max) P.pool_bytes = P.full_max - P.pool_off; // (a batch of one or two boxes: the drain launches need room for the largest)
		bt += P.pool_bytes;
		P.n_drain = gd_drain_launches(P.n_compact, P.full_total, P.full_max, bt);
	}
	mark("bt_off");
	// longest alignments first inside each class: the tail of the grid is then made of short jobs (a class whose members all have
	// one geometry -- a short-read batch -- is in order already)
	for (int k = 0; k < 4; ++k) {
		bool uniform = true;
		for (size_t j = 1; j < ids[k].size() && uniform; ++j) {
			const KswTask &A = h_tasks[ids[k][0]], &B = h_tasks[ids[k][j]];
			uniform = A.qlen == B.qlen && A.tlen == B.tlen && A.w == B.w;
		}
		if (uniform) continue;
		// (a stable sort by geometry, done by grouping: a short-read batch has 400 k alignments but a few dozen geometries)
		struct Geo { int qlen, tlen, w; std::vector<int32_t> members; };
		std::vector<Geo> geos;
		std::unordered_map<uint64_t, std::vector<int>> slot_of; // hash of the geometry -> geos[] entries with that hash
		int g_prev = -1;
		for (int32_t id : ids[k]) {
			const KswTask &A = h_tasks[id];
			if (g_prev >= 0 && geos[g_prev].qlen == A.qlen && geos[g_prev].tlen == A.tlen && geos[g_prev].w == A.w) { geos[g_prev].members.push_back(id); continue; }
			const uint64_t h = ((uint64_t)(uint32_t)A.qlen * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)(uint32_t)A.tlen * 0xC2B2AE3D27D4EB4Full) ^ (uint64_t)(uint32_t)A.w;
			std::vector<int> &cand = slot_of[h];
			int g = -1;
			for (int c : cand) if (geos[c].qlen == A.qlen && geos[c].tlen == A.tlen && geos[c].w == A.w) { g = c; break; }
			if (g < 0) { g = (int)geos.size(); geos.push_back(Geo{A.qlen, A.tlen, A.w, {}}); cand.push_back(g); }
			geos[g].members.push_back(id), g_prev = g;
		}
		std::vector<int> order(geos.size());
		for (size_t g = 0; g < geos.size(); ++g) order[g] = (int)g;
		std::sort(order.begin(), order.end(), [&](int a, int b) {
			const Geo &A = geos[a], &B = geos[b];
			if ((int64_t)A.qlen + A.tlen != (int64_t)B.qlen + B.tlen) return (int64_t)A.qlen + A.tlen > (int64_t)B.qlen + B.tlen;
			if (A.qlen != B.qlen) return A.qlen > B.qlen; // equal geometries are neighbours (16-lane quartets below)
			return A.w > B.w;
		});
		size_t at = 0;
		for (int g : order) for (int32_t id : geos[g].members) ids[k][at++] = id;
	}
	mark("order");
	// checkpointed wide-band alignments whose band fits a 96-block ring (w = 1300: 83 blocks) go to the form with one block + one half
	// block per lane; the rest (wider bands) keep two blocks per lane.  Both lists stay longest-first.
	size_t n_ring96 = 0;
	if (wide_ck) {
		std::vector<int32_t> &v = ids[GD_KIND_WAVE128];
		n_ring96 = (size_t)(std::stable_partition(v.begin(), v.end(), [&](int32_t id) {
			const KswTask &A = h_tasks[id];
			return gd_wave_supported(A.qlen, A.tlen, A.w, 96);
		}) - v.begin());
	}
	// the short-alignment kernels run 4 / 6 / 8 alignments of identical (qlen, tlen, w) per wavefront (groups of 16 / 10 / 8 lanes):
	// cut the sorted list into such groups, one list per group width (-1 pads an incomplete group)
	std::vector<int32_t> groups[3]; // [0]: 16 lanes, [1]: 10, [2]: 8
	// Full matrices (a short-read batch: w >= both lengths) of one geometry, enough of them to keep every group of a wavefront busy for a
	// few alignments, run as skewed pipelines instead (ksw_pipe_core.h): a wavefront takes np alignments per group, sized so that the
	// run fills the GPU's wavefront slots once.  O.use_pipe == false keeps the grouped kernels.
	const size_t pipe_np_min = 8; // see pipe_compact_kernel
	std::vector<int32_t> pipe_ids;
	P.pipes.clear(), P.pipe_runs.clear();
	{
		const std::vector<int32_t> &v = ids[GD_KIND_WAVE16];
		size_t i = 0;
		while (i < v.size()) {
			const KswTask &A = h_tasks[v[i]];
			if (O.use_pipe && gd_pipe_geometry_ok(A.qlen, A.tlen, A.w)) {
				size_t j = i + 1;
				while (j < v.size() && h_tasks[v[j]].qlen == A.qlen && h_tasks[v[j]].tlen == A.tlen && h_tasks[v[j]].row_bytes == A.row_bytes &&
				       gd_pipe_geometry_ok(A.qlen, A.tlen, h_tasks[v[j]].w)) ++j;
				const PipeGeo geo = gd_pipe_geo(A.qlen, A.tlen);
				const size_t m = j - i;
				if (m >= (size_t)(2 * geo.NG) || !gd_wave_supported(A.qlen, A.tlen, A.w, 16)) { // (the second: nothing else takes it, see gd_plan_one)
					// Alignments per group of a wavefront.  The kernel has 4 wavefront slots per SIMD.  A batch on its own (synchronous call): one
					// round of wavefronts over 70 % of the slots (100 000 pairs: np 6 -> 2.18 ms, 8 -> 2.48; 12 000 pairs: np 1 -> 0.30 ms,
					// 8 -> 0.84 -- a short run wants many short pipes, filling and draining is cheaper than an empty GPU).  A lane of a context
					// with batches in flight: half of the slots and at least 8 per group -- two batches' kernels share the GPU, and the longer
					// pipes lose less to filling and draining (26.4 -> 28.7 M reads/s with eight batches in flight) -- but never fewer than 256 wavefronts.
					const size_t all_slots = (size_t)(O.wave_slots / 5 * 4), groups = (m + geo.NG - 1) / geo.NG;
					size_t np;
					if (!O.lane) np = std::max<size_t>(1, (groups + all_slots * 7 / 10 - 1) / (all_slots * 7 / 10));
					else np = std::min(std::max<size_t>(8, (groups + all_slots / 2 - 1) / (all_slots / 2)), std::max<size_t>(1, groups / 256));
					np = std::min(np, groups);
					const size_t n_waves = (m + geo.NG * np - 1) / (geo.NG * np);
					PipeRun R;
					memset(&R, 0, sizeof(R));
					R.src_off = (int32_t)pipe_ids.size(), R.dst_off = R.src_off, R.m = (int32_t)m, R.wave_off = (int32_t)P.pipes.size(), R.n_waves = (int32_t)n_waves, R.ng = geo.NG, R.np_min = (int32_t)std::max<size_t>(1, std::min(np, pipe_np_min));
					for (size_t k = i; k < j; ++k) pipe_ids.push_back(v[k]);
					PipeWave W; // (id_off, cnt, np: pipe_compact_kernel, once the pre-filter has answered)
					memset(&W, 0, sizeof(W));
					W.qlen = A.qlen, W.tlen = A.tlen, W.row_bytes = A.row_bytes;
					P.pipes.insert(P.pipes.end(), n_waves, W);
					P.pipe_runs.push_back(R);
					i = j;
					continue;
				}
			}
			const int gl = A.row_bytes >> 4, per = 64 / gl, which = gl == 16 ? 0 : gl == 10 ? 1 : 2;
			size_t j = i + 1;
			while (j < v.size() && j < i + per) {
				const KswTask &B = h_tasks[v[j]];
				if (B.qlen != A.qlen || B.tlen != A.tlen || B.w != A.w) break;
				++j;
			}
			for (size_t k = i; k < i + per; ++k) groups[which].push_back(k < j ? v[k] : -1);
			i = j;
		}
	}
	mark("groups");
	P.ids.clear();
	for (int k = 0; k < 4; ++k) {
		P.id_off[k] = P.ids.size(), P.n_kind[k] = ids[k].size();
		if (k == GD_KIND_WAVE16) {
			for (int g = 0; g < 3; ++g) P.group_off[g] = P.ids.size(), P.n_group[g] = groups[g].size(), P.ids.insert(P.ids.end(), groups[g].begin(), groups[g].end());
			for (PipeRun &R : P.pipe_runs) R.src_off += (int32_t)P.ids.size(); // (relative to the batch's whole id list from here on)
			P.ids.insert(P.ids.end(), pipe_ids.begin(), pipe_ids.end());
			if (!P.pipes.empty()) P.mask |= 16;
		} else P.ids.insert(P.ids.end(), ids[k].begin(), ids[k].end());
	}
	P.n_pipe_ids = pipe_ids.size();
	P.cells = cells_sum, P.alg_bytes = alg_sum, P.max_cap = max_cap, P.bt = bt, P.wide_ck = wide_ck, P.n_ring96 = n_ring96;
}

// ---- auto mode of the quarter rung (ksw_wave.hip.h, "THE QUARTER RUNG") -----------------------------------------------------------------
// A box whose certificate fails at GD_W_QUARTER has paid for the quarter-block rows for nothing: offering the rung costs every box
// cost_quarter_row per anti-diagonal and saves a certified box cost_half_row, so it pays iff the certified share is above
// cost_quarter_row / cost_half_row = GD_QUARTER_BREAK_EVEN_NUM / _DEN = 4 / 5, from the measured kernel times of the two row forms
// (DESIGN.md section 3 has the derivation).  The context feeds the
// counters of every finished launch that offered the rung into gd_quarter_auto_update; a launch with at least GD_QUARTER_AUTO_MIN tries and
// a share below break-even makes the next GD_QUARTER_AUTO_HOLD launches not offer it, the one after probes again.  Results never depend
// on it.  Pure host arithmetic (tests/emul/quarter_plan_test.cpp); the context calls both under its dp_mu.
#define GD_QUARTER_BREAK_EVEN_NUM 4
#define GD_QUARTER_BREAK_EVEN_DEN 5
#define GD_QUARTER_AUTO_MIN 64
#define GD_QUARTER_AUTO_HOLD 15
struct GdQuarterAuto {
	int32_t hold = 0; // launches still to come that do not offer the rung
};
// does the launch about to be made offer the rung?  (counts it)
static inline bool gd_quarter_auto_offer(GdQuarterAuto &A)
{
	if (A.hold > 0) {
		--A.hold;
		return false;
	}
	return true;
}
// the counters of a finished launch that offered it
static inline void gd_quarter_auto_update(GdQuarterAuto &A, uint64_t tried, uint64_t certified)
{
	if (tried < GD_QUARTER_AUTO_MIN) return;
	if (certified * GD_QUARTER_BREAK_EVEN_DEN < tried * GD_QUARTER_BREAK_EVEN_NUM) A.hold = GD_QUARTER_AUTO_HOLD;
}
