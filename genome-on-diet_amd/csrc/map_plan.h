// The host tables of one mapping call (gd_map_range, map_pipeline.hip.h): the seed kernel's capacity classes, the scratch layout, and the
// box tables the DP, pack and record stages read.  Host arithmetic only -- no device call, no environment, no context -- so that
// tests/emul/map_plan_test.cpp can run it on the CPU; the caller grows the buffers, uploads and launches.  run(n, f) calls f(i) for every
// i in [0, n), in any order and on any threads.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>
#include "map_host.h"

// ---- seed stage: LDS sort capacity -----------------------------------------------------------------------------------------------
// minimizers expected of a read, with a quarter to spare: ~1.25 x (2 / (w + 1) of its sparsified bases)
static inline double gd_seed_est(const GdPattern &pat, int w, int64_t len) { return 1.25 * 2.0 / (w + 1) * gd_diet_len(pat, (unsigned)len, 0); }

// LDS sort capacity of the wave seed kernel for a read of len bases; *cls: its class (capacity = MAP_SORT_CAP << class)
static inline int gd_seed_cap(const GdPattern &pat, int w, int64_t len, int *cls = nullptr)
{
	const double est = gd_seed_est(pat, w, len);
	int cap = MAP_SORT_CAP, c = 0;
	while (cap < MAP_SORT_CAP_MAX && cap < est) cap <<= 1, ++c;
	if (cls) *cls = c;
	return cap;
}

// dynamic LDS bytes of a seed kernel that keeps the winnowing windows of 64 reads in LDS (w x 64 entries) and sorts in the same buffer.
// (The wave seed kernel holds no windows any more: its launches are sized by gd_seed_wave_lds_bytes, map_kernels.hip.h.)
static inline size_t gd_seed_lds_bytes(int w, int cap) { return std::max<size_t>((size_t)w * 64 * sizeof(GdMini), (size_t)cap * sizeof(uint64_t)); }

// Reads of very different lengths (ONT: log-normal up to 150 kbp): one launch per capacity class, each read in the class its own
// length asks for, so that a 30 kbp read does not hold the 128 KB of LDS the longest read of the batch needs -- 128 KB is one
// wavefront per CU, and never beside a DP kernel that keeps 48 KB of it.  (A read is treated exactly as if it were the longest read
// of its batch: every path of the kernel is exact, the capacity only selects between them.)
struct GdSeedClasses {
	int sort_cap = MAP_SORT_CAP;                // of the longest read of the batch
	std::vector<int32_t> ids;                   // the reads, class by class
	std::vector<std::pair<int, int>> classes;   // (capacity, reads), longest class first; empty: one launch over all reads
};
static inline void gd_seed_classes(const GdPattern &pat, int w, int n, const int64_t *roff, GdSeedClasses &S)
{
	int64_t max_len = 0;
	for (int i = 0; i < n; ++i) max_len = std::max<int64_t>(max_len, roff[i + 1] - roff[i]);
	S.sort_cap = gd_seed_cap(pat, w, max_len);
	S.ids.clear(), S.classes.clear();
	if (S.sort_cap <= MAP_SORT_CAP || n <= 1) return;
	std::vector<int> cap_of(n);
	int n_cls[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	for (int i = 0; i < n; ++i) gd_seed_cap(pat, w, roff[i + 1] - roff[i], &cap_of[i]), ++n_cls[cap_of[i]];
	int used = 0;
	for (int c = 0; c < 8; ++c) used += n_cls[c] > 0;
	if (used <= 1) return;
	S.ids.reserve(n);
	for (int c = 7; c >= 0; --c) {
		if (!n_cls[c]) continue;
		S.classes.push_back({MAP_SORT_CAP << c, n_cls[c]});
		for (int i = 0; i < n; ++i) if (cap_of[i] == c) S.ids.push_back(i);
	}
}

// ---- scratch layout ----------------------------------------------------------------------------------------------------------------
// mm_sketch2 keeps the minimizers of all W pattern phases back to back (LR/sketch.c:2185-2223): a phase has at most one per sparsified
// base, (len / W + 1) * ones; with -i < 1 phase 0 sees only the first max_seeds * len bases and the later phases stop at its count, with
// -i >= 1 every phase stops at (uint32_t)max_seeds.  For "10" and -i 0.2 that is a fifth of the read; a long pattern with many ones and
// a small window passes one entry per base (40 ones, w = 1, -i 0.2: eight per base).
static inline uint64_t gd_sketch2_bound(const GdPattern &pat, float max_seeds, uint32_t len)
{
	const uint64_t per_full = ((uint64_t)len / (uint32_t)pat.W + 1) * (uint32_t)pat.ones;
	const uint64_t per = max_seeds < 1 ? ((uint64_t)(uint32_t)((float)max_seeds * len) / (uint32_t)pat.W + 1) * (uint32_t)pat.ones : (uint64_t)(uint32_t)max_seeds;
	return (uint64_t)pat.W * std::min(per, per_full);
}

// minimizer lists: len/3 + 512 entries per read cover every density the presets produce; a read that overflows its list
// (tiny windows, homopolymer reads, long patterns) makes the whole batch retry once with the hard bound (full).  Returns the total of the capacities.
static inline uint64_t gd_scratch_layout(int n, const int64_t *roff, int w, const GdPattern &pat, float max_seeds, bool full, MapReadScratch *sc)
{
	uint64_t tot = 0;
	for (int i = 0; i < n; ++i) {
		const uint32_t len = (uint32_t)(roff[i + 1] - roff[i]);
		// hard bound: one minimizer per base (mm_sketch3) or the list of mm_sketch2, whichever is longer, plus a margin of
		// 64 * (w + 4) entries (once the staging lists of the sliced wavefront sketch; the tile sketch writes the list directly)
		const uint32_t hard = (uint32_t)std::max<uint64_t>(len, gd_sketch2_bound(pat, max_seeds, len));
		sc[i].mv_cap = full ? hard + 64 * (uint32_t)(w + 4) : len / 3 + 512, sc[i].mv_off = tot, sc[i].u64_off = 2 * tot, sc[i].seed_off = tot, sc[i].pad = 0;
		tot += sc[i].mv_cap;
	}
	return tot;
}

// ---- box tables --------------------------------------------------------------------------------------------------------------------
// What the box stage of a call leaves, whether it ran on the device (ShortReads: the tables are copies of the kernels' output) or on host
// threads (the functions below).  Read i owns the candidates cflat[cfirst[i] .. cfirst[i] + ccount[i]), which are the boxes
// box_first[i] .. box_first[i + 1) of the DP batch; qoff / toff / coff (nb + 1 entries): query window, target window and CIGAR slot of a box.
struct GdBoxTables {
	int nb = 0;
	GdCandBox *cflat = nullptr; // (the caller's buffer, kept between batches)
	std::vector<int> cfirst, ccount, box_first;
	std::vector<int64_t> qoff, toff, coff;
	std::vector<int32_t> bw, ex; // band width and exact-match score per box
	void reset(int n) { nb = 0, cfirst.assign(n + 1, 0), ccount.assign(n, 0), box_first.assign(n + 1, 0); }
};

// the packed host copy of the vote records: only the head of every record can be in use, n_cand + at most AF_max_loc (ShortReads) /
// vt_nb_loc + 2 (LongReads) candidates (a full-size array would be 680 B per read: 178 MB to allocate and clear per 262 k short reads)
static inline size_t gd_vote_head_bytes(const GdMapOpt &O)
{
	return offsetof(MapVoteOut, cand) + sizeof(GdVt) * std::min<size_t>((O.flag & GD_F_SR) ? (size_t)O.af_max_loc : (size_t)O.vt_nb_loc + 2, GDM_MAX_VT);
}
static inline const MapVoteOut &gd_vote_head(const uint8_t *vo_raw, size_t vo_head, int i) { return *reinterpret_cast<const MapVoteOut *>(vo_raw + vo_head * (size_t)i); }

// first candidate slot of every read, after T.reset(n) (capacity: what the vote kernel reported; the box stage may drop some); returns the slots needed
static inline int gd_box_slots(GdBoxTables &T, int n, const uint8_t *vo_raw, size_t vo_head)
{
	for (int i = 0; i < n; ++i) T.cfirst[i + 1] = T.cfirst[i] + (int)gd_vote_head(vo_raw, vo_head, i).n_cand;
	return T.cfirst[n];
}

// G1b / G2: candidates -> boxes of every read in T.cflat (entries [cfirst[i], cfirst[i] + ccount[i]) are written, nothing else is read later)
template <class Run>
static void gd_box_candidates(GdBoxTables &T, int n, const int64_t *roff, const uint8_t *vo_raw, size_t vo_head, const GdMapOpt &O, const GdRefView &R, Run run)
{
	const bool is_sr = (O.flag & GD_F_SR) != 0;
	GdCandBox *cflat = T.cflat;
	run(n, [&](int i) {
		const MapVoteOut &vo_i = gd_vote_head(vo_raw, vo_head, i); // head of the record only
		const unsigned nc = vo_i.n_cand;
		if (!nc) return;
		if (is_sr) { // straight into the flat array: a quarter of a million reads per batch, nothing allocated per read
			int k = 0;
			for (unsigned j = 0; j < nc; ++j)
				if (gd_sr_box_one(vo_i.cand[j], O, R, (uint32_t)(roff[i + 1] - roff[i]), cflat[(size_t)T.cfirst[i] + k])) ++k;
			T.ccount[i] = k;
			return;
		}
		std::vector<GdCand> C(nc);
		for (unsigned j = 0; j < nc; ++j) C[j].v = vo_i.cand[j];
		gd_lr_link_and_boxes(C, O, R, (uint32_t)(roff[i + 1] - roff[i]));
		T.ccount[i] = (int)std::min<size_t>(C.size(), nc);
		for (int j = 0; j < T.ccount[i]; ++j) cflat[(size_t)T.cfirst[i] + j] = gd_cand_box(C[j]);
	});
}

// A degenerate DP box (gd_box_degenerate) fails ITS READ -- it comes back unmapped (n_regs = 0) and is counted -- not the batch: a
// production run must not be lost to one pathological read.  fault (fault injection for the tests: no read built so far produces such
// a box; -1: none) marks the boxes of that read as degenerate.  Then box_first and nb.  Returns the number of failed reads.
static inline int64_t gd_box_fail_degenerate(GdBoxTables &T, int n, const int64_t *roff, int fault, int *last_bad)
{
	int64_t n_failed = 0;
	*last_bad = -1;
	for (int i = 0; i < n; ++i) {
		const uint32_t rl = (uint32_t)(roff[i + 1] - roff[i]);
		bool bad = i == fault && T.ccount[i] > 0;
		for (int j = 0; j < T.ccount[i] && !bad; ++j) bad = gd_box_degenerate(T.cflat[(size_t)T.cfirst[i] + j], rl);
		if (bad) T.ccount[i] = 0, ++n_failed, *last_bad = i;
	}
	for (int i = 0; i < n; ++i) T.box_first[i + 1] = T.box_first[i] + T.ccount[i];
	T.nb = T.box_first[n];
	return n_failed;
}

static inline std::string gd_failed_reads_warning(int64_t n_failed, int last_bad)
{
	char msg[160];
	snprintf(msg, sizeof msg, "%lld read(s) of the batch left unmapped: degenerate DP box (candidate window outside the read / contig), last: read %d of the call",
	         (long long)n_failed, last_bad);
	return msg;
}

// offsets of the windows and CIGAR slots, then the MapBox records (boxes: T.nb entries), band widths and exact-match scores
template <class Run, class Mark>
static void gd_box_fill(GdBoxTables &T, int n, const int64_t *roff, const GdMapOpt &O, const GdSrVoteOpt &sr, const GdRefView &R, MapBox *boxes, Run run, Mark &mark)
{
	const bool is_sr = (O.flag & GD_F_SR) != 0;
	const int nb = T.nb;
	const GdCandBox *cflat = T.cflat;
	T.qoff.assign(nb + 1, 0), T.toff.assign(nb + 1, 0), T.coff.assign(nb + 1, 0);
	T.bw.resize(nb), T.ex.resize(nb);
	// window offsets: a running sum over the boxes in batch order; the boxes themselves are filled by the host threads
	for (int i = 0; i < n; ++i)
		for (int j = 0; j < T.ccount[i]; ++j) {
			const GdCandBox &c = cflat[(size_t)T.cfirst[i] + j];
			const int b = T.box_first[i] + j;
			T.qoff[b + 1] = T.qoff[b] + c.qlen, T.toff[b + 1] = T.toff[b] + c.tlen;
			T.coff[b + 1] = T.coff[b] + c.qlen + c.tlen;
		}
	mark("g:offsets");
	run(n, [&](int i) {
		const uint32_t rl = (uint32_t)(roff[i + 1] - roff[i]);
		for (int j = 0; j < T.ccount[i]; ++j) {
			const GdCandBox &c = cflat[(size_t)T.cfirst[i] + j];
			const int b = T.box_first[i] + j;
			const GdSeqInfo *sq = c.target_id < R.n_seq ? &R.seq[c.target_id] : nullptr;
			boxes[b] = gd_map_box(c, roff[i], rl, sq ? &sq->len : nullptr, sq ? &sq->offset : nullptr, T.qoff[b], T.toff[b]);
			T.bw[b] = is_sr ? (int32_t)gd_sr_bw((int)rl, sr) : (int32_t)O.bw, T.ex[b] = c.exact_score; // SR/map.c:624-631,925 ; LR/map.c:1800
		}
	});
}
