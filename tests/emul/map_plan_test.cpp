// CPU test: the host tables of a mapping call (map_plan.h) on seeded synthetic batches -- the capacity classes of the seed kernel, the
// scratch layout, and the box tables of the host box stage with its failed reads.  What is checked is what the kernels and the later
// stages need from the tables, whatever the way they were made.
// usage: map_plan_test   (one line per scenario: "<name> key=value ..."; the first broken property goes to stderr and ends the run
//                         with status 1)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <thread>
#include "map_plan.h"

static uint64_t rng_state = 20261016;
static uint32_t rnd(uint32_t n) // [0, n)
{
	rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
	return (uint32_t)((rng_state >> 33) % n);
}
static int between(int lo, int hi) { return lo + (int)rnd((uint32_t)(hi - lo + 1)); }
static double gauss() // Box-Muller
{
	const double u1 = (rnd(1000000) + 1) / 1000001.0, u2 = rnd(1000000) / 1000000.0;
	return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

#define REQUIRE(cond, ...)                                          \
	do {                                                            \
		if (!(cond)) {                                              \
			fprintf(stderr, "%s: %s -- ", name, #cond);             \
			fprintf(stderr, __VA_ARGS__), fprintf(stderr, "\n");    \
			exit(1);                                                \
		}                                                           \
	} while (0)

static auto run_serial = [](int n, auto f) { for (int i = 0; i < n; ++i) f(i); };
static auto run_threads = [](int n, auto f) { // four threads, interleaved
	std::vector<std::thread> th;
	for (int t = 0; t < 4; ++t) th.emplace_back([=] { for (int i = t; i < n; i += 4) f(i); });
	for (auto &t : th) t.join();
};
static auto no_mark = [](const char *) {};

static std::vector<int64_t> offsets_of(const std::vector<int> &lens)
{
	std::vector<int64_t> roff(lens.size() + 1, 1000); // (a slice of a batch: the first read does not start at 0)
	for (size_t i = 0; i < lens.size(); ++i) roff[i + 1] = roff[i] + lens[i];
	return roff;
}
static std::vector<int> ont_lengths(int n) // log-normal around 20 kbp, up to 200 kbp
{
	std::vector<int> v(n);
	for (int &l : v) l = (int)std::min(200000.0, std::max(200.0, exp(log(20000.0) + 0.9 * gauss())));
	return v;
}
static std::vector<int> uniform_lengths(int n, int lo, int hi)
{
	std::vector<int> v(n);
	for (int &l : v) l = between(lo, hi);
	return v;
}

// ---- capacity classes -----------------------------------------------------------------------------------------------------------
static void check_classes(const char *name, const std::vector<int> &lens, int w, const GdPattern &P)
{
	const int n = (int)lens.size();
	const std::vector<int64_t> roff = offsets_of(lens);
	GdSeedClasses S;
	S.ids.assign(3, 7), S.classes.assign(2, {1, 1}); // (stale contents of an earlier call must not survive)
	gd_seed_classes(P, w, n, roff.data(), S);
	int max_cap = MAP_SORT_CAP, caps_used = 0;
	bool seen[32] = {false};
	for (int i = 0; i < n; ++i) {
		int cls = -1;
		const int cap = gd_seed_cap(P, w, lens[i], &cls);
		REQUIRE(cap == MAP_SORT_CAP << cls && cap >= MAP_SORT_CAP && cap <= MAP_SORT_CAP_MAX, "read %d: cap %d class %d", i, cap, cls);
		REQUIRE(cap >= gd_seed_est(P, w, lens[i]) || cap == MAP_SORT_CAP_MAX, "read %d: cap %d below its estimate %.1f", i, cap, gd_seed_est(P, w, lens[i]));
		REQUIRE(cap == MAP_SORT_CAP || cap / 2 < gd_seed_est(P, w, lens[i]), "read %d: cap %d is more than its estimate %.1f asks for", i, cap, gd_seed_est(P, w, lens[i]));
		max_cap = std::max(max_cap, cap);
		if (!seen[cls]) seen[cls] = true, ++caps_used;
	}
	REQUIRE(S.sort_cap == max_cap, "sort_cap %d, largest capacity of a read %d", S.sort_cap, max_cap);
	REQUIRE(gd_seed_lds_bytes(w, S.sort_cap) >= (size_t)S.sort_cap * 8 && gd_seed_lds_bytes(w, S.sort_cap) >= (size_t)w * 64 * sizeof(GdMini), "LDS bytes %zu", gd_seed_lds_bytes(w, S.sort_cap));
	REQUIRE(gd_seed_lds_bytes(w, S.sort_cap) == std::max((size_t)S.sort_cap * 8, (size_t)w * 64 * sizeof(GdMini)), "LDS bytes %zu are more than either need", gd_seed_lds_bytes(w, S.sort_cap));
	if (caps_used <= 1 || n == 1) REQUIRE(S.classes.empty() && S.ids.empty(), "%d capacities over %d reads, but %zu classes", caps_used, n, S.classes.size());
	else {
		REQUIRE((int)S.classes.size() == caps_used && (int)S.ids.size() == n, "%zu classes for %d capacities, %zu ids for %d reads", S.classes.size(), caps_used, S.ids.size(), n);
		std::vector<int> times(n, 0);
		int at = 0;
		for (size_t c = 0; c < S.classes.size(); ++c) {
			REQUIRE(S.classes[c].second > 0, "class %zu is empty", c);
			REQUIRE(c == 0 || S.classes[c].first < S.classes[c - 1].first, "class %zu (capacity %d) does not come longest first", c, S.classes[c].first);
			for (int j = 0; j < S.classes[c].second; ++j, ++at) {
				const int id = S.ids[at];
				REQUIRE(id >= 0 && id < n, "id %d", id);
				++times[id];
				REQUIRE(S.classes[c].first == gd_seed_cap(P, w, lens[id]), "read %d in the class of capacity %d, its own is %d", id, S.classes[c].first, gd_seed_cap(P, w, lens[id]));
				REQUIRE(j == 0 || S.ids[at - 1] < id, "class %zu: reads out of batch order", c);
			}
		}
		REQUIRE(at == n, "the classes hold %d of %d reads", at, n);
		for (int i = 0; i < n; ++i) REQUIRE(times[i] == 1, "read %d is in %d classes", i, times[i]);
		REQUIRE(S.classes[0].first == S.sort_cap, "first class %d, sort_cap %d", S.classes[0].first, S.sort_cap);
	}
	printf("%s n=%d classes=%zu caps_used=%d sort_cap=%d\n", name, n, S.classes.size(), caps_used, S.sort_cap);
}

// ---- scratch layout ---------------------------------------------------------------------------------------------------------------
// Z / max_seeds: -Z / -i (the hard bound must also hold mm_sketch2's list of all pattern phases)
static void check_layout(const char *name, const std::vector<int> &lens, int w, const char *Z = "10", float max_seeds = 0.2f)
{
	GdPattern P;
	REQUIRE(gd_pattern_init(P, Z, (int)strlen(Z)), "pattern %s", Z);
	const int n = (int)lens.size();
	const std::vector<int64_t> roff = offsets_of(lens);
	uint64_t tots[2];
	for (int full = 0; full < 2; ++full) {
		std::vector<MapReadScratch> sc(n);
		memset(sc.data(), 0xff, sizeof(MapReadScratch) * n);
		const uint64_t tot = gd_scratch_layout(n, roff.data(), w, P, max_seeds, full != 0, sc.data());
		uint64_t sum = 0;
		for (int i = 0; i < n; ++i) {
			REQUIRE(sc[i].mv_off == sum && sc[i].seed_off == sum && sc[i].u64_off == 2 * sum && sc[i].pad == 0, "full=%d read %d: offsets %llu %llu %llu, running sum %llu", full, i,
			        (unsigned long long)sc[i].mv_off, (unsigned long long)sc[i].seed_off, (unsigned long long)sc[i].u64_off, (unsigned long long)sum);
			// what mm_sketch2 can emit, counted phase by phase: a phase has at most its sparsified bases, phase 0 those of the cropped read, later phases phase 0's count
			uint64_t s2 = 0, cap0 = 0;
			for (int sh = 0; sh < P.W; ++sh) {
				const uint64_t all = gd_diet_len(P, (unsigned)lens[i], (unsigned)sh);
				uint64_t m = max_seeds < 1 ? (sh == 0 ? gd_diet_len(P, (unsigned)(max_seeds * lens[i]), 0) : std::min(all, cap0)) : std::min<uint64_t>(all, (uint32_t)max_seeds);
				if (sh == 0) cap0 = m;
				s2 += m;
			}
			const uint32_t hard = (uint32_t)std::max<uint64_t>((uint64_t)lens[i], gd_sketch2_bound(P, max_seeds, (uint32_t)lens[i]));
			REQUIRE(gd_sketch2_bound(P, max_seeds, (uint32_t)lens[i]) >= s2, "read %d of %d bases: mm_sketch2 can emit %llu minimizers, bound %llu", i, lens[i], (unsigned long long)s2,
			        (unsigned long long)gd_sketch2_bound(P, max_seeds, (uint32_t)lens[i]));
			REQUIRE(sc[i].mv_cap == (full ? hard + 64u * (uint32_t)(w + 4) : (uint32_t)lens[i] / 3 + 512), "full=%d read %d of %d bases: capacity %u", full, i, lens[i], sc[i].mv_cap);
			if (!strcmp(Z, "10") && max_seeds < 1) REQUIRE(hard == (uint32_t)lens[i], "read %d: the presets' hard bound is one entry per base, got %u", i, hard);
			sum += sc[i].mv_cap;
		}
		REQUIRE(tot == sum, "full=%d: total %llu, sum %llu", full, (unsigned long long)tot, (unsigned long long)sum);
		tots[full] = tot;
	}
	REQUIRE(tots[1] > tots[0], "the hard bound %llu is not above the first layout %llu", (unsigned long long)tots[1], (unsigned long long)tots[0]);
	printf("%s n=%d tot=%llu tot_full=%llu\n", name, n, (unsigned long long)tots[0], (unsigned long long)tots[1]);
}

// ---- box tables ---------------------------------------------------------------------------------------------------------------------
static const GdSeqInfo SEQS[4] = {{"c0", 0, 50000}, {"c1", 50000, 1200}, {"c2", 51200, 300000}, {"c3", 351200, 90}};
static const GdRefView REF = {nullptr, SEQS, 4};

static GdMapOpt make_opt(bool sr)
{
	GdMapOpt O;
	O.k = sr ? 21 : 19, O.w = sr ? 11 : 19, O.a = sr ? 2 : 1, O.bw = 1000;
	if (sr) O.flag |= GD_F_SR;
	return O;
}
static GdSrVoteOpt make_sr(const GdMapOpt &O)
{
	GdSrVoteOpt S;
	S.min_cnt = O.min_cnt, S.rec_threshold_frac = O.rec_threshold_frac, S.bw_frac = 0.35f, S.bw_min = 40, S.bw_max = 120; // (bounds that 76..400 bases reach both of)
	S.af_max_loc = O.af_max_loc, S.max_nb_seeds = UINT32_MAX, S.frag_mode = 0;
	return S;
}

struct Tally { int boxes = 0, hanging = 0, beyond = 0, no_contig = 0, rev = 0, empty = 0, bw_lo = 0, bw_hi = 0; };

// what the DP, pack and record stages need from the tables of nb boxes
static Tally check_tables(const char *name, const GdBoxTables &T, const std::vector<int> &lens, const std::vector<int64_t> &roff, const std::vector<MapBox> &boxes,
                          const GdMapOpt &O, const GdSrVoteOpt &sr)
{
	const int n = (int)lens.size();
	const bool is_sr = (O.flag & GD_F_SR) != 0;
	Tally t;
	REQUIRE((int)T.box_first.size() == n + 1 && (int)T.ccount.size() == n && T.box_first[0] == 0, "table sizes");
	for (int i = 0; i < n; ++i) REQUIRE(T.box_first[i + 1] - T.box_first[i] == T.ccount[i] && T.ccount[i] >= 0, "read %d: box_first %d..%d, ccount %d", i, T.box_first[i], T.box_first[i + 1], T.ccount[i]);
	const int nb = T.nb;
	REQUIRE(nb == T.box_first[n], "nb %d, box_first[n] %d", nb, T.box_first[n]);
	REQUIRE((int)T.qoff.size() == nb + 1 && (int)T.toff.size() == nb + 1 && (int)T.coff.size() == nb + 1 && (int)T.bw.size() == nb && (int)T.ex.size() == nb, "per-box table sizes");
	REQUIRE(T.qoff[0] == 0 && T.toff[0] == 0 && T.coff[0] == 0, "offsets do not start at 0");
	for (int i = 0; i < n; ++i) {
		const uint32_t rl = (uint32_t)lens[i];
		if (!T.ccount[i]) ++t.empty;
		for (int j = 0; j < T.ccount[i]; ++j) {
			const GdCandBox &c = T.cflat[(size_t)T.cfirst[i] + j];
			const int b = T.box_first[i] + j;
			const MapBox &M = boxes[b];
			REQUIRE(!gd_box_degenerate(c, rl), "box %d of read %d is degenerate and still there", j, i);
			REQUIRE(T.qoff[b + 1] - T.qoff[b] == c.qlen && T.toff[b + 1] - T.toff[b] == c.tlen && T.coff[b + 1] - T.coff[b] == (int64_t)c.qlen + c.tlen, "box %d: offsets are not the running sums", b);
			REQUIRE(M.q_dst == T.qoff[b] && M.t_dst == T.toff[b], "box %d: q_dst %lld t_dst %lld, qoff %lld toff %lld", b, (long long)M.q_dst, (long long)M.t_dst, (long long)T.qoff[b], (long long)T.toff[b]);
			REQUIRE(M.read_off == roff[i] && M.read_len == rl && M.qseq_off == c.qseq_off && M.qlen == c.qlen && M.tlen == c.tlen && M.rev == c.v.str, "box %d: not the box of its candidate", b);
			REQUIRE(M.qseq_off + M.qlen <= M.read_len, "box %d: query window [%u, +%u) outside the read of %u", b, M.qseq_off, M.qlen, M.read_len);
			REQUIRE(M.t_avail <= M.tlen, "box %d: t_avail %u > tlen %u", b, M.t_avail, M.tlen);
			if (c.target_id >= REF.n_seq) {
				REQUIRE(M.t_avail == 0, "box %d: contig %u does not exist, t_avail %u", b, c.target_id, M.t_avail);
				++t.no_contig;
			} else {
				const GdSeqInfo &sq = SEQS[c.target_id];
				if (c.target_start >= sq.len) {
					REQUIRE(M.t_avail == 0, "box %d: starts behind its contig, t_avail %u", b, M.t_avail);
					++t.beyond;
				} else {
					REQUIRE(M.t_avail == std::min(c.tlen, sq.len - c.target_start) && M.t_avail > 0, "box %d: t_avail %u", b, M.t_avail);
					REQUIRE(M.t_src == sq.offset + c.target_start && M.t_src + M.t_avail <= sq.offset + sq.len, "box %d: window [%llu, +%u) outside its contig", b, (unsigned long long)M.t_src, M.t_avail);
					t.hanging += M.t_avail < M.tlen;
				}
			}
			REQUIRE(T.bw[b] == (is_sr ? (int32_t)gd_sr_bw((int)rl, sr) : (int32_t)O.bw), "box %d: band width %d", b, T.bw[b]);
			REQUIRE(T.ex[b] == c.exact_score, "box %d: exact-match score %d", b, T.ex[b]);
			t.bw_lo += is_sr && T.bw[b] == sr.bw_min, t.bw_hi += is_sr && T.bw[b] == sr.bw_max;
			t.rev += M.rev != 0, ++t.boxes;
		}
	}
	return t;
}

static bool same_tables(const GdBoxTables &A, const GdBoxTables &B, const std::vector<MapBox> &ba, const std::vector<MapBox> &bb)
{
	return A.nb == B.nb && A.cfirst == B.cfirst && A.ccount == B.ccount && A.box_first == B.box_first && A.qoff == B.qoff && A.toff == B.toff && A.coff == B.coff && A.bw == B.bw &&
	       A.ex == B.ex && !memcmp(ba.data(), bb.data(), sizeof(MapBox) * (size_t)A.nb);
}

static void print_tally(const char *name, int n, const Tally &t, int64_t n_failed, int last_bad)
{
	printf("%s n=%d boxes=%d hanging=%d beyond=%d no_contig=%d rev=%d empty=%d bw_lo=%d bw_hi=%d failed=%lld last=%d\n", name, n, t.boxes, t.hanging, t.beyond, t.no_contig, t.rev, t.empty,
	       t.bw_lo, t.bw_hi, (long long)n_failed, last_bad);
}

// the whole host box stage on seeded vote records: slots, candidates, failed reads, fill -- serially and on threads
static void check_votes(const char *name, bool sr, int n)
{
	const GdMapOpt O = make_opt(sr);
	const GdSrVoteOpt SV = make_sr(O);
	std::vector<int> lens(n);
	for (int &l : lens) l = sr ? (rnd(8) ? between(76, 151) : between(250, 400)) : between(2000, 20000);
	const std::vector<int64_t> roff = offsets_of(lens);
	const size_t vo_head = gd_vote_head_bytes(O);
	REQUIRE(vo_head == offsetof(MapVoteOut, cand) + sizeof(GdVt) * (sr ? 20 : 5), "head of a vote record: %zu bytes", vo_head);
	std::vector<uint8_t> vo(vo_head * (size_t)n, 0);
	int n_votes = 0;
	for (int i = 0; i < n; ++i) {
		MapVoteOut *v = reinterpret_cast<MapVoteOut *>(vo.data() + vo_head * (size_t)i); // (head only: cand[j] below the packed size)
		const unsigned nc = rnd(6) ? (unsigned)between(1, sr ? 4 : 5) : 0;
		v->n_cand = nc, n_votes += (int)nc;
		for (unsigned j = 0; j < nc; ++j) {
			GdVt &g = v->cand[j];
			g.chrom_id = rnd(40) ? rnd(REF.n_seq) : REF.n_seq + rnd(3); // now and then a contig that does not exist
			const int clen = g.chrom_id < REF.n_seq ? (int)SEQS[g.chrom_id].len : 1000;
			g.str = rnd(2);
			g.first_query_loc = (uint32_t)between(O.k - 1, lens[i] / 2), g.last_query_loc = g.first_query_loc + (uint32_t)between(1, lens[i] / 2 - 1);
			g.first_target_loc = rnd(4) ? between(0, clen) : clen - between(0, lens[i]); // a quarter of them at the contig's end
			g.last_target_loc = sr ? 0 : g.first_target_loc + (int32_t)(g.last_query_loc - g.first_query_loc) + between(-20, 20);
			g.score = (uint32_t)between(3, 50);
		}
	}
	GdBoxTables T[2];
	std::vector<MapBox> boxes[2];
	std::vector<GdCandBox> cflat[2];
	int64_t n_failed[2];
	int last_bad[2];
	for (int r = 0; r < 2; ++r) {
		T[r].reset(n);
		const int slots = gd_box_slots(T[r], n, vo.data(), vo_head);
		REQUIRE(slots == n_votes && T[r].cfirst[0] == 0, "%d slots for %d votes", slots, n_votes);
		cflat[r].resize((size_t)slots + 1);
		T[r].cflat = cflat[r].data();
		if (r) gd_box_candidates(T[r], n, roff.data(), vo.data(), vo_head, O, REF, run_threads);
		else gd_box_candidates(T[r], n, roff.data(), vo.data(), vo_head, O, REF, run_serial);
		for (int i = 0; i < n; ++i) REQUIRE(T[r].ccount[i] >= 0 && T[r].ccount[i] <= T[r].cfirst[i + 1] - T[r].cfirst[i], "read %d: %d boxes in %d slots", i, T[r].ccount[i], T[r].cfirst[i + 1] - T[r].cfirst[i]);
		n_failed[r] = gd_box_fail_degenerate(T[r], n, roff.data(), -1, &last_bad[r]);
		boxes[r].resize((size_t)T[r].nb + 1);
		if (r) gd_box_fill(T[r], n, roff.data(), O, SV, REF, boxes[r].data(), run_threads, no_mark);
		else gd_box_fill(T[r], n, roff.data(), O, SV, REF, boxes[r].data(), run_serial, no_mark);
	}
	REQUIRE(same_tables(T[0], T[1], boxes[0], boxes[1]) && n_failed[0] == n_failed[1] && last_bad[0] == last_bad[1], "serial and threaded runs differ");
	const Tally t = check_tables(name, T[0], lens, roff, boxes[0], O, SV);
	print_tally(name, n, t, n_failed[0], last_bad[0]);
}

// a good box of `len` bases of the read against tlen bases of contig `id` at `start`
static GdCandBox make_box(uint32_t rl, uint32_t qlen, uint32_t tlen, uint32_t id, uint32_t start, uint32_t str)
{
	GdCandBox b;
	memset(&b, 0, sizeof b);
	b.v.chrom_id = id, b.v.str = str, b.v.score = 9, b.next = -1, b.valid = 1;
	b.target_id = id, b.target_start = start, b.target_end = start + tlen - 1, b.qlen = qlen, b.tlen = tlen, b.qseq_off = rl - qlen;
	b.query_start = b.qseq_off, b.query_end = rl - 1, b.exact_score = qlen == tlen && rl < 300 ? (int32_t)(2 * rl) : GD_NEG_INF_SCORE;
	return b;
}

struct Reads { // seeded candidates, read by read
	std::vector<int> lens;
	std::vector<std::vector<GdCandBox>> cand;
	std::vector<GdCandBox> flat;
	void into(GdBoxTables &T) // one slot more than a read has candidates: the box stage may have dropped one
	{
		const int n = (int)lens.size();
		T.reset(n);
		for (int i = 0; i < n; ++i) T.cfirst[i + 1] = T.cfirst[i] + (int)cand[i].size() + 1, T.ccount[i] = (int)cand[i].size();
		flat.assign((size_t)T.cfirst[n] + 1, make_box(10, 0, 0, 99, 0, 0)); // (unused slots hold a degenerate box: nobody may read them)
		for (int i = 0; i < n; ++i) std::copy(cand[i].begin(), cand[i].end(), flat.begin() + T.cfirst[i]);
		T.cflat = flat.data();
	}
};

// the tables from seeded boxes that include the windows the reference reads stale memory for
static void check_seeded_tables(const char *name, bool sr)
{
	const GdMapOpt O = make_opt(sr);
	const GdSrVoteOpt SV = make_sr(O);
	Reads Rd;
	const int n = 400;
	for (int i = 0; i < n; ++i) {
		const uint32_t rl = (uint32_t)(sr ? between(76, 400) : between(2000, 20000));
		Rd.lens.push_back((int)rl);
		Rd.cand.emplace_back();
		const int nc = i % 7 == 3 ? 0 : between(1, 4); // every seventh read has no candidates
		for (int j = 0; j < nc; ++j) {
			const uint32_t qlen = (uint32_t)between(20, (int)rl), tlen = sr ? qlen : qlen + (uint32_t)between(0, 500);
			const uint32_t id = rnd(3) == 0 ? 2 : rnd(REF.n_seq), clen = SEQS[id].len;
			const int kind = (i + j) % 9;
			if (kind == 0) Rd.cand[i].push_back(make_box(rl, qlen, tlen, id, clen - std::min(clen, 1 + rnd(tlen)), rnd(2))); // hangs off the contig's end (or just fits)
			else if (kind == 1) Rd.cand[i].push_back(make_box(rl, qlen, tlen, id, clen + rnd(50), rnd(2)));                  // starts behind it
			else if (kind == 2) Rd.cand[i].push_back(make_box(rl, qlen, tlen, REF.n_seq + rnd(5), rnd(1000), rnd(2)));       // no such contig
			else if (kind == 3) Rd.cand[i].push_back(make_box(rl, qlen, tlen, id, rnd(clen), 1));                            // reverse strand
			else Rd.cand[i].push_back(make_box(rl, qlen, tlen, id, rnd(clen), rnd(2)));
		}
	}
	const std::vector<int64_t> roff = offsets_of(Rd.lens);
	GdBoxTables T;
	Rd.into(T);
	const std::vector<int> count0 = T.ccount;
	int last_bad = 0;
	const int64_t n_failed = gd_box_fail_degenerate(T, n, roff.data(), -1, &last_bad);
	REQUIRE(n_failed == 0 && last_bad == -1 && T.ccount == count0, "%lld reads failed (last %d): none of these boxes is degenerate", (long long)n_failed, last_bad);
	std::vector<MapBox> boxes((size_t)T.nb + 1);
	gd_box_fill(T, n, roff.data(), O, SV, REF, boxes.data(), run_threads, no_mark);
	print_tally(name, n, check_tables(name, T, Rd.lens, roff, boxes, O, SV), n_failed, last_bad);
}

// ---- failed reads -----------------------------------------------------------------------------------------------------------------
static int terms_of(const GdCandBox &c, uint32_t rl) // which terms of the predicate hold, as a bit mask
{
	return (c.qlen == 0) | (c.tlen == 0) << 1 | (c.qlen > rl) << 2 | (c.qseq_off + c.qlen > rl) << 3 | (c.tlen > 8u * rl + 100000u) << 4;
}

static void check_failed(const char *name, int fault, int64_t want_failed, int want_last, int want_mask)
{
	const uint32_t rl = 150;
	Reads Rd;
	const int n = 12;
	for (int i = 0; i < n; ++i) {
		Rd.lens.push_back((int)rl);
		Rd.cand.emplace_back();
		if (i == 10) continue; // a read with no candidates: fault injection has nothing to fail there
		for (int j = 0; j < 3; ++j) Rd.cand[i].push_back(make_box(rl, 150, 150, 0, 1000 * (uint32_t)(i + j), j & 1));
	}
	// one degenerate box per term of the predicate, as the first, a middle or the last box of its read
	GdCandBox *bad[5] = {&Rd.cand[1][0], &Rd.cand[2][1], &Rd.cand[3][2], &Rd.cand[4][0], &Rd.cand[5][2]};
	bad[0]->qlen = 0, bad[0]->qseq_off = 0;
	bad[1]->tlen = 0;
	bad[2]->qlen = 151, bad[2]->qseq_off = 0xffffffffu - 100; // (the sum wraps to 50: only the third term sees this one)
	bad[3]->qlen = 100, bad[3]->qseq_off = 51;
	bad[4]->tlen = 8u * rl + 100001u;
	int mask = 0;
	for (int t = 0; t < 5; ++t) {
		REQUIRE(terms_of(*bad[t], rl) == 1 << t, "case %d holds the terms %#x", t, terms_of(*bad[t], rl));
		REQUIRE(gd_box_degenerate(*bad[t], rl), "case %d is not seen as degenerate", t);
		mask |= terms_of(*bad[t], rl);
	}
	GdCandBox edge = make_box(rl, 150, 8u * rl + 100000u, 2, 0, 0); // the largest window that is still taken
	REQUIRE(terms_of(edge, rl) == 0 && !gd_box_degenerate(edge, rl), "a box at the bounds counts as degenerate");
	Rd.cand[7][1] = edge;
	const std::vector<int64_t> roff = offsets_of(Rd.lens);
	GdBoxTables T;
	Rd.into(T);
	const std::vector<int> count0 = T.ccount;
	int last_bad = 0;
	const int64_t n_failed = gd_box_fail_degenerate(T, n, roff.data(), fault, &last_bad);
	int lost = 0;
	for (int i = 0; i < n; ++i) {
		const bool should = (i >= 1 && i <= 5) || (i == fault && count0[i] > 0);
		REQUIRE(T.ccount[i] == (should ? 0 : count0[i]), "read %d keeps %d of %d boxes", i, T.ccount[i], count0[i]);
		lost += should;
	}
	REQUIRE(n_failed == lost && n_failed == want_failed && last_bad == want_last, "%lld reads failed, last %d; %d lost their boxes", (long long)n_failed, last_bad, lost);
	REQUIRE(T.nb == 3 * (n - 1 - (int)n_failed) && T.box_first[n] == T.nb, "%d boxes left", T.nb);
	const std::string warn = gd_failed_reads_warning(n_failed, last_bad);
	char want[64];
	snprintf(want, sizeof want, "%lld read(s)", (long long)n_failed);
	REQUIRE(warn.find("degenerate DP box") != std::string::npos && warn.find(want) == 0 && warn.find("read " + std::to_string(last_bad) + " of the call") != std::string::npos, "warning: %s", warn.c_str());
	// the tables of what is left
	const GdMapOpt O = make_opt(true);
	const GdSrVoteOpt SV = make_sr(O);
	std::vector<MapBox> boxes((size_t)T.nb + 1);
	gd_box_fill(T, n, roff.data(), O, SV, REF, boxes.data(), run_serial, no_mark);
	const Tally t = check_tables(name, T, Rd.lens, roff, boxes, O, SV);
	REQUIRE(mask == want_mask, "terms covered: %#x", mask);
	printf("%s n=%d boxes=%d failed=%lld last=%d terms=%d warned=1\n", name, n, t.boxes, (long long)n_failed, last_bad, mask);
}

int main()
{
	GdPattern P;
	if (!gd_pattern_init(P, "10", 2)) return 2;
	check_classes("classes_ont", ont_lengths(3000), 10, P);
	check_classes("classes_hifi", uniform_lengths(3000, 10000, 25000), 19, P);
	check_classes("classes_hifi_long", uniform_lengths(500, 70000, 100000), 19, P); // one capacity above the smallest serves all reads
	check_classes("classes_one_read", std::vector<int>(1, 150000), 10, P);
	check_classes("classes_two_reads", std::vector<int>{150000, 3000}, 10, P);
	check_layout("layout_ont", ont_lengths(3000), 10);
	check_layout("layout_sr", uniform_lengths(5000, 76, 151), 11);
	// patterns of the option grid whose mm_sketch2 list is longer than the read (tests/golden/opts/grid.json)
	check_layout("layout_40ones_w10", ont_lengths(300), 10, "11110111101111011110111101111011110111101111011110", 0.2f);
	check_layout("layout_W36_w1", ont_lengths(300), 1, "100000001000100000001000100000001000", 0.2f);
	check_layout("layout_40ones_w1_i64", ont_lengths(300), 1, "11110111101111011110111101111011110111101111011110", 64.0f);
	check_layout("layout_1_w1", ont_lengths(100), 1, "1", 0.5f);
	check_votes("votes_sr", true, 6000);
	check_votes("votes_lr", false, 1500);
	check_seeded_tables("tables_sr", true);
	check_seeded_tables("tables_lr", false);
	check_failed("failed", 8, 6, 8, 31);
	check_failed("failed_no_fault", -1, 5, 5, 31);
	check_failed("failed_fault_on_empty_read", 10, 5, 5, 31);
	check_failed("failed_fault_on_failed_read", 3, 5, 5, 31);
	return 0;
}
