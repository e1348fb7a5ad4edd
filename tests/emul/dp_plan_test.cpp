// CPU test: the planner of a DP batch (gd_plan_batch, ksw_plan.h) on seeded batches of the shapes the mapping modes produce.  What is
// checked is what the kernels and the arena need from a plan, whatever the planner's way to get there: every alignment on exactly one
// list, that of a kernel that takes its geometry; groups and pipeline runs of one geometry; backtrace slots that do not overlap; the
// longest alignments first; the same plan however the slices are run.
// usage: dp_plan_test   (one line per batch: "<name> n=.. err=.. mask=.. kinds=g,w64,w16,w128 groups=a,b,c runs=.. pipes=.. pipe_ids=.. wide_ck=.. ring96=..";
//                        the first broken property goes to stderr and ends the run with status 1)
#define __host__
#define __device__
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <thread>
#include "ksw_plan.h"

struct Batch {
	std::vector<int64_t> qoff{0}, toff{0}, cig{0};
	std::vector<int32_t> w, ex;
	int n() const { return (int)w.size(); }
	void add(int qlen, int tlen, int w_)
	{
		qoff.push_back(qoff.back() + qlen), toff.push_back(toff.back() + tlen), cig.push_back(cig.back() + qlen + tlen + 2);
		w.push_back(w_), ex.push_back(2 * qlen);
	}
};

static uint64_t rng_state = 20251005;
static uint32_t rnd(uint32_t n) // [0, n)
{
	rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
	return (uint32_t)((rng_state >> 33) % n);
}
static int between(int lo, int hi) { return lo + (int)rnd((uint32_t)(hi - lo + 1)); }

// the length mix of tests/pipe_digest_check.py at w = 150
static void add_short_read(Batch &B)
{
	static const int lens[11] = {150, 150, 150, 150, 151, 151, 149, 148, 120, 100, 76};
	const int ln = lens[rnd(11)];
	B.add(ln, ln, 150);
}
static void add_pipe_only(Batch &B) { B.add(between(241, 256), between(241, 256), 256); } // 17 blocks with the spill: the pipelines or nothing
static void add_hifi(Batch &B)
{
	const int q = between(1000, 20000);
	B.add(q, q + between(-60, 60), between(300, 500));
}
static void add_ont(Batch &B)
{
	const int q = between(3000, 30000);
	B.add(q, q + between(-250, 250), rnd(3) ? between(1250, 1330) : between(1700, 1900)); // ~83 blocks: the 96-block ring; ~115: two blocks per lane
}

#define REQUIRE(cond, ...)                                          \
	do {                                                            \
		if (!(cond)) {                                              \
			fprintf(stderr, "%s: %s -- ", name, #cond);             \
			fprintf(stderr, __VA_ARGS__), fprintf(stderr, "\n");    \
			exit(1);                                                \
		}                                                           \
	} while (0)

struct Planned {
	GdPlan P;
	std::vector<KswTask> tasks;
};

static void plan(Planned &R, const GdPlanOpt &O, const Batch &B, bool threads)
{
	R.tasks.assign((size_t)B.n(), KswTask());
	auto noop = [](const char *) {};
	if (!threads)
		gd_plan_batch(R.P, O, B.n(), B.qoff.data(), B.toff.data(), B.w.data(), B.cig.data(), B.ex.data(), R.tasks.data(), [](int n_sl, auto f) { for (int sl = 0; sl < n_sl; ++sl) f(sl); }, noop);
	else
		gd_plan_batch(R.P, O, B.n(), B.qoff.data(), B.toff.data(), B.w.data(), B.cig.data(), B.ex.data(), R.tasks.data(), [](int n_sl, auto f) {
			std::vector<std::thread> th;
			for (int t = 0; t < 4; ++t) th.emplace_back([=]() { for (int sl = n_sl - 1 - t; sl >= 0; sl -= 4) f(sl); });
			for (std::thread &x : th) x.join();
		}, noop);
}

static bool same_plan(const Planned &A, const Planned &B)
{
	const GdPlan &P = A.P, &Q = B.P;
	if (P.err != Q.err || P.mask != Q.mask) return false;
	if (memcmp(A.tasks.data(), B.tasks.data(), sizeof(KswTask) * A.tasks.size())) return false;
	if (P.err) return true;
	if (P.cells != Q.cells || P.alg_bytes != Q.alg_bytes || P.max_cap != Q.max_cap || P.bt != Q.bt || P.wide_ck != Q.wide_ck || P.n_ring96 != Q.n_ring96 || P.n_pipe_ids != Q.n_pipe_ids) return false;
	if (memcmp(P.id_off, Q.id_off, sizeof P.id_off) || memcmp(P.n_kind, Q.n_kind, sizeof P.n_kind) || memcmp(P.group_off, Q.group_off, sizeof P.group_off) || memcmp(P.n_group, Q.n_group, sizeof P.n_group)) return false;
	if (P.ids != Q.ids || P.pipes.size() != Q.pipes.size() || P.pipe_runs.size() != Q.pipe_runs.size()) return false;
	return (P.pipes.empty() || !memcmp(P.pipes.data(), Q.pipes.data(), sizeof(PipeWave) * P.pipes.size())) &&
	       (P.pipe_runs.empty() || !memcmp(P.pipe_runs.data(), Q.pipe_runs.data(), sizeof(PipeRun) * P.pipe_runs.size()));
}

// qlen + tlen never increases along ids[a, b), pads skipped
static bool longest_first(const std::vector<KswTask> &T, const std::vector<int32_t> &ids, size_t a, size_t b)
{
	int64_t prev = INT64_MAX;
	for (size_t j = a; j < b; ++j) {
		if (ids[j] < 0) continue;
		const int64_t s = (int64_t)T[ids[j]].qlen + T[ids[j]].tlen;
		if (s > prev) return false;
		prev = s;
	}
	return true;
}

// plans the batch both ways, checks the plan, prints its line; returns it
static Planned run(const char *name, const GdPlanOpt &O, const Batch &B, int want_err = 0)
{
	Planned R, R2;
	plan(R, O, B, false), plan(R2, O, B, true);
	REQUIRE(same_plan(R, R2), "the plan depends on how the slices are run");
	const GdPlan &P = R.P;
	const std::vector<KswTask> &T = R.tasks;
	const int n = B.n();
	REQUIRE(P.err == want_err, "err %d, expected %d", P.err, want_err);
	if (P.err) {
		printf("%s n=%d err=%d\n", name, n, P.err);
		return R;
	}
	// ---- every alignment: its own fields, a kernel that takes it -------------------------------------------------------------
	size_t n_kind[4] = {0, 0, 0, 0};
	for (int i = 0; i < n; ++i) {
		const KswTask &A = T[i];
		REQUIRE(A.qlen == B.qoff[i + 1] - B.qoff[i] && A.tlen == B.toff[i + 1] - B.toff[i] && A.w == B.w[i] && A.qoff == B.qoff[i] && A.toff == B.toff[i], "task %d: geometry", i);
		REQUIRE(A.cig_off == B.cig[i] && A.cig_cap == B.cig[i + 1] - B.cig[i] && A.exact_score == B.ex[i], "task %d: CIGAR slot / exact score", i);
		REQUIRE(A.kind >= 0 && A.kind < 4, "task %d: kind %d", i, A.kind);
		++n_kind[A.kind];
		if (O.kernel_mode == 1 || !O.wave_scoring_ok) REQUIRE(A.kind == GD_KIND_GENERIC, "task %d: kind %d where only the generic kernel may run", i, A.kind);
		if (O.kernel_mode == 2) REQUIRE(A.kind != GD_KIND_GENERIC, "task %d: generic in wave-only mode", i);
		if (A.kind == GD_KIND_GENERIC || A.kind == GD_KIND_WAVE128) REQUIRE(A.row_bytes == 16 * gd_ncol16(A.qlen, A.tlen, A.w), "task %d: row_bytes %d", i, A.row_bytes);
		if (A.kind == GD_KIND_WAVE64) REQUIRE(A.row_bytes == 16 * 64 && gd_wave_supported(A.qlen, A.tlen, A.w, 64), "task %d: not a 64-lane geometry", i);
		if (A.kind == GD_KIND_WAVE128) REQUIRE(gd_wave_supported(A.qlen, A.tlen, A.w, 128), "task %d: not a 128-block geometry", i);
		if (A.kind == GD_KIND_GENERIC) REQUIRE(gd_generic_cap(A.qlen, A.tlen, A.w) <= P.max_cap && P.max_cap * 7 <= 160 * 1024 - 1024, "task %d: LDS window", i);
	}
	for (int k = 0; k < 4; ++k) REQUIRE(n_kind[k] == P.n_kind[k], "kind %d: %zu tasks, %zu planned", k, n_kind[k], P.n_kind[k]);
	REQUIRE(!(P.mask & 1) == !n_kind[GD_KIND_WAVE64] && !(P.mask & 2) == !n_kind[GD_KIND_GENERIC] && !(P.mask & 4) == !n_kind[GD_KIND_WAVE16] &&
	        !(P.mask & 8) == !n_kind[GD_KIND_WAVE128] && !(P.mask & 16) == P.pipes.empty() && !(P.mask & ~31), "mask %d", P.mask);
	// ---- the id lists: back to back, every alignment once, in the list of its kind ----------------------------------------------
	const size_t pipe_off = P.group_off[2] + P.n_group[2];
	REQUIRE(P.id_off[0] == 0 && P.ids.size() == P.id_off[3] + P.n_kind[3], "id lists: ends");
	for (int k = 0; k < 3; ++k)
		if (k != GD_KIND_WAVE16) REQUIRE(P.id_off[k + 1] == P.id_off[k] + P.n_kind[k], "id list %d: not back to back", k);
	REQUIRE(P.group_off[0] == P.id_off[GD_KIND_WAVE16] && P.group_off[1] == P.group_off[0] + P.n_group[0] && P.group_off[2] == P.group_off[1] + P.n_group[1] &&
	        pipe_off + P.n_pipe_ids == P.id_off[GD_KIND_WAVE16 + 1], "short-alignment lists: not back to back");
	std::vector<uint8_t> seen((size_t)n, 0);
	for (int k = 0; k < 4; ++k)
		for (size_t j = P.id_off[k]; j < (k < 3 ? P.id_off[k + 1] : P.ids.size()); ++j) {
			const int32_t id = P.ids[j];
			if (id == -1 && k == GD_KIND_WAVE16 && j < pipe_off) continue;
			REQUIRE(id >= 0 && id < n, "ids[%zu] = %d", j, id);
			REQUIRE(T[id].kind == k, "alignment %d of kind %d on the list of kind %d", id, T[id].kind, k);
			REQUIRE(!seen[id]++, "alignment %d listed twice", id);
		}
	for (int i = 0; i < n; ++i) REQUIRE(seen[i], "alignment %d on no list", i);
	// ---- groups of 4 / 6 / 8 ---------------------------------------------------------------------------------------------------
	for (int g = 0; g < 3; ++g) {
		const int lanes = g == 0 ? 16 : g == 1 ? 10 : 8, per = 64 / lanes;
		REQUIRE(P.n_group[g] % per == 0, "%d-lane list: %zu entries", lanes, P.n_group[g]);
		for (size_t j = P.group_off[g]; j < P.group_off[g] + P.n_group[g]; j += per) {
			REQUIRE(P.ids[j] >= 0, "%d-lane group at %zu starts with a pad", lanes, j);
			const KswTask &A = T[P.ids[j]];
			REQUIRE(gd_wave_supported(A.qlen, A.tlen, A.w, 16) && A.tlen <= 16 * lanes, "%d-lane group at %zu: geometry %d x %d w %d", lanes, j, A.qlen, A.tlen, A.w);
			bool pad = false;
			for (int k = 0; k < per; ++k) {
				if (P.ids[j + k] < 0) { pad = true; continue; }
				const KswTask &M = T[P.ids[j + k]];
				REQUIRE(!pad, "%d-lane group at %zu: an alignment behind a pad", lanes, j);
				REQUIRE(M.qlen == A.qlen && M.tlen == A.tlen && M.w == A.w && M.row_bytes == 16 * lanes, "%d-lane group at %zu: members differ", lanes, j);
			}
		}
		REQUIRE(longest_first(T, P.ids, P.group_off[g], P.group_off[g] + P.n_group[g]), "%d-lane list: not longest first", lanes);
	}
	// ---- pipeline runs -----------------------------------------------------------------------------------------------------------
	REQUIRE(longest_first(T, P.ids, pipe_off, pipe_off + P.n_pipe_ids), "pipeline ids: not longest first");
	{
		std::vector<uint8_t> src_used(P.n_pipe_ids, 0), dst_used(P.n_pipe_ids, 0), wave_used(P.pipes.size(), 0);
		size_t n_src = 0, n_wave = 0;
		for (size_t r = 0; r < P.pipe_runs.size(); ++r) {
			const PipeRun &R_ = P.pipe_runs[r];
			REQUIRE(R_.m >= 1 && R_.src_off >= (int64_t)pipe_off && (size_t)R_.src_off + R_.m <= pipe_off + P.n_pipe_ids, "run %zu: ids outside the pipeline list", r);
			REQUIRE(R_.dst_off >= 0 && (size_t)R_.dst_off + R_.m <= P.n_pipe_ids, "run %zu: compacted ids outside their buffer", r);
			REQUIRE(R_.wave_off >= 0 && R_.n_waves >= 1 && (size_t)R_.wave_off + R_.n_waves <= P.pipes.size(), "run %zu: wavefronts outside the table", r);
			const KswTask &A = T[P.ids[R_.src_off]];
			const PipeGeo geo = gd_pipe_geo(A.qlen, A.tlen);
			REQUIRE(R_.ng == geo.NG && R_.n_waves <= (R_.m + geo.NG - 1) / geo.NG, "run %zu: ng %d n_waves %d for m %d", r, R_.ng, R_.n_waves, R_.m);
			REQUIRE(R_.np_min >= 1 && R_.np_min <= 8 && R_.count == 0 && R_.done == 0, "run %zu: np_min %d count %d done %d", r, R_.np_min, R_.count, R_.done);
			for (int k = 0; k < R_.m; ++k) {
				const KswTask &M = T[P.ids[R_.src_off + k]];
				REQUIRE(M.qlen == A.qlen && M.tlen == A.tlen && M.row_bytes == A.row_bytes && gd_pipe_geometry_ok(M.qlen, M.tlen, M.w), "run %zu: member %d", r, k);
				REQUIRE(!src_used[R_.src_off - pipe_off + k]++ && !dst_used[R_.dst_off + k]++, "run %zu overlaps another", r);
			}
			REQUIRE(A.row_bytes >= 16 * geo.G, "run %zu: rows of %d bytes for %d blocks", r, A.row_bytes, geo.G);
			for (int k = 0; k < R_.n_waves; ++k) {
				const PipeWave &W = P.pipes[R_.wave_off + k];
				REQUIRE(!wave_used[R_.wave_off + k]++, "run %zu: wavefront of another run", r);
				REQUIRE(W.qlen == A.qlen && W.tlen == A.tlen && W.row_bytes == A.row_bytes && W.id_off == 0 && W.np == 0 && W.cnt == 0, "run %zu: wavefront record %d", r, k);
			}
			n_src += R_.m, n_wave += R_.n_waves;
		}
		REQUIRE(n_src == P.n_pipe_ids && n_wave == P.pipes.size(), "runs cover %zu of %zu ids, %zu of %zu wavefronts", n_src, P.n_pipe_ids, n_wave, P.pipes.size());
	}
	// ---- the other kinds: longest first; the two forms of the checkpointed wide-band kernel -------------------------------------------
	REQUIRE(longest_first(T, P.ids, P.id_off[GD_KIND_GENERIC], P.id_off[GD_KIND_GENERIC] + n_kind[GD_KIND_GENERIC]), "generic list: not longest first");
	REQUIRE(longest_first(T, P.ids, P.id_off[GD_KIND_WAVE64], P.id_off[GD_KIND_WAVE64] + n_kind[GD_KIND_WAVE64]), "64-lane list: not longest first");
	{
		const size_t a = P.id_off[GD_KIND_WAVE128], b = a + n_kind[GD_KIND_WAVE128];
		REQUIRE(P.n_ring96 <= n_kind[GD_KIND_WAVE128] && (P.wide_ck || P.n_ring96 == 0), "n_ring96 %zu", P.n_ring96);
		REQUIRE(longest_first(T, P.ids, a, a + P.n_ring96) && longest_first(T, P.ids, a + P.n_ring96, b), "wide-band list: not longest first");
		if (P.wide_ck)
			for (size_t j = a; j < b; ++j) {
				const KswTask &A = T[P.ids[j]];
				REQUIRE(gd_wave_supported(A.qlen, A.tlen, A.w, 96) == (j < a + P.n_ring96), "wide-band alignment %d on the wrong side of n_ring96", P.ids[j]);
			}
		if (O.single_affine) REQUIRE(!P.wide_ck, "checkpointed form for a single-affine batch");
		if (O.wide_ckpt >= 0 && n_kind[GD_KIND_WAVE128] && !O.single_affine) REQUIRE(P.wide_ck == (O.wide_ckpt == 1), "wide_ckpt %d ignored", O.wide_ckpt);
	}
	// ---- backtrace slots -------------------------------------------------------------------------------------------------------------
	for (int i = 0; i < n; ++i) {
		const KswTask &A = T[i];
		const size_t size = P.wide_ck && A.kind == GD_KIND_WAVE128 ? gd_ck_bytes(A.qlen, A.tlen, A.row_bytes) : (size_t)(A.qlen + A.tlen - 1) * (size_t)A.row_bytes;
		const size_t end = i + 1 < n ? (size_t)T[i + 1].bt_off : P.bt;
		REQUIRE(A.bt_off >= 0 && A.bt_off % 256 == 0 && (i > 0 || A.bt_off == 0), "task %d: bt_off %lld", i, (long long)A.bt_off);
		REQUIRE((size_t)A.bt_off + size + 64 <= end && end < (size_t)A.bt_off + size + 64 + 256, "task %d: slot [%lld, %zu) for %zu bytes", i, (long long)A.bt_off, end, size);
	}
	REQUIRE(P.bt % 256 == 0, "arena of %zu bytes", P.bt);
	printf("%s n=%d err=0 mask=%d kinds=%zu,%zu,%zu,%zu groups=%zu,%zu,%zu runs=%zu pipes=%zu pipe_ids=%zu wide_ck=%d ring96=%zu\n", name, n, P.mask, n_kind[0], n_kind[1], n_kind[2],
	       n_kind[3], P.n_group[0], P.n_group[1], P.n_group[2], P.pipe_runs.size(), P.pipes.size(), P.n_pipe_ids, (int)P.wide_ck, P.n_ring96);
	return R;
}

int main()
{
	GdPlanOpt root; // the defaults: a context of its own on a device of 5120 wavefront slots
	GdPlanOpt lane = root;
	lane.lane = true;

	Batch sr, p17, hifi, ont, ont_few, mix;
	for (int i = 0; i < 120000; ++i) add_short_read(sr);
	for (int i = 0; i < 6000; ++i) add_pipe_only(p17);
	for (int i = 0; i < 4000; ++i) add_hifi(hifi);
	for (int i = 0; i < 1500; ++i) add_ont(ont);
	for (int i = 0; i < 600; ++i) add_ont(ont_few);
	for (int i = 0; i < 24000; ++i) {
		const uint32_t c = rnd(32);
		if (c < 20) add_short_read(mix);
		else if (c < 24) add_pipe_only(mix);
		else if (c < 27) add_hifi(mix);
		else if (c < 31) add_ont(mix);
		else if (rnd(2)) mix.add(between(9000, 12000), between(9000, 12000), 5000); // 300 blocks: no wave kernel
		else if (rnd(2)) mix.add(between(30, 200), between(30, 200), between(5, 40));  // a short one, narrow band, lengths apart
		else mix.add(100, 100 + between(0, 1), 10 * between(3, 6));                    // short, banded: groups must not mix the bands of one length
	}

	run("sr_root", root, sr);
	const Planned sr_lane = run("sr_lane", lane, sr);
	for (const PipeRun &R : sr_lane.P.pipe_runs) // a lane's pipes: at least 8 per group unless that leaves fewer than 256 wavefronts
		if (R.m >= 256 * 8 * R.ng && R.np_min != 8) { fprintf(stderr, "sr_lane: np_min %d for a run of %d\n", R.np_min, R.m); return 1; }
	GdPlanOpt o = root;
	o.use_pipe = false;
	run("sr_nopipe", o, sr);
	o = root, o.group_lanes = 16;
	run("sr_lanes16", o, sr);
	o.use_pipe = false;
	run("sr_lanes16_nopipe", o, sr);
	run("pipe_only", root, p17);
	run("hifi", root, hifi);
	run("ont", root, ont);
	run("ont_few", root, ont_few);
	o = root, o.wide_ckpt = 0;
	run("ont_nockpt", o, ont);
	o = root, o.wide_ckpt = 1;
	run("ont_few_ckpt", o, ont_few);
	o = root, o.single_affine = true;
	run("ont_single", o, ont);
	run("mix_root", root, mix);
	run("mix_lane", lane, mix);
	o = root, o.kernel_mode = 1;
	run("mix_generic", o, mix);
	o = root, o.wave_scoring_ok = false;
	run("mix_scoring", o, mix);
	o = root, o.kernel_mode = 2;
	run("mix_waveonly", o, mix, 2);  // the 300-block alignments
	run("sr_waveonly", o, sr);

	// errors: 1 (empty sequence) before 2 (no wave kernel, wave-only mode) before 4 (beyond the generic kernel's LDS window)
	Batch big = hifi, big_empty;
	big.add(20000, 20000, 20000); // full matrix of 20 kbp: 1 251 blocks, an LDS ring of 32 768 cells
	big_empty = big;
	big_empty.add(0, 100, 50), big_empty.add(100, 100, 50);
	o = root;
	run("big", o, big, 4);
	run("big_empty", o, big_empty, 1);
	o.kernel_mode = 1;
	run("big_generic", o, big, 4);
	o.kernel_mode = 2;
	run("big_waveonly", o, big, 2);
	run("big_empty_waveonly", o, big_empty, 1);
	Batch empty_t = sr;
	empty_t.add(100, 0, 50);
	run("sr_empty", root, empty_t, 1);
	return 0;
}
