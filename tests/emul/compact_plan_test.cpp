// CPU test: the compact backtrace arena of gd_plan_batch (ksw_plan.h) on random batch geometries.  With GdPlanOpt::compact a box the
// planner marks GD_NARROW_TRY gets a slot for the half-block rows only; behind the last slot lies the overflow pool such a box claims
// its full-band rows from, and the plan says how many drain launches serve every box that found no room there.  Checked: slots disjoint
// and 256-aligned, every GD_NARROW_TRY slot holds its 512-byte rows, every other slot is the one of the full-size layout, the pool lies
// behind the last slot, P.bt is the sum; without the option the layout is the full-size one; and a host model of the claim (one atomic
// add per box on the launch's counter, boxes in random order) needs no more launches than the plan says when ALL boxes fall back and
// the pool is empty.
// usage: compact_plan_test   (one line per batch: "<name> n=.. try=.. bt=.. full_bt=.. pool=.. drain=.. model=..", model = the most launches any order took;
//                             the first broken property goes to stderr and ends the run with status 1)
#define __host__
#define __device__
#include <stdio.h>
#include <stdlib.h>
#include <numeric>
#include "ksw_plan.h"

static uint64_t rng_state = 20261019;
static uint32_t rnd(uint32_t n) // [0, n)
{
	rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
	return (uint32_t)((rng_state >> 33) % n);
}
static int between(int lo, int hi) { return lo + (int)rnd((uint32_t)(hi - lo + 1)); }

struct Batch {
	std::vector<int64_t> qoff{0}, toff{0}, cig{0};
	std::vector<int32_t> w;
	int n() const { return (int)w.size(); }
	void add(int qlen, int tlen, int w_)
	{
		qoff.push_back(qoff.back() + qlen), toff.push_back(toff.back() + tlen), cig.push_back(cig.back() + qlen + tlen + 2);
		w.push_back(w_);
	}
};

#define REQUIRE(cond, ...)                                          \
	do {                                                            \
		if (!(cond)) {                                              \
			fprintf(stderr, "%s: %s -- ", name, #cond);             \
			fprintf(stderr, __VA_ARGS__), fprintf(stderr, "\n");    \
			exit(1);                                                \
		}                                                           \
	} while (0)

static void plan(GdPlan &P, std::vector<KswTask> &T, const GdPlanOpt &O, const Batch &B)
{
	T.assign((size_t)B.n(), KswTask());
	gd_plan_batch(P, O, B.n(), B.qoff.data(), B.toff.data(), B.w.data(), B.cig.data(), nullptr, T.data(), [](int n_sl, auto f) { for (int sl = 0; sl < n_sl; ++sl) f(sl); }, [](const char *) {});
}

// the kernel's claim on the host: launches over the boxes still pending, in a fresh random order each, until none is left
static int model_launches(std::vector<size_t> need /* bytes per pending box */, size_t arena, int give_up)
{
	int launches = 0;
	while (!need.empty() && launches < give_up) {
		for (size_t i = need.size(); i > 1; --i) std::swap(need[i - 1], need[rnd((uint32_t)i)]);
		std::vector<size_t> left;
		uint64_t counter = 0; // (units of 256 bytes, as the kernel's)
		for (size_t f : need) {
			const uint64_t at = counter, units = f >> 8;
			counter += units; // the atomic add happens whether the claim fits or not
			if (at + units > (arena >> 8)) left.push_back(f);
		}
		need.swap(left), ++launches;
	}
	return need.empty() ? launches : give_up + 1;
}

static void run(const char *name, const Batch &B, int64_t overflow_bytes, bool single_affine = false)
{
	GdPlanOpt full, O;
	full.single_affine = O.single_affine = single_affine;
	O.compact = true, O.overflow_bytes = overflow_bytes;
	GdPlan PF, P;
	std::vector<KswTask> TF, T;
	plan(PF, TF, full, B), plan(P, T, O, B);
	const int n = B.n();
	REQUIRE(PF.err == 0 && P.err == 0, "err %d / %d", PF.err, P.err);
	// ---- without the option: today's layout, no pool, no drain launch -------------------------------------------------------------------
	REQUIRE(PF.pool_bytes == 0 && PF.pool_off == 0 && PF.n_drain == 0 && PF.n_compact == 0, "full-size layout with a pool");
	size_t at = 0;
	for (int i = 0; i < n; ++i) {
		REQUIRE((size_t)TF[i].bt_off == at, "full-size layout: task %d at %lld, expected %zu", i, (long long)TF[i].bt_off, at);
		at += gd_align256((size_t)(TF[i].qlen + TF[i].tlen - 1) * (size_t)TF[i].row_bytes + 64); // (no wide-band box in these batches)
	}
	REQUIRE(PF.bt == at, "full-size layout: arena %zu, expected %zu", PF.bt, at);
	// ---- the compact layout ---------------------------------------------------------------------------------------------------------
	size_t n_try = 0, full_total = 0, full_max = 0;
	std::vector<size_t> need;
	at = 0;
	for (int i = 0; i < n; ++i) {
		const KswTask &A = T[i];
		REQUIRE(A.kind == TF[i].kind && A.row_bytes == TF[i].row_bytes && A.pad == TF[i].pad, "task %d: kind / rows / mark depend on the layout", i);
		REQUIRE(A.bt_off >= 0 && A.bt_off % 256 == 0 && (size_t)A.bt_off == at, "task %d: slot at %lld, the one before ends at %zu", i, (long long)A.bt_off, at);
		const size_t full_slot = gd_align256((size_t)(A.qlen + A.tlen - 1) * (size_t)A.row_bytes + 64);
		const size_t end = i + 1 < n ? (size_t)T[i + 1].bt_off : P.pool_off ? P.pool_off : P.bt;
		if (A.kind == GD_KIND_WAVE64 && A.pad == GD_NARROW_TRY) {
			REQUIRE(A.row_bytes == 1024 && full_slot == (size_t)gd_full_units(A.qlen, A.tlen) << 8, "task %d: the kernel claims %u units for a slot of %zu bytes", i, gd_full_units(A.qlen, A.tlen), full_slot);
			REQUIRE((size_t)A.bt_off + (size_t)(A.qlen + A.tlen - 1) * 512 <= end && end - (size_t)A.bt_off < full_slot, "task %d: slot of %zu bytes", i, end - (size_t)A.bt_off);
			++n_try, full_total += full_slot, full_max = std::max(full_max, full_slot), need.push_back(full_slot);
		} else REQUIRE(end - (size_t)A.bt_off == full_slot, "task %d (mark %d): slot of %zu bytes, full size %zu", i, A.pad, end - (size_t)A.bt_off, full_slot);
		at = end;
	}
	REQUIRE(P.n_compact == n_try && P.full_total == full_total && P.full_max == full_max, "accounting: %zu boxes, %zu bytes, largest %zu", P.n_compact, P.full_total, P.full_max);
	if (n_try == 0) {
		REQUIRE(P.bt == PF.bt && P.pool_bytes == 0 && P.n_drain == 0, "no box tries the narrow band, yet the layouts differ");
		printf("%s n=%d try=0 bt=%zu full_bt=%zu pool=0 drain=0 model=0\n", name, n, P.bt, PF.bt);
		return;
	}
	REQUIRE(P.pool_off == at && P.pool_off % 256 == 0 && P.pool_bytes % 256 == 0, "pool at %zu, the last slot ends at %zu", P.pool_off, at);
	REQUIRE(P.bt == P.pool_off + P.pool_bytes, "arena %zu, slots %zu + pool %zu", P.bt, P.pool_off, P.pool_bytes);
	if (overflow_bytes >= 0) REQUIRE(P.pool_bytes == std::max(gd_align256((size_t)overflow_bytes), P.full_max > P.pool_off ? P.full_max - P.pool_off : 0), "pool of %zu bytes for %lld asked", P.pool_bytes, (long long)overflow_bytes);
	else REQUIRE(P.pool_bytes == std::max(std::max(gd_align256(P.pool_off / 16), std::min(P.full_total, (size_t)64 << 20)), P.full_max > P.pool_off ? P.full_max - P.pool_off : 0),
	             "default pool of %zu bytes behind %zu", P.pool_bytes, P.pool_off);
	REQUIRE(P.bt >= P.full_max && P.n_drain >= 1 && (size_t)P.n_drain <= n_try, "arena %zu, largest box %zu, %d drain launches", P.bt, P.full_max, P.n_drain);
	// ---- the claim: every box falls back, nothing found room in the pool; drain launches over the whole arena -----------------------------
	int worst = 0;
	for (int rep = 0; rep < 24; ++rep) worst = std::max(worst, model_launches(need, P.bt, P.n_drain));
	{ // ... and two orders that are hard on it: largest first, smallest first
		std::vector<size_t> s = need;
		std::sort(s.begin(), s.end());
		for (int dir = 0; dir < 2; ++dir) {
			std::vector<size_t> left = s;
			int launches = 0;
			while (!left.empty() && launches <= P.n_drain) {
				std::vector<size_t> next;
				uint64_t counter = 0;
				for (size_t k = 0; k < left.size(); ++k) {
					const size_t f = dir ? left[left.size() - 1 - k] : left[k];
					const uint64_t a0 = counter;
					counter += f >> 8;
					if (a0 + (f >> 8) > (P.bt >> 8)) next.push_back(f);
				}
				std::sort(next.begin(), next.end());
				left.swap(next), ++launches;
			}
			worst = std::max(worst, left.empty() ? launches : P.n_drain + 1);
		}
	}
	REQUIRE(worst <= P.n_drain, "%d drain launches planned, an order of the claims needed more", P.n_drain);
	printf("%s n=%d try=%zu bt=%zu full_bt=%zu pool=%zu drain=%d model=%d\n", name, n, n_try, P.bt, PF.bt, P.pool_bytes, P.n_drain, worst);
}

int main()
{
	// HiFi boxes at w = 1000: whole reads and the short boxes between anchors; some with the lengths too far apart to try the narrow band
	// (mark NO), some at bands of their own up to GD_W_NARROW (mark OWN), some short reads (the grouped kernels)
	for (int b = 0; b < 12; ++b) {
		Batch B;
		const int n = b < 2 ? 1 + b : between(3, 1500);
		for (int i = 0; i < n; ++i) {
			const uint32_t c = b < 2 ? 0 : rnd(16); // (the batches of one and two boxes: boxes that try the narrow band)
			if (c < 9) { const int q = between(600, 26000); B.add(q, q + between(-200, 200), 1000); }
			else if (c < 11) { const int q = between(3000, 20000); B.add(q, q + between(500, 900) * (rnd(2) ? 1 : -1), 1000); }
			else if (c < 13) { const int q = between(1000, 20000); B.add(q, q + between(-60, 60), between(300, 495)); }
			else if (c < 15) { const int q = between(400, 3000); B.add(q, q + between(-30, 30), 1000); }
			else B.add(150, 150, 150);
		}
		char name[32];
		snprintf(name, sizeof name, "hifi%d", b);
		run(name, B, b % 3 == 0 ? 0 : b % 3 == 1 ? -1 : (int64_t)between(1, 64) << 20);
	}
	{ // one box, two equal boxes, pool 0: the pool grows to what the drain launch needs for the largest
		Batch B1, B2;
		B1.add(15000, 15010, 1000);
		B2.add(9000, 9000, 1000), B2.add(9000, 9000, 1000);
		run("one", B1, 0), run("two", B2, 0);
	}
	{ // 24 equal boxes, pool 0: the arena is half of what they need
		Batch B;
		for (int i = 0; i < 24; ++i) B.add(4000, 4100, 1000);
		run("twentyfour", B, 0);
	}
	{ // no box tries the narrow band: short reads; a single-affine batch
		Batch S, H;
		for (int i = 0; i < 500; ++i) S.add(150, 150, 150);
		for (int i = 0; i < 50; ++i) H.add(8000, 8000, 1000);
		run("short", S, -1), run("single", H, -1, true);
	}
	return 0;
}
