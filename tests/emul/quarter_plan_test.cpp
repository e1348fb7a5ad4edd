// CPU test of the quarter form's admission, of the rung the kernel decides on and of the auto mode (ksw_wave_core.h "the quarter form",
// ksw_plan.h "auto mode of the quarter rung").
//   1. GD_W_QUARTER is the widest band whose rows fit 16 blocks for every geometry.
//   2. gd_quarter_supported (O(1), the form the kernel evaluates) against its loop form on random geometries, and every admitted geometry
//      against what the quarter-block rows need anti-diagonal by anti-diagonal (gd_quarter_rows_ok).
//   3. gd_quarter_rung on the planner's marks of the hifi / own / mix batches of narrow_plan_test.cpp, against its definition in loop form.
//   4. gd_quarter_auto_offer / _update: stops below break-even, probes again, ignores launches with fewer than 64 tries.
// prints "w_quarter <W> cases <n> admitted <a> differ <d> rows_checked <k> rows_bad <b>", "rung <name> n=.. at239=.. own=.. none=.." and "auto ok"
#define __host__
#define __device__
#include <stdio.h>
#include <stdlib.h>
#include "ksw_plan.h"

static uint64_t rng_state = 20261018;
static uint32_t rnd(uint32_t n)
{
	rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
	return (uint32_t)((rng_state >> 33) % n);
}
static int between(int lo, int hi) { return lo + (int)rnd((uint32_t)(hi - lo + 1)); }

struct Batch {
	std::vector<int64_t> qoff{0}, toff{0}, cig{0};
	std::vector<int32_t> w;
	void add(int qlen, int tlen, int w_)
	{
		qoff.push_back(qoff.back() + qlen), toff.push_back(toff.back() + tlen), cig.push_back(cig.back() + qlen + tlen + 2);
		w.push_back(w_);
	}
};

static int rungs_and_check(const char *name, const Batch &B)
{
	const int n = (int)B.w.size();
	std::vector<KswTask> T((size_t)n);
	GdPlan P;
	gd_plan_batch(P, GdPlanOpt(), n, B.qoff.data(), B.toff.data(), B.w.data(), B.cig.data(), nullptr, T.data(), [](int n_sl, auto f) { for (int sl = 0; sl < n_sl; ++sl) f(sl); }, [](const char *) {});
	if (P.err) { fprintf(stderr, "%s: plan error %d\n", name, P.err); return 1; }
	long n_239 = 0, n_own = 0, n_none = 0;
	for (int i = 0; i < n; ++i) {
		const KswTask &A = T[i];
		const int w = A.w < 0 ? std::max(A.qlen, A.tlen) : A.w, delta = A.tlen - A.qlen;
		int want = 0;
		if (A.pad != GD_NARROW_NO) {
			if (w <= GD_W_QUARTER) want = A.pad == GD_NARROW_OWN && gd_quarter_supported_loop(A.qlen, A.tlen, w) ? w : 0;
			else want = abs(delta) <= GD_W_QUARTER && gd_quarter_supported_loop(A.qlen, A.tlen, GD_W_QUARTER) ? GD_W_QUARTER : 0;
		}
		const int got = gd_quarter_rung(A.pad, A.qlen, A.tlen, w, GD_W_QUARTER);
		if (got != want) { fprintf(stderr, "%s: task %d (%d x %d, w %d, mark %d): rung %d, expected %d\n", name, i, A.qlen, A.tlen, A.w, A.pad, got, want); return 1; }
		if (gd_quarter_rung(A.pad, A.qlen, A.tlen, w, 0) != 0) { fprintf(stderr, "%s: task %d: a rung although none is offered\n", name, i); return 1; }
		if (got && !gd_quarter_rows_ok(A.qlen, A.tlen, got)) { fprintf(stderr, "%s: task %d: the rows at band %d\n", name, i, got); return 1; }
		// what the certificate of the rung needs: the corner inside the band
		if (got && abs(delta) > got) { fprintf(stderr, "%s: task %d: corner outside the rung's band\n", name, i); return 1; }
		n_239 += got == GD_W_QUARTER && w > GD_W_QUARTER, n_own += got && w <= GD_W_QUARTER, n_none += !got;
	}
	printf("rung %s n=%d at239=%ld own=%ld none=%ld\n", name, n, n_239, n_own, n_none);
	return 0;
}

static int auto_mode()
{
	GdQuarterAuto A;
	auto fail = [](const char *what) { fprintf(stderr, "auto mode: %s\n", what); return 1; };
	// offered from the start, and for as long as the boxes certify (or too few tried to tell)
	for (int i = 0; i < 40; ++i) {
		if (!gd_quarter_auto_offer(A)) return fail("not offered although nothing spoke against it");
		if (i % 3 == 0) gd_quarter_auto_update(A, 5000, 4990);
		else if (i % 3 == 1) gd_quarter_auto_update(A, GD_QUARTER_AUTO_MIN - 1, 0); // fewer than 64 tries: ignored
		else gd_quarter_auto_update(A, 0, 0);
	}
	// exactly at break-even it stays on; one box below, it stops
	const uint64_t tried = 100 * GD_QUARTER_BREAK_EVEN_DEN, even = 100 * GD_QUARTER_BREAK_EVEN_NUM;
	gd_quarter_auto_update(A, tried, even);
	if (!gd_quarter_auto_offer(A)) return fail("stopped at break-even");
	gd_quarter_auto_update(A, tried, even - 1);
	for (int i = 0; i < GD_QUARTER_AUTO_HOLD; ++i) {
		if (gd_quarter_auto_offer(A)) return fail("offered during the hold");
		gd_quarter_auto_update(A, 0, 0); // (a launch that did not offer the rung has no tries)
	}
	if (!gd_quarter_auto_offer(A)) return fail("no probe after the hold");
	gd_quarter_auto_update(A, 5000, 100); // the probe fails: another hold
	for (int i = 0; i < GD_QUARTER_AUTO_HOLD; ++i)
		if (gd_quarter_auto_offer(A)) return fail("offered during the second hold");
	if (!gd_quarter_auto_offer(A)) return fail("no second probe");
	gd_quarter_auto_update(A, 5000, 4000); // the probe succeeds: on for good
	for (int i = 0; i < 40; ++i) {
		if (!gd_quarter_auto_offer(A)) return fail("off after a good probe");
		gd_quarter_auto_update(A, 5000, 4000);
	}
	if (!(0 < GD_QUARTER_BREAK_EVEN_NUM && GD_QUARTER_BREAK_EVEN_NUM < GD_QUARTER_BREAK_EVEN_DEN)) return fail("break-even is not a share");
	printf("auto ok break_even %d/%d min %d hold %d\n", GD_QUARTER_BREAK_EVEN_NUM, GD_QUARTER_BREAK_EVEN_DEN, GD_QUARTER_AUTO_MIN, GD_QUARTER_AUTO_HOLD);
	return 0;
}

int main(int argc, char **argv)
{
	const long n_it = argc > 1 ? atol(argv[1]) : 300000;
	// 1. the constant
	int wmax = 0;
	for (int w = 1; w < 2000; ++w) {
		bool fits = true;
		for (int ln : {w + 1, 2 * w, 5000, 100000}) fits = fits && gd_ncol16(ln, ln, w) <= 16 && ((w + 16) >> 4) + 1 <= 16;
		if (fits) wmax = w;
	}
	// 2. the two forms of the admission test; the rows of what it admits
	long n = 0, ok = 0, diff = 0, rows = 0, rows_bad = 0;
	for (long it = 0; it < n_it; ++it) {
		const int w = it % 3 == 0 ? GD_W_QUARTER - (int)rnd(3) : it % 3 == 1 ? 1 + (int)rnd(GD_W_QUARTER + 40) : 1 + (int)rnd(120);
		const int lmax = it % 5 == 0 ? 300 : it % 5 == 1 ? 6000 : it % 5 == 2 ? 40000 : it % 5 == 3 ? 1200 : 2000;
		int qlen = 1 + (int)rnd(lmax), tlen = qlen + (int)rnd(2 * w + 40) - w - 20;
		if (rnd(5) == 0) tlen = 1 + (int)rnd(lmax);
		if (rnd(9) == 0) tlen = qlen + (int)rnd(5) - 2;
		if (tlen < 1) tlen = 1;
		const bool a = gd_quarter_supported_loop(qlen, tlen, w), b = gd_quarter_supported(qlen, tlen, w);
		++n, ok += a;
		if (a != b) {
			if (diff < 5) fprintf(stderr, "DIFF qlen %d tlen %d w %d: loop %d fast %d\n", qlen, tlen, w, (int)a, (int)b);
			++diff;
		}
		// the rung of a box at its own band up to GD_W_QUARTER (called directly: today's planner gives every geometry admitted to 16 blocks
		// to the grouped kernels, so no box of the 64-lane kernel carries such a mark)
		if (w <= GD_W_QUARTER && (gd_quarter_rung(GD_NARROW_OWN, qlen, tlen, w, GD_W_QUARTER) != (a ? w : 0) || gd_quarter_rung(GD_NARROW_TRY, qlen, tlen, w, GD_W_QUARTER) != 0 ||
		                          gd_quarter_rung(GD_NARROW_NO, qlen, tlen, w, GD_W_QUARTER) != 0)) ++diff;
		if (b && qlen + tlen < 9000 && it % 4 == 0) {
			++rows;
			if (!gd_quarter_rows_ok(qlen, tlen, w)) {
				if (rows_bad < 5) fprintf(stderr, "ROWS qlen %d tlen %d w %d admitted, but the rows do not fit\n", qlen, tlen, w);
				++rows_bad;
			}
		}
	}
	printf("w_quarter %d cases %ld admitted %ld differ %ld rows_checked %ld rows_bad %ld\n", wmax, n, ok, diff, rows, rows_bad);
	if (wmax != GD_W_QUARTER || diff || rows_bad) return 1;
	// 3. the rung, on the batches of narrow_plan_test.cpp
	Batch hifi, own, mix;
	for (int i = 0; i < 3000; ++i) {
		const int q = between(600, 20000);
		hifi.add(q, q + between(-60, 60), 1000);
	}
	for (int i = 0; i < 3000; ++i) {
		const int q = between(1000, 20000);
		own.add(q, q + between(-60, 60), between(300, GD_W_NARROW));
	}
	for (int i = 0; i < 6000; ++i) {
		const uint32_t c = rnd(8);
		const int q = between(700, 16000);
		if (c == 0) mix.add(q, q + between(-GD_W_NARROW - 30, GD_W_NARROW + 30), 1000);        // lengths further apart than either narrow band
		else if (c == 1) mix.add(q, q + between(-250, 250), between(1250, 1330));                 // wide bands: another kernel
		else if (c == 2) mix.add(between(100, 150), between(100, 150), 150);                       // short reads
		else if (c == 3) mix.add(q, q + between(-3, 3), between(GD_W_NARROW - 2, GD_W_NARROW + 2)); // around the constant
		else if (c == 4) mix.add(q, q + between(-40, 40), between(200, 700));
		else if (c == 5) mix.add(q, q + between(-3, 3), between(GD_W_QUARTER - 2, GD_W_QUARTER + 2)); // around the quarter constant
		else if (c == 6) mix.add(q, q + between(-GD_W_QUARTER - 3, GD_W_QUARTER + 3), 1000);           // lengths around it apart
		else mix.add(q, q + between(-60, 60), 1000);
	}
	if (rungs_and_check("hifi", hifi) || rungs_and_check("own", own) || rungs_and_check("mix", mix)) return 1;
	// 4. auto mode
	return auto_mode();
}
