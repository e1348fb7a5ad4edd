// CPU test of the narrow form's admission and of the planner's marks (ksw_wave_core.h "the narrow form", ksw_plan.h).
//   1. GD_W_NARROW is the widest band whose rows fit 32 blocks for every geometry.
//   2. gd_narrow_supported (O(1)) against its loop form on random geometries, and every admitted geometry against what the half-block rows
//      need anti-diagonal by anti-diagonal (gd_narrow_rows_ok).
//   3. gd_plan_batch: which boxes are marked GD_NARROW_TRY / GD_NARROW_OWN, and the arena -- every slot still holds the full-band rows.
// prints "w_narrow <W> cases <n> admitted <a> differ <d> rows_checked <k> rows_bad <b>" and "plan <name> n=.. try=.. own=.. no=.. bt=.."
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

static int plan_and_check(const char *name, const GdPlanOpt &O, const Batch &B)
{
	const int n = (int)B.w.size();
	std::vector<KswTask> T((size_t)n);
	GdPlan P;
	gd_plan_batch(P, O, n, B.qoff.data(), B.toff.data(), B.w.data(), B.cig.data(), nullptr, T.data(), [](int n_sl, auto f) { for (int sl = 0; sl < n_sl; ++sl) f(sl); }, [](const char *) {});
	if (P.err) { fprintf(stderr, "%s: plan error %d\n", name, P.err); return 1; }
	long n_try = 0, n_own = 0, n_no = 0;
	size_t bt = 0;
	for (int i = 0; i < n; ++i) {
		const KswTask &A = T[i];
		const int w = A.w < 0 ? std::max(A.qlen, A.tlen) : A.w, delta = A.tlen - A.qlen;
		int want = GD_NARROW_NO;
		if (A.kind == GD_KIND_WAVE64 && !O.single_affine) {
			if (w > GD_W_NARROW && abs(delta) <= GD_W_NARROW && gd_narrow_supported_loop(A.qlen, A.tlen, GD_W_NARROW)) want = GD_NARROW_TRY;
			if (w <= GD_W_NARROW && gd_narrow_supported_loop(A.qlen, A.tlen, w)) want = GD_NARROW_OWN;
		}
		if (A.pad != want) { fprintf(stderr, "%s: task %d (%d x %d, w %d, kind %d) marked %d, expected %d\n", name, i, A.qlen, A.tlen, A.w, A.kind, A.pad, want); return 1; }
		if (A.pad == GD_NARROW_TRY && !gd_narrow_rows_ok(A.qlen, A.tlen, GD_W_NARROW)) { fprintf(stderr, "%s: task %d: the rows at the narrow band\n", name, i); return 1; }
		if (A.pad == GD_NARROW_OWN && !gd_narrow_rows_ok(A.qlen, A.tlen, w)) { fprintf(stderr, "%s: task %d: the rows at its own band\n", name, i); return 1; }
		n_try += A.pad == GD_NARROW_TRY, n_own += A.pad == GD_NARROW_OWN, n_no += A.pad == GD_NARROW_NO;
		// the arena as before: rows of 64 blocks for every alignment of the 64-lane kernel, marked or not
		if (A.kind == GD_KIND_WAVE64 && A.row_bytes != 1024) { fprintf(stderr, "%s: task %d: rows of %d bytes\n", name, i, A.row_bytes); return 1; }
		if ((size_t)A.bt_off != bt) { fprintf(stderr, "%s: task %d: bt_off %lld, expected %zu\n", name, i, (long long)A.bt_off, bt); return 1; }
		if (!(P.wide_ck && A.kind == GD_KIND_WAVE128)) bt += gd_align256((size_t)(A.qlen + A.tlen - 1) * (size_t)A.row_bytes + 64);
		else bt += gd_align256(gd_ck_bytes(A.qlen, A.tlen, A.row_bytes) + 64);
	}
	if (bt != P.bt) { fprintf(stderr, "%s: arena %zu, expected %zu\n", name, P.bt, bt); return 1; }
	printf("plan %s n=%d try=%ld own=%ld no=%ld bt=%zu\n", name, n, n_try, n_own, n_no, P.bt);
	return 0;
}

int main(int argc, char **argv)
{
	const long n_it = argc > 1 ? atol(argv[1]) : 300000;
	// 1. the constant
	int wmax = 0;
	for (int w = 1; w < 2000; ++w) {
		bool fits = true;
		for (int ln : {w + 1, 2 * w, 5000, 100000}) fits = fits && gd_ncol16(ln, ln, w) <= 32;
		if (fits) wmax = w;
	}
	// 2. the two forms of the admission test; the rows of what it admits
	long n = 0, ok = 0, diff = 0, rows = 0, rows_bad = 0;
	for (long it = 0; it < n_it; ++it) {
		const int w = it % 3 == 0 ? GD_W_NARROW - (int)rnd(3) : it % 3 == 1 ? 1 + (int)rnd(GD_W_NARROW + 40) : 1 + (int)rnd(120);
		const int lmax = it % 5 == 0 ? 300 : it % 5 == 1 ? 6000 : it % 5 == 2 ? 40000 : it % 5 == 3 ? 1200 : 2000;
		int qlen = 1 + (int)rnd(lmax), tlen = qlen + (int)rnd(2 * w + 40) - w - 20;
		if (rnd(5) == 0) tlen = 1 + (int)rnd(lmax);
		if (rnd(9) == 0) tlen = qlen + (int)rnd(5) - 2;
		if (tlen < 1) tlen = 1;
		const bool a = gd_narrow_supported_loop(qlen, tlen, w), b = gd_narrow_supported(qlen, tlen, w);
		++n, ok += a;
		if (a != b) {
			if (diff < 5) fprintf(stderr, "DIFF qlen %d tlen %d w %d: loop %d fast %d\n", qlen, tlen, w, (int)a, (int)b);
			++diff;
		}
		if (b && qlen + tlen < 9000 && it % 4 == 0) {
			++rows;
			if (!gd_narrow_rows_ok(qlen, tlen, w)) {
				if (rows_bad < 5) fprintf(stderr, "ROWS qlen %d tlen %d w %d admitted, but the rows do not fit\n", qlen, tlen, w);
				++rows_bad;
			}
		}
		if (w <= GD_W_NARROW && b != (gd_narrow_mode(qlen, tlen, w) == GD_NARROW_OWN)) ++diff;
	}
	printf("w_narrow %d cases %ld admitted %ld differ %ld rows_checked %ld rows_bad %ld\n", wmax, n, ok, diff, rows, rows_bad);
	if (wmax != GD_W_NARROW || diff || rows_bad) return 1;
	// 3. the planner
	GdPlanOpt root;
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
		if (c == 0) mix.add(q, q + between(-GD_W_NARROW - 30, GD_W_NARROW + 30), 1000);        // lengths further apart than the narrow band
		else if (c == 1) mix.add(q, q + between(-250, 250), between(1250, 1330));                 // wide bands: another kernel
		else if (c == 2) mix.add(between(100, 150), between(100, 150), 150);                       // short reads
		else if (c == 3) mix.add(q, q + between(-3, 3), between(GD_W_NARROW - 2, GD_W_NARROW + 2)); // around the constant
		else if (c == 4) mix.add(q, q + between(-40, 40), between(200, 700));
		else mix.add(q, q + between(-60, 60), 1000);
	}
	if (plan_and_check("hifi", root, hifi) || plan_and_check("own", root, own) || plan_and_check("mix", root, mix)) return 1;
	GdPlanOpt single = root;
	single.single_affine = true;
	if (plan_and_check("hifi_single", single, hifi)) return 1;
	return 0;
}
