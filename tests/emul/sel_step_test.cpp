// The two-lane update of the score selectors in the paired steady rows of the quarter-block and half-block forms (gdw_quarter_rows,
// gdw_narrow_rows in ksw_wave.hip.h; gdw_sel_step_quarter / gdw_sel_step_half in ksw_wave_core.h).  64 emulated lanes keep what the
// selectors depend on -- (blk, quarter | half, SEL, m_lowest) -- through the device's row loop with its statements: general rows, the
// paired rows with every lane making its selectors on the first pair, on a pair that takes a block over and in a band whose two rows
// differ in `up`, two lanes patched on every other pair, general rows again.  After the first row of EVERY pair, and after every general row that keeps the selectors of the row before, every lane is compared with what
// gdw_make_sel_quarter / gdw_make_sel_half give outright for that row's window and with the
// m_lowest expression; a patch must also leave the lane's other selector dword what it was.
//
//   g++ -O2 -I genome-on-diet_amd/csrc tests/emul/sel_step_test.cpp -o sel_step_test && ./sel_step_test
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#define __host__
#define __device__
#include "ksw_wave_core.h"

struct Counts { long geoms = 0, full = 0, patched = 0, rows = 0, wraps = 0; };

struct Lane { int blk, sub; u32 sel[2]; }; // what a lane's selectors depend on, and the selectors
struct QuarterForm {
	static constexpr int SUBS = 4, RING = 16, NW = 1;
	static void make(int blk, int sub, int st0, int up, u32 out[2]) // gdw_make_sel_quarter for the lane holding (blk, sub)
	{
		WaveQuarter T;
		T.blk = blk, T.quarter = sub;
		gdw_make_sel_quarter(T, st0, up);
		out[0] = T.SEL, out[1] = 0;
	}
	static GdwSelStep step(int m, int w) { return gdw_sel_step_quarter(m, w); }
	static bool admitted(int qlen, int tlen, int w) { return w <= GD_W_QUARTER && gd_quarter_supported(qlen, tlen, w); }
};
struct HalfForm {
	static constexpr int SUBS = 2, RING = 32, NW = 2;
	static void make(int blk, int sub, int st0, int up, u32 out[2]) // gdw_make_sel_half
	{
		WaveHalf T;
		T.blk = blk, T.half = sub;
		gdw_make_sel_half(T, st0, up);
		out[0] = T.SEL[0], out[1] = T.SEL[1];
	}
	static GdwSelStep step(int m, int w) { return gdw_sel_step_half(m, w); }
	static bool admitted(int qlen, int tlen, int w) { return w <= GD_W_NARROW && gd_narrow_supported(qlen, tlen, w); }
};

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "  (qlen %d tlen %d w %d)\n", qlen, tlen, w); exit(2); } while (0)

template <class F> static void run(int qlen, int tlen, int w, Counts &C)
{
	const int rend = qlen + tlen - 2;
	Lane H[64];
	u32 m_lowest[64] = {0};
	for (int l = 0; l < 64; ++l) {
		H[l].blk = l / F::SUBS, H[l].sub = l % F::SUBS;
		H[l].sel[0] = 0x03020100u, H[l].sel[1] = F::NW > 1 ? 0x03020100u : 0u; // (gdw_load_quarter / gdw_load_half)
	}
	int prev_st_ = 0, prev_st0 = -1, prev_up = -1;
	auto take_over = [&](int st_, int r) {
		for (int l = 0; l < 64; ++l)
			if (H[l].blk < st_) {
				H[l].blk += F::RING;
				for (int g = 0; g < F::NW; ++g) H[l].sel[g] = 0x03020100u;
				if (H[l].blk < st_) FAIL("row %d lane %d: still below the window after taking a block over\n", r, l);
			}
	};
	auto check = [&](int st0, int up, int r, const char *what) { // every lane against the selectors made outright
		for (int l = 0; l < 64; ++l) {
			u32 out[2];
			F::make(H[l].blk, H[l].sub, st0, up, out);
			for (int g = 0; g < F::NW; ++g)
				if (out[g] != H[l].sel[g]) FAIL("%s row %d lane %d dword %d: holds %08x, outright %08x\n", what, r, l, g, H[l].sel[g], out[g]);
		}
	};
	auto dp_row = [&](const int r) { // the selector statements of the device's dp_row
		int st0, en0;
		gd_band(r, qlen, tlen, w, st0, en0);
		const int st_ = st0 >> 4, up = st0 + (((en0 - st0 + 16) >> 4) << 4);
		const int advanced = st_ > prev_st_;
		if (advanced) take_over(st_, r);
		if (st0 != prev_st0 || up != prev_up || advanced)
			for (int l = 0; l < 64; ++l) F::make(H[l].blk, H[l].sub, st0, up, H[l].sel);
		else check(st0, up, r, "general"); // (selectors carried over from the row before, the last paired row included)
		prev_st_ = st_, prev_st0 = st0, prev_up = up;
	};
	const int nblkA = (w - 1 + 16) >> 4, nblkB = (w + 16) >> 4;
	const int step_mask = nblkA == nblkB ? 15 : 0;
	int m_full = 0;
	auto pair_row = [&](const int r, const int m, const bool ROW_A) { // ... and of its pair_row
		const int st0 = m, en0 = ROW_A ? m + w - 1 : m + w, st_ = m >> 4, up = m + ((ROW_A ? nblkA : nblkB) << 4);
		{
			int s, e;
			gd_band(r, qlen, tlen, w, s, e);
			if (s != st0 || e != en0 || up != s + (((e - s + 16) >> 4) << 4)) FAIL("pair row %d: band mismatch\n", r);
		}
		const int advanced = ROW_A && (m & 15) == 0;
		const int pst_ = (m - (ROW_A ? 1 : 0)) >> 4;
		if (pst_ != prev_st_ || pst_ != st_ - advanced) FAIL("pair row %d: pst_ %d, prev_st_ %d\n", r, pst_, prev_st_);
		if (ROW_A) // (the mask the query shift uses is that of the row before; on a second row that is the first row's, checked below)
			for (int l = 0; l < 64; ++l)
				if (m_lowest[l] != ((H[l].blk == pst_ && H[l].sub == 0) ? ~0u : 0u)) FAIL("pair row %d lane %d: stale lowest-block mask for the query shift\n", r, l);
		if (advanced) take_over(st_, r);
		if (ROW_A ? (m & step_mask) == 0 || m == m_full : nblkA != nblkB) {
			for (int l = 0; l < 64; ++l) {
				F::make(H[l].blk, H[l].sub, st0, up, H[l].sel);
				m_lowest[l] = (H[l].blk == st_ && H[l].sub == 0) ? ~0u : 0u;
			}
			if (ROW_A) ++C.full;
		} else if (ROW_A) {
			const GdwSelStep S = F::step(m, w);
			if (S.lane[0] == S.lane[1]) FAIL("pair row %d: one lane patched twice\n", r);
			for (int k = 0; k < 2; ++k) {
				if (S.lane[k] < 0 || S.lane[k] > 63 || S.word[k] < 0 || S.word[k] >= F::NW) FAIL("pair row %d: lane %d dword %d\n", r, S.lane[k], S.word[k]);
				Lane &L = H[S.lane[k]];
				for (int g = 0; g < F::NW; ++g) {
					if (g != S.word[k] && S.sel[k][g] != L.sel[g]) FAIL("pair row %d lane %d: the other dword would change, %08x -> %08x\n", r, S.lane[k], L.sel[g], S.sel[k][g]);
					L.sel[g] = S.sel[k][g]; // v_writelane_b32
				}
			}
			++C.patched;
		}
		if (ROW_A) check(st0, up, r, "pair"); // (a second row either makes them outright or has the first row's window and touches nothing)
		else if (nblkA == nblkB && (st0 != prev_st0 || up != prev_up)) FAIL("pair row %d: the window moves on a second row\n", r);
		if (ROW_A)
			for (int l = 0; l < 64; ++l)
				if (m_lowest[l] != ((H[l].blk == st_ && H[l].sub == 0) ? ~0u : 0u)) FAIL("pair row %d lane %d: lowest-block mask\n", r, l);
		prev_st_ = st_, prev_st0 = st0, prev_up = up;
	};
	int rA, rS;
	gdw_steady_rows(qlen, tlen, w, rA, rS);
	int r = 0;
	for (; r <= rend && r < rA; ++r) dp_row(r);
	if (r == rA && rS > rA) {
		int m = (rA - w + 1) >> 1;
		m_full = m;
		for (int l = 0; l < 64; ++l) m_lowest[l] = (H[l].blk == prev_st_ && H[l].sub == 0) ? ~0u : 0u;
		const int m0 = m;
		for (; r < rS; r += 2, ++m) {
			pair_row(r, m, true);
			pair_row(r + 1, m, false);
		}
		--m;
		if (prev_st_ != m >> 4 || prev_st0 != m || prev_up != m + (nblkB << 4)) FAIL("band bookkeeping after the paired rows\n");
		C.wraps += ((m >> 4) - (m0 >> 4)) / F::RING;
	}
	for (; r <= rend; ++r) dp_row(r); // (the rows behind compare prev_st0 / prev_up: the patched selectors are handed back to them)
	C.rows += rend + 1, ++C.geoms;
}

template <class F> static int grid(const char *name, const int *bands, int nb)
{
	for (int b = 0; b < nb; ++b) {
		const int w = bands[b];
		Counts C;
		const int mods[] = {0, 1, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15}; // tlen on and next to every quarter and half boundary
		for (int mod : mods)
			for (int dk = 0; dk < 7; ++dk) {
				const int dabs = dk == 0 ? 0 : dk <= 2 ? 1 : dk <= 4 ? w - 1 : w, delta = (dk & 1) ? dabs : -dabs; // tlen - qlen
				// the length classes of quarter_emul / narrow_emul at both ends of what they draw from (around the band: w - 40 .. w + 39; the
				// band binds: w + 30 .. w + 229; paired rows: 2 w + 200 .. 2 w + 599, where the ring wraps once or twice) and 5 w + 700:
				// about ten times round the ring of 16 blocks, five times round the ring of 32
				const int bases[] = {w - 40, w + 39, w + 30, w + 229, 2 * w + 200, 2 * w + 599, 5 * w + 700};
				for (int lk = 0; lk < 7; ++lk) {
					int base = bases[lk];
					if (delta > 0 && lk >= 4) base += delta; // (the shorter of the two decides how long the paired rows run)
					int tlen = (base & ~15) + mod;
					if (tlen <= dabs + 20) tlen += (dabs + 36) & ~15;
					const int qlen = tlen - delta;
					if (qlen < 20 || !F::admitted(qlen, tlen, w)) continue;
					run<F>(qlen, tlen, w, C);
				}
			}
		printf("%s band %d geometries %ld rows %ld full_pairs %ld patched_pairs %ld ring_wraps %ld\n", name, w, C.geoms, C.rows, C.full, C.patched, C.wraps);
		if (!C.geoms) return 3;
	}
	return 0;
}

int main()
{
	// quarter blocks: the rung's band and next to it, 223 (one block fewer), the bands of the emulator's grid, own bands on both sides
	// of a multiple of 16 (224: the two rows of a pair differ in `up`, every pair makes its selectors)
	const int qbands[] = {239, 238, 237, 223, 224, 225, 119, 55};
	// half blocks: the same around 495; 479 / 480 / 481, 400 / 401, and the bands of the emulator's grid
	const int hbands[] = {495, 494, 479, 480, 481, 400, 401, 247, 119};
	int rc = grid<QuarterForm>("quarter", qbands, (int)(sizeof(qbands) / sizeof(int)));
	if (!rc) rc = grid<HalfForm>("half", hbands, (int)(sizeof(hbands) / sizeof(int)));
	if (!rc) printf("sel_step_test ok\n");
	return rc;
}
