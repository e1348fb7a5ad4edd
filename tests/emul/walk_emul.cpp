// Host emulator of the wavefront walks (gd_bt_wave_walk / gd_walk_rows in genome-on-diet_amd/csrc/ksw_backtrack.hip.h): 64 emulated lanes
// fetch the window of the diagonal the walk stands on, decode their byte, the "ballots" become the masks of ksw_walk_core.h and the shared
// gd_walk_window consumes them -- against the oracle's gdo_backtrack on the same backtrace in the reference's layout.  The matrices are
// SYNTHETIC bytes, not DP output, so that every branch of the state machine is reached: random directions and continuation bits, planted
// match runs of 1, 63, 64, 65, 127, 128, 129 cells ended by each of the four gap states, gaps longer than a window, gaps back to back,
// walks that start outside the stored window of their row, lengths 1..400 and bands 8, 50, 239, 1000 and -1.  Every matrix is walked in
// one piece and in chunks of 32 and 192 anti-diagonals (r0 stepping down, as the checkpointed kernels call gd_walk_rows), each with a
// CIGAR capacity of 0, 1, 3 and ample.  On matrices of direction 0 only the number of loop iterations is bounded, which the
// cell-at-a-time loop cannot meet.
//
//   g++ -O2 -I genome-on-diet_amd/csrc -I oracle tests/emul/walk_emul.cpp oracle/gdo_ksw2.c -o walk_emul
//   ./walk_emul <seed>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <random>
#define __host__
#define __device__
#include "ksw_walk_core.h"
#include "gdo_ksw2.h"

struct Matrix {
	int qlen, tlen, w, ncol; // w as the walks use it (-1 already replaced)
	std::vector<uint8_t> ref, dev; // the reference's bytes / the register-resident kernels' bytes, both at r * ncol * 16 + (i - off[r])
	std::vector<int> off, off_end;
};

// the reference's byte d | cX<<3 | cY<<4 | cX2<<5 | cY2<<6 -> the byte of the register-resident kernels, bit 3 random
static uint8_t encode(uint32_t t, uint32_t rnd)
{
	return (uint8_t)((4 - (t & 7)) | (rnd & 1) << 3 | (~t >> 6 & 1) << 4 | (~t >> 5 & 1) << 5 | (~t >> 4 & 1) << 6 | (~t >> 3 & 1) << 7);
}

static void make_matrix(std::mt19937 &g, Matrix &M, int qlen, int tlen, int w_arg, int p_plain /* direction 0 in p_plain of 1000 cells */)
{
	M.qlen = qlen, M.tlen = tlen, M.w = w_arg < 0 ? (tlen > qlen ? tlen : qlen) : w_arg;
	M.ncol = gd_ncol16(qlen, tlen, M.w);
	const int rows = qlen + tlen - 1;
	M.ref.assign((size_t)rows * M.ncol * 16, 0);
	M.off.resize(rows), M.off_end.resize(rows);
	for (int r = 0; r < rows; ++r) {
		int st0, en0;
		gd_band(r, qlen, tlen, M.w, st0, en0);
		M.off[r] = st0 & ~15, M.off_end[r] = en0 | 15;
		if (M.off_end[r] - M.off[r] >= M.ncol * 16) { fprintf(stderr, "row %d wider than n_col\n", r); exit(2); }
	}
	for (auto &b : M.ref) {
		const uint32_t x = g();
		const uint32_t d = (int)(x % 1000) < p_plain ? 0 : 1 + (x >> 10) % 4;
		b = (uint8_t)(d | (x >> 16 & 15) << 3);
	}
}

static uint8_t *cell(Matrix &M, int i, int j)
{
	static uint8_t outside;
	const int r = i + j;
	if (i < M.off[r] || i > M.off_end[r]) return &outside; // not stored: the walk's state is forced there
	return &M.ref[(size_t)r * M.ncol * 16 + (i - M.off[r])];
}

// writes, along the path it describes from the last cell, the bytes that make ksw_backtrack follow it (where the band stores the cells):
// `first` match cells, then gaps of the states 1..4 in turn, each after a match run of one of the lengths that matter to a 64-cell window
static void plant(std::mt19937 &g, Matrix &M, int first, bool back_to_back)
{
	static const int RUNS[7] = {1, 63, 64, 65, 127, 128, 129}, GAPS[6] = {1, 2, 5, 70, 130, 3};
	int i = M.tlen - 1, j = M.qlen - 1, prev = 0, s = 1 + g() % 4;
	int L = first;
	while (i >= 0 && j >= 0) {
		for (int n = 0; n < L && i >= 0 && j >= 0; ++n, --i, --j) { // a match run: direction 0, the gap before it not continued
			uint8_t *c = cell(M, i, j);
			*c = (uint8_t)((g() & 15) << 3);
			if (prev) *c &= (uint8_t)~(1u << (prev + 2));
			prev = 0;
		}
		const int glen = GAPS[g() % 6];
		for (int n = 0; n < glen && i >= 0 && j >= 0; ++n) {
			uint8_t *c = cell(M, i, j);
			if (n == 0) { // opens: the state before it not continued, direction s
				*c = (uint8_t)(s | (g() & 15) << 3);
				if (prev) *c &= (uint8_t)~(1u << (prev + 2));
			} else *c = (uint8_t)((g() % 5) | (g() & 15) << 3 | 1u << (s + 2)); // continued whatever the direction says
			prev = s;
			if (s == 1 || s == 3) --i; else --j;
		}
		s = s % 4 + 1;
		L = back_to_back && g() % 3 == 0 ? 0 : RUNS[g() % 7];
	}
}

static void finish_matrix(std::mt19937 &g, Matrix &M)
{
	M.dev.resize(M.ref.size());
	for (size_t k = 0; k < M.ref.size(); ++k) {
		M.dev[k] = encode(M.ref[k], g());
		if (gd_bt_decode(M.dev[k]) != M.ref[k]) { fprintf(stderr, "encode / gd_bt_decode disagree on %02x\n", M.ref[k]); exit(2); }
	}
}

// gd_walk_rows on 64 emulated lanes: the rows r >= r0 of the matrix are at hand
static long walk_rows(GdWalk &W, const Matrix &M, int r0, uint32_t *cg, int cap)
{
	long steps = 0;
	while (W.i >= 0 && W.j >= 0 && W.i + W.j >= r0) {
		GdWalkMasks B;
		memset(&B, 0, sizeof(B));
		for (int lane = 0; lane < 64; ++lane) {
			const int ik = W.i - lane, jk = W.j - lane;
			const bool inside = ik >= 0 && jk >= 0 && ik + jk >= r0;
			int fs = -1;
			uint32_t tmp = 0;
			if (inside) {
				const int r = ik + jk;
				int st0, en0;
				gd_band(r, M.qlen, M.tlen, M.w, st0, en0);
				const int off = st0 & ~15, off_end = en0 | 15;
				if (ik < off) fs = 2;
				if (ik > off_end) fs = 1;
				if (fs < 0) tmp = gd_bt_decode(M.dev[(size_t)r * M.ncol * 16 + (ik - off)]);
			}
			const uint64_t bit = 1ull << lane;
			if (inside) B.valid |= bit;
			if (fs == 1) B.f1 |= bit;
			if (fs == 2) B.f2 |= bit;
			if (tmp & 1) B.d0 |= bit;
			if (tmp & 2) B.d1 |= bit;
			if (tmp & 4) B.d2 |= bit;
			if (tmp & 0x08) B.c1 |= bit;
			if (tmp & 0x10) B.c2 |= bit;
			if (tmp & 0x20) B.c3 |= bit;
			if (tmp & 0x40) B.c4 |= bit;
		}
		const int n = gd_walk_window(W, cg, cap, true, B);
		if (n < 1) { fprintf(stderr, "a window consumed nothing\n"); exit(2); }
		steps += n;
	}
	return steps;
}

struct Emu { int nc; std::vector<uint32_t> ops; long steps; };
static Emu emulate(const Matrix &M, int chunk_rows /* 0: one piece */, int cap)
{
	Emu e;
	e.ops.assign(cap, 0xdeadbeefu); // exactly the capacity: a store past it is the sanitizer's
	e.steps = 0;
	GdWalk W;
	gd_walk_init(W, M.qlen, M.tlen);
	if (chunk_rows == 0) e.steps += walk_rows(W, M, 0, e.ops.data(), cap);
	else
		for (int k = (M.qlen + M.tlen - 2) / chunk_rows; k >= 0 && W.i >= 0 && W.j >= 0; --k) e.steps += walk_rows(W, M, k * chunk_rows, e.ops.data(), cap);
	e.nc = gd_walk_tail(W, e.ops.data(), cap, true);
	if (e.nc <= cap)
		for (int k = 0; k < e.nc >> 1; ++k) std::swap(e.ops[k], e.ops[e.nc - 1 - k]);
	return e;
}

int main(int argc, char **argv)
{
	const unsigned seed = argc > 1 ? atoi(argv[1]) : 1;
	std::mt19937 g(seed);
	const int bands[5] = {8, 50, 239, 1000, -1}, plain[3] = {900, 990, 1000}, chunks[3] = {0, 32, 192};
	long n_cases = 0, n_bad = 0, n_forced_start = 0, n_edge_end = 0, n_capped = 0, n_planted = 0, n_counted = 0, worst_excess = -1000, max_ops = 0;
	for (int it = 0; it < 1720; ++it) {
		const int w = bands[it % 5], pp = plain[(it / 5) % 3];
		int qlen = 1 + g() % 400, tlen = 1 + g() % 400;
		if (it % 4 == 1) tlen = qlen; // the walk can end in the corner
		if (it % 4 == 2) { tlen = qlen + (int)(g() % 21) - 10; if (tlen < 1) tlen = 1; }
		Matrix M;
		make_matrix(g, M, qlen, tlen, w, pp);
		const bool planted = (it / 15) % 2 == 1;
		if (planted) plant(g, M, it % 131, it % 3 == 0), ++n_planted;
		finish_matrix(g, M);
		{
			const int r = qlen + tlen - 2;
			if (tlen - 1 < M.off[r] || tlen - 1 > M.off_end[r]) ++n_forced_start;
		}
		int m_cigar = 0, n_cigar = 0;
		uint32_t *cigar = 0;
		gdo_backtrack(0, 0, M.ref.data(), M.off.data(), M.off_end.data(), M.ncol * 16, tlen - 1, qlen - 1, &m_cigar, &n_cigar, &cigar);
		if (n_cigar > max_ops) max_ops = n_cigar;
		if (n_cigar > 0 && (cigar[0] & 0xf) != 0) ++n_edge_end; // the first op is the run along the matrix's edge: i or j reached -1 first
		const int caps[4] = {0, 1, 3, qlen + tlen + 1};
		for (int ck : chunks)
			for (int cap : caps) {
				const Emu e = emulate(M, ck, cap);
				++n_cases;
				bool ok = e.nc == n_cigar;
				if (e.nc <= cap) ok = ok && (n_cigar == 0 || !memcmp(e.ops.data(), cigar, 4 * (size_t)n_cigar));
				else ++n_capped;
				if (!ok) {
					++n_bad;
					if (n_bad <= 10) fprintf(stderr, "MISMATCH it=%d qlen=%d tlen=%d w=%d plain=%d planted=%d chunk=%d cap=%d n_cigar emu=%d oracle=%d\n", it, qlen, tlen, w, pp, (int)planted, ck, cap, e.nc, n_cigar);
				}
				// direction 0 everywhere and every cell stored: L = min(qlen, tlen) cells on one diagonal, one iteration per window of 64
				if (pp == 1000 && !planted && w == -1 && ck == 0) {
					const int L = qlen < tlen ? qlen : tlen;
					const long excess = e.steps - ((L + 63) / 64 + 2);
					++n_counted;
					if (excess > worst_excess) worst_excess = excess;
				}
			}
		free(cigar);
	}
	printf("walk_emul cases=%ld mismatches=%ld planted=%ld forced_start=%ld edge_end=%ld capped=%ld max_ops=%ld counted=%ld worst_step_excess=%ld\n",
	       n_cases, n_bad, n_planted, n_forced_start, n_edge_end, n_capped, max_ops, n_counted, worst_excess);
	return n_bad || worst_excess > 0 ? 1 : 0;
}
