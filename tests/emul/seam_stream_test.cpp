// The seam stream of the paired steady rows of the quarter-block and half-block forms (gdw_quarter_rows, gdw_narrow_rows in ksw_wave.hip.h;
// GdwSeam, gdw_seam_init / gdw_seam_next in ksw_wave_core.h).  The seam statements of the device's pair loop run over the geometry grid of
// sel_step_test.cpp, with the query at each of the 8 byte places of an aligned 8-byte window (so at all four byte alignments of a dword,
// twice), and on EVERY paired row the byte the stream hands out is compared with gdw_qbyte and with a host copy of gdw_seam_byte, with j
// taken from the band of the row before as the general rows take it (r - 16 (st0 of row r - 1 >> 4)).  Every load the stream issues goes
// through a hook: the address is 4-aligned and the dword holds at least one byte of the query.  The query sits in an allocation that ends
// with the last dword holding one of its bytes, so that under AddressSanitizer a dword further on is a report of its own.
// Added to the grid: query lengths at which the paired rows end by the query (2 qlen - w - 1), one for every residue of the last pair's
// m mod 16, so that j reaches qlen - 1, qlen and qlen + 14 inside the paired rows; the program fails if it has not seen all three.
//
//   g++ -O2 -I genome-on-diet_amd/csrc tests/emul/seam_stream_test.cpp -o seam_stream_test && ./seam_stream_test
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#define __host__
#define __device__
static void seam_hook(const uint8_t *p);
#define GDW_SEAM_LOAD_HOOK(p) seam_hook(p)
#include "ksw_wave_core.h"

static const uint8_t *g_q;
static int g_qlen;
static long g_loads, g_rows, g_refills, g_backs, g_geoms, g_hit_qm1, g_hit_q, g_hit_q14, g_past_end;
static void seam_hook(const uint8_t *p)
{
	if (((uintptr_t)p & 3) != 0) { fprintf(stderr, "load at an address that is not 4-aligned\n"); exit(2); }
	if (p + 3 < g_q || p >= g_q + g_qlen) { fprintf(stderr, "load of a dword that holds no byte of the query (offset %ld, qlen %d)\n", (long)(p - g_q), g_qlen); exit(2); }
	++g_loads;
}

// gdw_seam_byte of ksw_wave.hip.h with the host's load
static u32 seam_byte_host(const uint8_t *query, int qlen, int j)
{
	if (j < 0 || j >= qlen) return 0u;
	const uintptr_t a = (uintptr_t)(query + j);
	const uint8_t *d = (const uint8_t *)(a & ~(uintptr_t)3);
	seam_hook(d), --g_loads;
	const u32 wd = (u32)d[0] | (u32)d[1] << 8 | (u32)d[2] << 16 | (u32)d[3] << 24;
	return (wd >> (8 * (a & 3))) & 0xffu;
}

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "  (qlen %d tlen %d w %d query at byte %d)\n", qlen, tlen, w, place); exit(2); } while (0)

// the seam statements of the device's pair loop
static void run(int qlen, int tlen, int w, int place)
{
	// the query at byte `place` of an 8-aligned window; the allocation ends with the last dword that holds a byte of it
	const size_t size = ((size_t)place + qlen + 3) & ~(size_t)3;
	uint8_t *buf = (uint8_t *)malloc(size);
	if (!buf || ((uintptr_t)buf & 7)) { fprintf(stderr, "malloc: no 8-aligned block\n"); exit(2); }
	memset(buf, 0xEE, size);
	uint8_t *q = buf + place;
	for (int i = 0; i < qlen; ++i) q[i] = (uint8_t)(1 + (i * 2654435761u >> 7) % 250); // no zero: a byte wrongly zero-filled shows
	g_q = q, g_qlen = qlen;
	int rA, rS;
	gdw_steady_rows(qlen, tlen, w, rA, rS);
	int r = rA;
	if (rS > rA) {
		int m = (rA - w + 1) >> 1;
		GdwSeam S;
		gdw_seam_init(S, q, qlen, r, m - 1);
		auto row = [&](int rr, int mb) { // (the device's pst_ is mb >> 4)
			const int pst_ = mb >> 4;
			int s0, e0;
			gd_band(rr - 1, qlen, tlen, w, s0, e0);
			if ((s0 >> 4) != pst_) FAIL("row %d: pst_ %d is not the block of the row before (%d)\n", rr, pst_, s0 >> 4);
			const int j = rr - (pst_ << 4);
			if (j < 17) FAIL("row %d: j = %d\n", rr, j);
			const long before = g_loads;
			const u32 got = gdw_seam_next(S, q, qlen, rr, mb), want = gdw_qbyte(q, qlen, j);
			if (g_loads != before) ++g_refills;
			if (got != want || got != seam_byte_host(q, qlen, j)) FAIL("row %d j %d: the stream gives %02x, query byte %02x\n", rr, j, got, want);
			g_hit_qm1 += j == qlen - 1, g_hit_q += j == qlen, g_hit_q14 += j == qlen + 14, g_past_end += j >= qlen;
			if (j > qlen + 14) FAIL("row %d: j = qlen + %d\n", rr, j - qlen);
			++g_rows;
		};
		for (; r < rS; r += 2, ++m) {
			row(r, m - 1);
			if ((m & 15) == 0) gdw_seam_init(S, q, qlen, r + 1, m), ++g_backs; // (the step back by 15)
			row(r + 1, m);
		}
	}
	free(buf);
	++g_geoms;
}

static bool admitted(bool quarter, int qlen, int tlen, int w)
{
	return quarter ? w <= GD_W_QUARTER && gd_quarter_supported(qlen, tlen, w) : w <= GD_W_NARROW && gd_narrow_supported(qlen, tlen, w);
}

static int grid(bool quarter, const int *bands, int nb)
{
	for (int b = 0; b < nb; ++b) {
		const int w = bands[b];
		const long g0 = g_geoms, r0 = g_rows;
		const int mods[] = {0, 1, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15};
		for (int mod : mods)
			for (int dk = 0; dk < 7; ++dk) {
				const int dabs = dk == 0 ? 0 : dk <= 2 ? 1 : dk <= 4 ? w - 1 : w, delta = (dk & 1) ? dabs : -dabs; // tlen - qlen
				const int bases[] = {w - 40, w + 39, w + 30, w + 229, 2 * w + 200, 2 * w + 599, 5 * w + 700}; // (sel_step_test.cpp)
				for (int lk = 0; lk < 7; ++lk) {
					int base = bases[lk];
					if (delta > 0 && lk >= 4) base += delta;
					int tlen = (base & ~15) + mod;
					if (tlen <= dabs + 20) tlen += (dabs + 36) & ~15;
					const int qlen = tlen - delta;
					if (qlen < 20 || !admitted(quarter, qlen, tlen, w)) continue;
					for (int place = 0; place < 8; ++place) run(qlen, tlen, w, place);
				}
			}
		// the paired rows end by the query: the last row has j = qlen - 1 + (m & 15), m = qlen - w - 1
		for (int k = 0; k < 16; ++k) {
			const int qlen = 2 * w + 300 + k, tlen = qlen + 40;
			if (!admitted(quarter, qlen, tlen, w)) continue;
			for (int place = 0; place < 8; ++place) run(qlen, tlen, w, place);
		}
		printf("%s band %d geometries %ld paired_rows %ld\n", quarter ? "quarter" : "half", w, g_geoms - g0, g_rows - r0);
		if (g_geoms == g0) return 3;
	}
	return 0;
}

int main()
{
	const int qbands[] = {239, 238, 237, 223, 224, 225, 119, 55};
	const int hbands[] = {495, 494, 479, 480, 481, 400, 401, 247, 119};
	int rc = grid(true, qbands, (int)(sizeof(qbands) / sizeof(int)));
	if (!rc) rc = grid(false, hbands, (int)(sizeof(hbands) / sizeof(int)));
	printf("seam_stream_test geometries=%ld paired_rows=%ld loads=%ld refills=%ld steps_back=%ld j_qlen_m1=%ld j_qlen=%ld j_qlen_p14=%ld past_end=%ld\n",
	       g_geoms, g_rows, g_loads, g_refills, g_backs, g_hit_qm1, g_hit_q, g_hit_q14, g_past_end);
	if (!rc && !(g_hit_qm1 && g_hit_q && g_hit_q14)) rc = 4;
	if (!rc) printf("seam_stream_test ok\n");
	return rc;
}
