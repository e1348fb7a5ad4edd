// Stand-alone host run of the two P1 kernels (map_kernels.hip.h) per alignment, meant to be built with -fsanitize=address,undefined:
//   (a) what map_post_kernel<false> does: gdp_update_extra (map_post.h), the thread form's code;
//   (b) a lock-step restatement of map_post_wave_kernel over 64 lanes, built from the gdp_ helpers the kernel calls: lane 0 runs
//       gdp_fix_cigar, every 64-base chunk of an M becomes one gdp_seg_base per lane, the lanes are joined by the kernel's tree
//       (d = 1, 2, .. 32, lane i takes lane i + d's segment where i + d < 64, its own otherwise -- what __shfl_down returns), lane 0's
//       segment is folded into the running state.  Between two exchanges the lanes run one after the other, in the order 0..63 and
//       again in the order 63..0: a lane that read what another had not yet written would give two different answers.
// Every CIGAR sits in a heap block of exactly its slot's size and the two windows in blocks of exactly their lengths, so nothing can step
// outside without the sanitizer seeing it.
//   post_emul <in> <out>
//   in : int32 n_rec; per record eight int32 {n_cigar, slot words, qlen, tlen, score, q, e, log_gap}, int8 mat[25] and three bytes of
//        padding, the slot's words (the raw CIGAR first), qlen query codes, tlen target codes
//   out: per record and for (a), (b) forwards, (b) backwards: int32 n_cigar, the six int32 of GdPostOut (qshift, tshift, mlen, blen,
//        dp_max, n_ambi), the slot's words (slot words of them: also those behind the new n_cigar)
// A slot is dead by the kernels' rule (score -0x40000000, n_cigar <= 0 or above the slot): all zero, slot and n_cigar untouched.
// -DGDP_MISTAKE=n (1..8) builds one seeded mistake into the helpers (map_post.h): tests/test_post.py asks which inputs notice.
#define GDP_POST_EMUL 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "map_post.h"

#define NEG_INF_SCORE (-0x40000000)

static void zero(GdPostOut &P) { P.qshift = P.tshift = P.mlen = P.blen = P.dp_max = 0, P.n_ambi = 0; }

static void thread_form(uint32_t *cg, int64_t cap, int32_t *n_cigar, int32_t score, const uint8_t *q, const uint8_t *t, const int8_t *mat, int8_t gq, int8_t ge,
                        int log_gap, GdPostOut &P)
{
	zero(P);
	const int32_t n0 = *n_cigar;
	if (score != NEG_INF_SCORE && n0 > 0 && (int64_t)n0 <= cap) {
		uint32_t n = (uint32_t)n0;
		gdp_update_extra(cg, &n, q, t, mat, gq, ge, log_gap, &P);
		*n_cigar = (int32_t)n;
	}
}

struct Lanes { // the order in which the 64 lanes take their turn between two exchanges
	bool rev;
	int at(int i) const { return rev ? 63 - i : i; }
};

static void wave_form(uint32_t *cg, int64_t cap, int32_t *n_cigar, int32_t score, const uint8_t *qseq, const uint8_t *tseq, const int8_t *mat, int8_t gq, int8_t ge,
                      int log_gap, GdPostOut &P, Lanes L)
{
	int8_t s_mat[32];
	for (int i = 0; i < 64; ++i) {
		const int lane = L.at(i);
		if (lane < 25) s_mat[lane] = mat[lane];
		if (lane >= 25 && lane < 32) s_mat[lane] = 0;
	}
	zero(P);
	const int32_t n0 = *n_cigar;
	if (!(score != NEG_INF_SCORE && n0 > 0 && (int64_t)n0 <= cap)) return;
	uint32_t n_fix = (uint32_t)n0;
	int32_t qshift = 0, tshift = 0;
	gdp_fix_cigar(cg, &n_fix, qseq, tseq, &qshift, &tshift); // lane 0
	*n_cigar = (int32_t)n_fix;
	const uint32_t n = n_fix;
	P.qshift = qshift, P.tshift = tshift;
	qseq += P.qshift, tseq += P.tshift;
	int32_t Si = 0, Sf = 0, MXi = 0, MXf = 0;
	int32_t qoff = 0, toff = 0, blen = 0, mlen = 0;
	uint32_t n_ambi_tot = 0;
	for (uint32_t k = 0; k < n; ++k) {
		const uint32_t c = cg[k], op = c & 0xf, len = c >> 4;
		if (op == 0) {
			for (uint32_t base = 0; base < len; base += 64) {
				GdpSeg g[64], o[64];
				int cnt2[64], oc[64];
				for (int i = 0; i < 64; ++i) {
					const int lane = L.at(i);
					const GdpSeg none = {0, GDP_NONE, GDP_NONE, GDP_NONE};
					g[lane] = none, cnt2[lane] = 0;
					const uint32_t l = base + (uint32_t)lane;
					if (l < len) {
						const int cq = qseq[qoff + l], ct = tseq[toff + l];
						if (ct > 3 || cq > 3) cnt2[lane] = 1;
						else if (ct != cq) cnt2[lane] = 1 << 16;
						const int idx = ct * 5 + cq;
						const int32_t a = idx < 25 ? (int32_t)s_mat[idx] : 0;
						g[lane] = gdp_seg_base(a);
					}
				}
				for (int d = 1; d < 64; d <<= 1) {
					for (int lane = 0; lane < 64; ++lane) { // the exchange: every lane's registers as they stand
						const int src = lane + d < 64 ? lane + d : lane;
						o[lane] = g[src], oc[lane] = cnt2[src];
					}
					for (int i = 0; i < 64; ++i) {
						const int lane = L.at(i);
						if (lane + d < 64) g[lane] = gdp_seg_join(g[lane], o[lane]), cnt2[lane] += oc[lane];
					}
				}
				const int32_t A = g[0].A, Bc = g[0].B, Pm = g[0].P, Qm = g[0].Q;
				const int c2 = cnt2[0], na = c2 & 0xffff, nd = c2 >> 16;
				gdp_run_fold(A, Bc, Pm, Qm, Si, Sf, MXi, MXf);
				const uint32_t cnt = len - base < 64 ? len - base : 64;
				blen += (int32_t)cnt - na, mlen += (int32_t)cnt - (na + nd), n_ambi_tot += (uint32_t)na;
			}
			toff += len, qoff += len;
		} else if (op == 1 || op == 2) {
			int na = 0;
			const uint8_t *src = op == 1 ? qseq + qoff : tseq + toff;
			for (uint32_t l0 = 0; l0 < len; l0 += 64) {
				uint64_t ballot = 0;
				for (int i = 0; i < 64; ++i) {
					const int lane = L.at(i);
					if (l0 + (uint32_t)lane < len && src[l0 + lane] > 3) ballot |= 1ull << lane;
				}
				na += __builtin_popcountll(ballot);
			}
			blen += (int32_t)len - na, n_ambi_tot += (uint32_t)na;
			const double tot = gdp_gap_cost(gq, ge, log_gap, len);
			const int32_t Ti = gdp_gap_int(tot);
			const int32_t Tf = gdp_gap_frac(tot, Ti);
			gdp_run_gap(Ti, Tf, Si, Sf);
			if (op == 1) qoff += len; else toff += len;
		} else if (op == 3) toff += len;
	}
	P.mlen = mlen, P.blen = blen, P.n_ambi = n_ambi_tot;
	P.dp_max = gdp_run_round(MXi, MXf);
}

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: post_emul <in> <out>\n"); return 2; }
	FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
	if (!f || !g) { perror(f ? argv[2] : argv[1]); return 2; }
	int32_t n_rec = 0;
	if (fread(&n_rec, 4, 1, f) != 1) return 3;
	for (int32_t r = 0; r < n_rec; ++r) {
		int32_t h[8];
		int8_t mat[28];
		if (fread(h, 4, 8, f) != 8 || fread(mat, 1, 28, f) != 28) return 3;
		const int32_t n0 = h[0], cap = h[1], ql = h[2], tl = h[3], score = h[4];
		if (cap < 0 || ql < 0 || tl < 0) return 3;
		std::vector<uint32_t> raw((size_t)cap);
		if (cap && fread(raw.data(), 4, (size_t)cap, f) != (size_t)cap) return 3;
		uint8_t *q = (uint8_t *)malloc((size_t)ql), *t = (uint8_t *)malloc((size_t)tl); // (exact sizes; a zero-sized block may still not be read)
		if ((ql && fread(q, 1, (size_t)ql, f) != (size_t)ql) || (tl && fread(t, 1, (size_t)tl, f) != (size_t)tl)) return 3;
		for (int v = 0; v < 3; ++v) {
			uint32_t *cg = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)cap);
			if (cap) memcpy(cg, raw.data(), sizeof(uint32_t) * (size_t)cap);
			int32_t nc = n0;
			GdPostOut P;
			if (v == 0) thread_form(cg, cap, &nc, score, q, t, mat, (int8_t)h[5], (int8_t)h[6], h[7], P);
			else wave_form(cg, cap, &nc, score, q, t, mat, (int8_t)h[5], (int8_t)h[6], h[7], P, Lanes{v == 2});
			const int32_t out[7] = {nc, P.qshift, P.tshift, P.mlen, P.blen, P.dp_max, (int32_t)P.n_ambi};
			fwrite(out, 4, 7, g);
			if (cap) fwrite(cg, 4, (size_t)cap, g);
			free(cg);
		}
		free(q), free(t);
	}
	fclose(f);
	return fclose(g) ? 3 : 0;
}
