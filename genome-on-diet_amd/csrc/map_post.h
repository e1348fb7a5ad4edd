// P1 on raw arrays: mm_fix_cigar + mm_update_extra (LR/align.c:93-172,259-318), written once for the host stages (map_host.h) and
// for the device kernel map_post_kernel (map_kernels.hip.h: one thread per alignment right behind the backtrack, so that the
// host never has to fetch 15 kbp of reference and walk 15 kbp of CIGAR per candidate).
// Floating point follows the reference operation by operation -- a double accumulator, float mg_log2 -- with contraction into
// fused multiply-adds switched off (the reference's x86-64 build has none; the GPU would fuse by default and round differently).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define GDP_HD __host__ __device__ __forceinline__
#else
#define GDP_HD static inline
#endif

struct GdPostOut { // what P1 leaves in mm_reg1_t / mm_extra_t besides the CIGAR
	int32_t qshift, tshift; // leading I / D removed from the CIGAR: the caller moves qs (or qe on the reverse strand) / rs by these
	int32_t mlen, blen, dp_max;
	uint32_t n_ambi;
};

GDP_HD float gdp_mg_log2(float x) // LR/mmpriv.h:146-157
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	union { float f; uint32_t i; } z = {x};
	float log_2 = (float)(((z.i >> 23) & 255) - 128);
	z.i &= ~(255u << 23);
	z.i += 127u << 23;
	const float t1 = -0.34484843f * z.f;
	const float t2 = t1 + 2.02466578f;
	const float t3 = t2 * z.f;
	const float t4 = t3 - 0.67487759f;
	log_2 += t4;
	return log_2;
}

// mm_fix_cigar on cg[0..*n): left-aligns indels, merges I/D runs, drops zero-length ops and a leading I / D
GDP_HD void gdp_fix_cigar(uint32_t *cg, uint32_t *n_io, const uint8_t *qseq, const uint8_t *tseq, int32_t *qshift, int32_t *tshift)
{
	int32_t toff = 0, qoff = 0, to_shrink = 0;
	uint32_t k, n = *n_io;
	*qshift = *tshift = 0;
	if (n <= 1) return;
	for (k = 0; k < n; ++k) { // indel left alignment
		const uint32_t op = cg[k] & 0xf, len = cg[k] >> 4;
		if (len == 0) to_shrink = 1;
		if (op == 0) toff += len, qoff += len;
		else if (op == 1 || op == 2) {
			if (k > 0 && k < n - 1 && (cg[k - 1] & 0xf) == 0 && (cg[k + 1] & 0xf) == 0) {
				int l, prev_len = (int)(cg[k - 1] >> 4);
				if (op == 1) { for (l = 0; l < prev_len; ++l) if (qseq[qoff - 1 - l] != qseq[qoff + len - 1 - l]) break; }
				else { for (l = 0; l < prev_len; ++l) if (tseq[toff - 1 - l] != tseq[toff + len - 1 - l]) break; }
				if (l > 0) cg[k - 1] -= (uint32_t)l << 4, cg[k + 1] += (uint32_t)l << 4, qoff -= l, toff -= l;
				if (l == prev_len) to_shrink = 1;
			}
			if (op == 1) qoff += len; else toff += len;
		} else if (op == 3) toff += len;
	}
	for (k = 0; k + 2 < n; ++k) { // fix CIGAR like 5I6D7I   (k < n_cigar - 2 with unsigned n_cigar >= 2)
		if ((cg[k] & 0xf) > 0 && (cg[k] & 0xf) + (cg[k + 1] & 0xf) == 3) {
			uint32_t l, s[3] = {0, 0, 0};
			for (l = k; l < n; ++l) {
				const uint32_t op = cg[l] & 0xf;
				if (op == 1 || op == 2 || cg[l] >> 4 == 0) s[op] += cg[l] >> 4;
				else break;
			}
			if (s[1] > 0 && s[2] > 0 && l - k > 2) {
				cg[k] = s[1] << 4 | 1, cg[k + 1] = s[2] << 4 | 2;
				for (k += 2; k < l; ++k) cg[k] &= 0xf;
				to_shrink = 1;
			}
			k = l;
		}
	}
	if (to_shrink) {
		uint32_t l = 0;
		for (k = 0; k < n; ++k) if (cg[k] >> 4 != 0) cg[l++] = cg[k];
		n = l;
		for (k = l = 0; k < n; ++k)
			if (k == n - 1 || (cg[k] & 0xf) != (cg[k + 1] & 0xf)) cg[l++] = cg[k];
			else cg[k + 1] += cg[k] >> 4 << 4;
		n = l;
	}
	if ((cg[0] & 0xf) == 1 || (cg[0] & 0xf) == 2) { // get rid of leading I or D
		const int32_t l = (int32_t)(cg[0] >> 4);
		if ((cg[0] & 0xf) == 1) *qshift = l;
		else *tshift = l;
		--n;
		for (k = 0; k < n; ++k) cg[k] = cg[k + 1];
	}
	*n_io = n;
}

// mm_update_extra: fix the CIGAR, then mlen / blen / n_ambi / dp_max.  mat: the 5 x 5 matrix of the caller (match a, mismatch -b,
// 0 against N); an index past it (query byte 7 = N of a reverse-complemented read against a target N) is undefined in the reference
// and taken as 0.  n_ambi_in: the record's count before the call (the reference adds to it).
GDP_HD void gdp_update_extra(uint32_t *cg, uint32_t *n_io, const uint8_t *qseq, const uint8_t *tseq, const int8_t *mat, int8_t q, int8_t e, int log_gap,
                             GdPostOut *out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	int32_t qshift, tshift, toff = 0, qoff = 0;
	double s = 0.0, mx = 0.0;
	gdp_fix_cigar(cg, n_io, qseq, tseq, &qshift, &tshift);
	qseq += qshift, tseq += tshift;
	int32_t blen = 0, mlen = 0;
	uint32_t n_ambi_tot = 0;
	const uint32_t n = *n_io;
	if (!log_gap) {
		// The short-read form (no logarithmic gap cost): every term of the running score is an integer, so the reference's double accumulator
		// holds integers and int32 arithmetic gives the same values.  Eight bases per load; a group without an ambiguous base (codes 0..3
		// on both sides: no bit 2 anywhere) scores mat[0] / mat[1] by equality, any other group goes through the table base by base.
		int32_t si = 0, mxi = 0;
		const int32_t mch = mat[0], mis = mat[1];
		bool uniform = true; // (one match and one mismatch score among the four bases: what mm_set_opt builds; else everything through the table)
		for (int i = 0; i < 4; ++i)
			for (int j = 0; j < 4; ++j) uniform &= mat[i * 5 + j] == (i == j ? mch : mis);
		for (uint32_t k = 0; k < n; ++k) {
			const uint32_t op = cg[k] & 0xf, len = cg[k] >> 4;
			if (op == 0) {
				int n_ambi = 0, n_diff = 0;
				uint32_t l = 0;
				for (; l + 8 <= len; l += 8) {
					uint64_t a, b;
					__builtin_memcpy(&a, qseq + qoff + l, 8), __builtin_memcpy(&b, tseq + toff + l, 8);
					if (uniform && !((a | b) & 0x0404040404040404ull)) {
						const uint64_t x = a ^ b;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
						for (int j = 0; j < 8; ++j) {
							const int d = ((x >> (8 * j)) & 0xff) != 0;
							n_diff += d;
							si += d ? mis : mch;
							if (si < 0) si = 0;
							else mxi = mxi > si ? mxi : si;
						}
					} else
						for (int j = 0; j < 8; ++j) {
							const int cq = (int)((a >> (8 * j)) & 0xff), ct = (int)((b >> (8 * j)) & 0xff);
							if (ct > 3 || cq > 3) ++n_ambi;
							else if (ct != cq) ++n_diff;
							si += (ct * 5 + cq < 25) ? (int32_t)mat[ct * 5 + cq] : 0;
							if (si < 0) si = 0;
							else mxi = mxi > si ? mxi : si;
						}
				}
				for (; l < len; ++l) {
					const int cq = qseq[qoff + l], ct = tseq[toff + l];
					if (ct > 3 || cq > 3) ++n_ambi;
					else if (ct != cq) ++n_diff;
					si += (ct * 5 + cq < 25) ? (int32_t)mat[ct * 5 + cq] : 0;
					if (si < 0) si = 0;
					else mxi = mxi > si ? mxi : si;
				}
				blen += (int32_t)len - n_ambi, mlen += (int32_t)len - (n_ambi + n_diff), n_ambi_tot += (uint32_t)n_ambi;
				toff += len, qoff += len;
			} else if (op == 1 || op == 2) {
				int n_ambi = 0;
				for (uint32_t l = 0; l < len; ++l)
					if ((op == 1 ? qseq[qoff + l] : tseq[toff + l]) > 3) ++n_ambi;
				blen += (int32_t)len - n_ambi, n_ambi_tot += (uint32_t)n_ambi;
				si -= (int32_t)(q + e);
				if (si < 0) si = 0;
				if (op == 1) qoff += len; else toff += len;
			} else if (op == 3) toff += len;
		}
		out->qshift = qshift, out->tshift = tshift, out->mlen = mlen, out->blen = blen, out->n_ambi = n_ambi_tot;
		out->dp_max = mxi; // ((int32_t)(mx + .499) of an integer-valued mx)
		return;
	}
	for (uint32_t k = 0; k < n; ++k) {
		const uint32_t op = cg[k] & 0xf, len = cg[k] >> 4;
		if (op == 0) {
			int n_ambi = 0, n_diff = 0;
			for (uint32_t l = 0; l < len; ++l) {
				const int cq = qseq[qoff + l], ct = tseq[toff + l];
				if (ct > 3 || cq > 3) ++n_ambi;
				else if (ct != cq) ++n_diff;
				s += (ct * 5 + cq < 25) ? (double)mat[ct * 5 + cq] : 0.0;
				if (s < 0) s = 0;
				else mx = mx > s ? mx : s;
			}
			blen += (int32_t)len - n_ambi, mlen += (int32_t)len - (n_ambi + n_diff), n_ambi_tot += (uint32_t)n_ambi;
			toff += len, qoff += len;
		} else if (op == 1 || op == 2) {
			int n_ambi = 0;
			for (uint32_t l = 0; l < len; ++l)
				if ((op == 1 ? qseq[qoff + l] : tseq[toff + l]) > 3) ++n_ambi;
			blen += (int32_t)len - n_ambi, n_ambi_tot += (uint32_t)n_ambi;
			if (log_gap) {
				const double pen = (double)e * (double)gdp_mg_log2(1.0f + (float)len);
				const double tot = (double)q + pen;
				s -= tot;
			} else s -= (double)(q + e);
			if (s < 0) s = 0;
			if (op == 1) qoff += len; else toff += len;
		} else if (op == 3) toff += len;
	}
	out->qshift = qshift, out->tshift = tshift, out->mlen = mlen, out->blen = blen, out->n_ambi = n_ambi_tot;
	out->dp_max = (int32_t)(mx + .499);
}

// ---- the arithmetic of the wave-parallel form (map_post_wave_kernel, map_kernels.hip.h, which explains it) ------------------------------
// Written here so that a host program can run it lane by lane (tests/emul/post_emul.cpp); the kernel calls exactly these.
// GDP_MISTAKE = n swaps one expression below for a wrong one: the seeded mistakes of tests/test_post.py, compiled by the emulator's
// build alone.
#if defined(GDP_MISTAKE) && !defined(GDP_POST_EMUL)
#error "GDP_MISTAKE belongs to the build of tests/emul/post_emul.cpp alone"
#endif
#ifndef GDP_MISTAKE
#define GDP_MISTAKE 0
#endif
#define GDP_MIS(n, right, wrong) (GDP_MISTAKE == (n) ? (wrong) : (right))

#define GDP_FRAC 30
struct GdpSeg { int32_t A, B, P, Q; }; // in units of 1 (base scores are integers); B / Q = GDP_NONE: no clamp inside the segment
#define GDP_NONE (-0x20000000)
GDP_HD GdpSeg gdp_seg_join(const GdpSeg &x, const GdpSeg &y)
{
	GdpSeg r;
	r.A = x.A + y.A;
	const int32_t bx = x.B == GDP_NONE ? GDP_NONE : GDP_MIS(1, x.B + y.A, x.B);
	r.B = bx > y.B ? bx : y.B;
	const int32_t p2 = y.P == GDP_NONE ? GDP_NONE : GDP_MIS(2, x.A + y.P, y.P);
	r.P = x.P > p2 ? x.P : p2;
	const int32_t q2 = (x.B == GDP_NONE || y.P == GDP_NONE) ? GDP_NONE : GDP_MIS(3, x.B + y.P, GDP_NONE);
	int32_t q = x.Q > y.Q ? x.Q : y.Q;
	r.Q = q > q2 ? q : q2;
	return r;
}

// one base of score a:  s -> max(s + a, 0); the state after it is max(s + a, 0) as well
GDP_HD GdpSeg gdp_seg_base(int32_t a)
{
	GdpSeg g;
	g.A = a, g.B = 0, g.P = a, g.Q = 0;
	return g;
}

// A chunk's segment (A, Bc, Pm, Qm) folded into the running score S and its maximum MX, each as (integer part, fraction in units of
// 2^-GDP_FRAC, 0 <= fraction < 2^GDP_FRAC): base scores are integers, only gap penalties carry a fraction.
GDP_HD void gdp_run_fold(int32_t A, int32_t Bc, int32_t Pm, int32_t Qm, int32_t &Si, int32_t &Sf, int32_t &MXi, int32_t &MXf)
{
	if (Pm != GDP_NONE && (Si + Pm > MXi || GDP_MIS(4, (Si + Pm == MXi && Sf > MXf), false))) MXi = Si + Pm, MXf = Sf; // MX = max(MX, S + P)
	if (Qm != GDP_NONE && GDP_MIS(5, (Qm > MXi), (Qm >= MXi))) MXi = Qm, MXf = 0;                                      // MX = max(MX, Q)
	Si += A;
	if (Bc != GDP_NONE && Si < Bc) Si = Bc, Sf = GDP_MIS(6, 0, Sf); // S = max(S + A, B): with 0 <= fraction < 1, S + A < B iff its integer part is
}

// A gap's cost q + e * mg_log2(1 + len) (or q + e): >= 0, a multiple of 2^-GDP_FRAC below 2^12 -- integer part and fraction, both exact
GDP_HD double gdp_gap_cost(int8_t q, int8_t e, int log_gap, uint32_t len)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	double tot;
	if (log_gap) {
		const double pen = (double)e * (double)gdp_mg_log2(1.0f + (float)len);
		tot = (double)q + pen;
	} else tot = (double)(q + e);
	return tot;
}
GDP_HD int32_t gdp_gap_int(double tot) { return (int32_t)tot; }
GDP_HD int32_t gdp_gap_frac(double tot, int32_t Ti)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	return (int32_t)((tot - (double)Ti) * (double)(1 << GDP_FRAC));
}
GDP_HD void gdp_run_gap(int32_t Ti, int32_t Tf, int32_t &Si, int32_t &Sf)
{
	Sf -= Tf, Si -= Ti;
	if (Sf < 0) Sf += 1 << GDP_FRAC, Si -= GDP_MIS(7, 1, 0);
	if (Si < 0) Si = 0, Sf = 0; // (s < 0 iff its integer part is)
}

GDP_HD int32_t gdp_run_round(int32_t MXi, int32_t MXf)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	return (int32_t)((double)MXi + (double)MXf / (double)(1 << GDP_FRAC) + GDP_MIS(8, .499, .5));
}

// ---- mm_update_cigar_eqx (SR/align.c:174-257; --eqx of the ShortReads variant): every M becomes its runs of = (7) and X (8) -------------
// Called where the reference calls it (SR/align.c:315-317): behind mm_update_extra, on the CIGAR as gdp_fix_cigar leaves it (no
// zero-length operation) and on the sequences moved by the shifts that function returned.  "Equal" is equality of the two bytes, as in the
// reference: an N of a forward read (4) against a target N (4) is =, an N of a reverse-complemented read (7: SR/map.c:748,755, and what the
// device windows hold) against a target N is X.
// bit j of the result: byte j of a and b differ
GDP_HD uint32_t gdp_diff8(uint64_t a, uint64_t b)
{
	const uint64_t x = a ^ b;
	const uint64_t h = (((x & 0x7f7f7f7f7f7f7f7full) + 0x7f7f7f7f7f7f7f7full) | x) & 0x8080808080808080ull;
	return (uint32_t)(((h >> 7) * 0x0102040810204080ull) >> 56);
}

// The reference's first pass (:180-210): the number of = / X runs of all M operations (*n_eqx) and of M operations (*n_m); returns the
// length of the rewritten CIGAR.  Eight bases per load: a group adds the number of places where its difference mask changes.
GDP_HD uint32_t gdp_cigar_eqx_count(const uint32_t *cg, uint32_t n, const uint8_t *qseq, const uint8_t *tseq, uint32_t *n_eqx, uint32_t *n_m)
{
	uint32_t toff = 0, qoff = 0, runs = 0, n_M = 0;
	for (uint32_t k = 0; k < n; ++k) {
		const uint32_t op = cg[k] & 0xf, len = cg[k] >> 4;
		if (op == 0) {
			uint32_t prev = 0, l = 0;
			bool first = true;
			for (; l + 8 <= len; l += 8) {
				uint64_t a, b;
				__builtin_memcpy(&a, qseq + qoff + l, 8), __builtin_memcpy(&b, tseq + toff + l, 8);
				const uint32_t m = gdp_diff8(a, b);
				runs += (uint32_t)__builtin_popcount((m ^ (m << 1 | (first ? ~m & 1 : prev))) & 0xff);
				prev = m >> 7, first = false;
			}
			for (; l < len; ++l) {
				const uint32_t d = qseq[qoff + l] != tseq[toff + l];
				runs += first || d != prev;
				prev = d, first = false;
			}
			++n_M;
			toff += len, qoff += len;
		} else if (op == 1) qoff += len;
		else if (op == 2 || op == 3) toff += len;
	}
	*n_eqx = runs, *n_m = n_M;
	return runs == n_M ? n : n + runs - n_M; // (:212 and :220; runs >= n_M where no M is empty)
}

// The reference's second half on the slot itself (it copies into a new allocation: :219-256).  Count rule (:212-218): as many runs as M
// operations -- every M is relabelled =, whatever its bases are.  Otherwise the CIGAR grows to n_new = gdp_cigar_eqx_count(...) operations in
// place, written from the last operation backwards: operation k's runs end where operation k + 1's begin, and as every operation in
// front of k yields at least one, nothing is written over an operation not yet read.  cg must have room for n_new words.
GDP_HD void gdp_cigar_eqx_write(uint32_t *cg, uint32_t n, uint32_t n_new, uint32_t n_eqx, uint32_t n_m, const uint8_t *qseq, const uint8_t *tseq)
{
	if (n_eqx == n_m) {
		for (uint32_t k = 0; k < n; ++k)
			if ((cg[k] & 0xf) == 0) cg[k] = cg[k] >> 4 << 4 | 7;
		return;
	}
	uint32_t toff = 0, qoff = 0;
	for (uint32_t k = 0; k < n; ++k) { // the ends of the two sequences
		const uint32_t op = cg[k] & 0xf, len = cg[k] >> 4;
		if (op == 0) toff += len, qoff += len;
		else if (op == 1) qoff += len;
		else if (op == 2 || op == 3) toff += len;
	}
	uint32_t m = n_new;
	for (uint32_t k = n; k-- > 0;) { // (n_new - n + n_M runs and n - n_M other operations: exactly n_new stores)
		const uint32_t c = cg[k], op = c & 0xf, len = c >> 4;
		if (op != 0) {
			if (op == 1) qoff -= len;
			else if (op == 2 || op == 3) toff -= len;
			cg[--m] = c;
			continue;
		}
		toff -= len, qoff -= len;
		uint32_t cur = 0, cnt = 0, l = len; // the run being collected, from the M's last base towards its first
		while (l >= 8) {
			l -= 8;
			uint64_t a, b;
			__builtin_memcpy(&a, qseq + qoff + l, 8), __builtin_memcpy(&b, tseq + toff + l, 8);
			const uint32_t d8 = gdp_diff8(a, b);
			if (cnt && d8 == (cur ? 0xffu : 0u)) { cnt += 8; continue; }
			for (int j = 7; j >= 0; --j) {
				const uint32_t d = d8 >> j & 1;
				if (cnt && d != cur) { cg[--m] = cnt << 4 | (cur ? 8 : 7); cnt = 0; }
				cur = d, ++cnt;
			}
		}
		while (l > 0) {
			--l;
			const uint32_t d = qseq[qoff + l] != tseq[toff + l];
			if (cnt && d != cur) { cg[--m] = cnt << 4 | (cur ? 8 : 7); cnt = 0; }
			cur = d, ++cnt;
		}
		if (cnt) cg[--m] = cnt << 4 | (cur ? 8 : 7);
	}
}

GDP_HD void gdp_cigar_eqx(uint32_t *cg, uint32_t *n_io, const uint8_t *qseq, const uint8_t *tseq)
{
	uint32_t n_eqx, n_m;
	const uint32_t n = *n_io, n_new = gdp_cigar_eqx_count(cg, n, qseq, tseq, &n_eqx, &n_m);
	gdp_cigar_eqx_write(cg, n, n_new, n_eqx, n_m, qseq, tseq);
	*n_io = n_new;
}
