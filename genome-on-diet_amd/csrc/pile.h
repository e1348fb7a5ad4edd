// Pileup and variant sites from BAM alignment records (include/gdiet_hip.h, "Pileup"): the statements of the accumulator, written once for
// the kernels (pile.hip.h), for the host emulator that runs them as loops over 64 lanes (tests/emul/pile_emul.cpp) and for the driver.
// No HIP in here.  The record statements -- the head, the real CIGAR, PASS 1's verdict, the filter chain -- are coverage's (cov.h).
//
// ONE WAVEFRONT PER RECORD, two passes as in cov.h:
//   PASS 1         coverage's validation (gdc_head_words, gdc_op, gdc_decide); gdp_summary_bits adds the category no_seq in front of
//                  `counted`.  A bad record ends here: it has touched nothing.
//   PASS 2         per round of 64 operations the two exclusive scans give every lane the cursors of its operation (gdp_op says what the
//                  operation piles up: the bases of an M = X run, the positions of a D run, the one anchor of an I).  THE RUNS OF THE
//                  ROUND ARE THEN TAKEN ONE AFTER ANOTHER, WAVE-UNIFORMLY, as gdc_qual_share takes them: kind, start, length and query
//                  start of the run's lane go to every lane, the region of the run's start is found by a wave-uniform binary search
//                  (gdp_region_lower), and gdp_run_share deals the run's positions over the 64 lanes, position lo + lane, + 64, ...,
//                  region piece after region piece.  Each lane reads its own SEQ nibble and QUAL byte and issues its own adds.
// THE COUNTERS are uint32, eight per position (A C G T N DEL INS REV: 32 bytes, one 32-byte row per position), the regions back to back
// at GdpRegion::off (64-bit).
// BOUNDS.  Every load is checked against the record's own end (H.n) and l_seq, every add goes to a slot of the region piece the position
// lies in (off + p - beg with beg <= p < end): a record that contradicts itself can lose counts, never touch a row outside the regions.
// No lane reads what another wrote: the adds are integer atomics, so their order cannot matter.
#pragma once
#include "cov.h"

enum { GDP_A = 0, GDP_C, GDP_G, GDP_T, GDP_N, GDP_DEL, GDP_INS, GDP_REV, GDP_N_CNT };
// the summary: coverage's ten counters, then these two (gdiet_pile_summary_t)
enum { GDP_S_NO_SEQ = GDC_N_SUMMARY, GDP_S_SKIPPED_BASEQ, GDP_N_SUMMARY };
enum { GDP_K_NONE = 0, GDP_K_BASES, GDP_K_DEL, GDP_K_INS }; // what an operation piles up
enum { GDP_ALT_DEL = 4, GDP_ALT_INS = 5 };                  // a site's alt: 0..3 A C G T, then these

struct GdpRegion {
	uint64_t off; // the number of the region's first position among all positions
	uint32_t rid, beg, end, pad;
};

// bit i: the record adds 1 to counter i of the summary (skipped_baseq is not a bit: it counts bases); *counted: it goes through PASS 2
GDB_HD uint32_t gdp_summary_bits(const GdcHead &H, uint32_t reason, uint32_t excl_flags, uint32_t min_mapq, uint32_t *counted)
{
	uint32_t bits = gdc_summary_bits(H, reason, excl_flags, min_mapq, counted);
	if (*counted && H.l_seq == 0) bits = (bits & ~(1u << GDC_S_COUNTED)) | 1u << GDP_S_NO_SEQ, *counted = 0;
	return bits;
}

// operation k of the real CIGAR as gdc_op reads it, and what it piles up: GDP_K_BASES for M = X, GDP_K_DEL for D, GDP_K_INS for I
GDB_HD uint32_t gdp_op(const uint8_t *rec, const GdcHead &H, uint32_t k, uint32_t *len, uint32_t *rl, uint32_t *ql)
{
	uint32_t bad = 0;
	if (gdc_op(rec, H, k, len, rl, ql, &bad)) return GDP_K_BASES;
	const uint64_t p = H.ops_at + 4ull * k;
	if (bad || k >= H.n_ops || p + 4 > H.n) return GDP_K_NONE;
	const uint32_t op = gdc_ld32(rec + p) & 15u;
	return op == 2u ? GDP_K_DEL : op == 1u ? GDP_K_INS : GDP_K_NONE;
}
// The run a lane's operation gives the round: 1 with its start and length if there is one.  r: the reference cursor in front of the
// operation.  An M = X or D run of length 0 is none; an I is the one position r - 1, if an operation before it has consumed reference.
GDB_HD uint32_t gdp_run_of(uint32_t kind, uint32_t r, uint32_t pos, uint32_t L, uint32_t *start, uint32_t *len)
{
	*start = r, *len = L;
	if (kind == GDP_K_INS) {
		*start = r - 1, *len = 1;
		return r > pos;
	}
	return kind != GDP_K_NONE && L != 0;
}

// the first region (rid', beg', end') with rid' > rid, or rid' == rid and end' > p: the region p lies in, if any does, else the next one
template <class W> GDB_HD uint32_t gdp_region_lower(W &w, const GdpRegion *regs, uint32_t n_reg, uint32_t rid, uint32_t p)
{
	uint32_t lo = 0, hi = n_reg;
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		const uint32_t mr = w.uni(regs[mid].rid), me = w.uni(regs[mid].end);
		if (mr < rid || (mr == rid && me <= p)) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}

// the counter a SEQ nibble selects
GDB_HD uint32_t gdp_nibble_counter(uint32_t nib) { return nib == 1u ? GDP_A : nib == 2u ? GDP_C : nib == 4u ? GDP_G : nib == 8u ? GDP_T : GDP_N; }

// Lane `lane` of 64: its share of the run [s, s + len) of contig rid, of kind `kind`, whose first query base is q (GDP_K_BASES), from
// region i0 = gdp_region_lower(rid, s) on.  Everything but `lane` is wave-uniform; W::uni makes a loaded value a scalar, W::add is the
// add (an atomic on the device).  Returns the bases this lane skipped for their quality.
template <class W> GDB_HD uint32_t gdp_run_share(W &w, uint32_t *cnt, const GdpRegion *regs, uint32_t n_reg, uint32_t i0, const uint8_t *rec, const GdcHead &H, uint32_t kind,
                                                 uint32_t s, uint32_t len, uint32_t q, uint32_t min_baseq, uint32_t lane)
{
	uint32_t skipped = 0;
	const uint64_t e = (uint64_t)s + len;
	const uint32_t rid = (uint32_t)H.refID, rev = H.flag >> 4 & 1u;
	const uint64_t seq_at = H.qual_at - (H.l_seq + 1u) / 2u;
	for (uint32_t i = i0; i < n_reg; ++i) {
		const uint32_t rr = w.uni(regs[i].rid), rb = w.uni(regs[i].beg), re = w.uni(regs[i].end);
		if (rr != rid || rb >= e) break;
		const uint64_t off = w.uni64(regs[i].off);
		const uint32_t lo = rb > s ? rb : s, hi = re < e ? re : (uint32_t)e; // (rb < e <= 2^32 and re > s: lo < hi)
		uint32_t *row0 = cnt + (off + (lo - rb)) * GDP_N_CNT;                  // the row of position lo: wave-uniform, 64-bit
#pragma unroll 1
		for (uint32_t b = lane; b < hi - lo; b += 64) { // position lo + b < hi <= re: row b of the piece lies inside the region's slots
			uint32_t *row = row0 + (size_t)b * GDP_N_CNT;
			if (kind != GDP_K_BASES) {
				w.add(row + (kind == GDP_K_DEL ? GDP_DEL : GDP_INS));
				continue;
			}
			const uint32_t qi = q + (lo - s) + b;
			if (qi >= H.l_seq || H.qual_at + qi >= H.n) continue; // (PASS 1 has seen the query end inside l_seq, the head l_seq inside the record)
			if (H.has_qual && rec[H.qual_at + qi] < min_baseq) { ++skipped; continue; }
			const uint32_t nib = rec[seq_at + (qi >> 1)] >> ((~qi & 1u) << 2) & 15u;
			w.add(row + gdp_nibble_counter(nib));
			if (rev) w.add(row + GDP_REV);
		}
	}
	return skipped;
}

// ---- the calls, after finish ------------------------------------------------------------------------------------------------------------
struct GdpCallOpt { uint32_t min_depth, min_alt, num, den; };

// position t of all: its region (the last one with off <= t); n_reg >= 1
GDB_HD uint32_t gdp_region_of(const GdpRegion *regs, uint32_t n_reg, uint64_t t)
{
	uint32_t lo = 0, hi = n_reg;
	while (hi - lo > 1) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (regs[mid].off <= t) lo = mid;
		else hi = mid;
	}
	return lo;
}
// base u of the packed reference S (eight 4-bit codes a word): 0..3, 4 for N
GDB_HD uint32_t gdp_ref_base(const uint32_t *S, uint64_t u)
{
	const uint32_t c = S[u >> 3] >> ((uint32_t)(u & 7u) << 2) & 15u;
	return c > 4u ? 4u : c;
}
GDB_HD bool gdp_qualifies(uint32_t c, uint64_t depth, const GdpCallOpt &o) { return c >= o.min_alt && (uint64_t)c * o.den >= (uint64_t)o.num * depth; }

// One position from its eight counters c and its reference base: the consensus byte, the depth, the alt allele (0..5, meaningful at a
// site only); returns 1 at a site.  The alleles are A C G T DEL in this order: counters 0, 1, 2, 3, 5.
GDB_HD uint32_t gdp_call(const uint32_t *c, uint32_t refc, const GdpCallOpt &o, uint8_t *cons, uint32_t *depth_out, uint32_t *alt_out)
{
	const uint64_t depth = (uint64_t)c[GDP_A] + c[GDP_C] + c[GDP_G] + c[GDP_T] + c[GDP_N] + c[GDP_DEL];
	uint32_t best = 0, best_c = 0, alt = GDP_ALT_INS, alt_c = 0, any = 0;
#pragma unroll
	for (uint32_t a = 0; a < 5; ++a) {
		const uint32_t v = c[a < 4 ? a : (uint32_t)GDP_DEL];
		if (v > best_c) best = a, best_c = v;
		// (refc 4 is a reference N, allele 4 is DEL: never the reference base)
		if ((a == 4u || a != refc) && gdp_qualifies(v, depth, o) && (!any || v > alt_c)) alt = a, alt_c = v, any = 1;
	}
	if (!any) any = gdp_qualifies(c[GDP_INS], depth, o);
	const bool deep = depth >= o.min_depth;
	*cons = (uint8_t)(!deep || best_c == 0 ? 'N' : best < 4 ? (0x54474341u >> (best << 3) & 0xffu) : '*');
	*depth_out = (uint32_t)depth, *alt_out = alt;
	return deep && any;
}
