// Duplicate marking of BAM alignment records (include/gdiet_hip.h, "Duplicate marking"): the statements of the key pass, of the decision
// and of the flag rewrite, written once for the kernels (bam_markdup.hip.h), for the host emulator that runs them as loops over 64 lanes
// (tests/emul/markdup_emul.cpp) and for the driver.  No HIP in here.  Like the accumulators (cov.h, whose loads, head and CG walk it uses)
// it reads nothing but the records' own bytes.
//
// ONE WAVEFRONT PER RECORD in the key pass.  The real CIGAR (the record's words, or the CG:B:I array of a placeholder) is taken in rounds
// of 64 words, lane l the word b0 + l:
//   gdm_round_lane  a lane's word of a round: its reference length is added to the lane's sum, a code above 8 is remembered, and the lane
//                   says whether its word is an operation other than S and H.  The round's answers are one 64-bit mask (a ballot on the
//                   device, a loop on the host), from which gdm_round_mask keeps, wave-uniformly, the index of the FIRST such word of the
//                   record and the index behind the LAST: two scalars, no cross-lane reduction, and no lane-stride wrap to get wrong.
//   gdm_clip_lane   a lane's share of the clip lengths in front of the first (forward strand) or behind the last (reverse strand):
//                   the words lo + l, lo + l + 64, ... of [lo, hi).  Every word in that range is an S or an H by construction.
//   gdm_key         the 5' coordinate u from pos, the reference length and the clip sum, in 64 bits, and the group key
//                   refID << 34 | (u + 2^32) << 1 | strand.  The all-ones word is the sentinel of an ineligible record, so u may run from
//                   -2^32 to 2^32 - 2 and refID must be below 2^30: everything else is a bad record (GDM_BAD_U).
//   gdm_qual_share  a lane's share of the score: the QUAL bytes up to the first 4-byte boundary go as single bytes (lanes 0 .. 2), from
//                   there lane l takes the dwords l, l + 64, ..., the last 0 .. 3 bytes go as single bytes again.
// THE DECISION works on the entries {key, score} in output order: a stable sort by descending score, then a stable sort by key, leave
// every group together with its best-scoring, earliest member first.  gdm_is_dup says whether a sorted entry is a duplicate (its key
// equals its predecessor's and is not the sentinel); gdm_group_end finds the end of the group that starts at an entry by bisection.
// gdm_apply rewrites bit 0x400 of one record: a single byte store at offset 19, the high byte of the unaligned flag field.
// BOUNDS.  Every CIGAR load is checked against the record's own end (H.n) and gdc_head_words has seen that QUAL lies inside the record.
#pragma once
#include "cov.h"

enum { GDM_BAD_U = GDC_BAD_FIELDS + 1 };
enum { GDM_INELIGIBLE = 0xB04, GDM_DUP = 0x400, GDM_MIN_Q = 15 };
#define GDM_SENTINEL (~(uint64_t)0)

struct GdmStats { int64_t examined = 0, eligible = 0, duplicates = 0, max_group = 0; };

static inline const char *gdm_reason_text(uint32_t reason)
{
	return reason == GDM_BAD_U ? "the 5' coordinate or the refID leaves the range of the group key" : gdc_reason_text(reason);
}

GDB_HD uint32_t gdm_eligible(uint32_t flag, int32_t refID, int32_t pos) { return !(flag & (uint32_t)GDM_INELIGIBLE) && refID >= 0 && pos >= 0; }

// word k of the real CIGAR; *in = 0 (and 0) outside it or outside the record
GDB_HD uint32_t gdm_word(const uint8_t *rec, const GdcHead &H, uint32_t k, uint32_t *in)
{
	const uint64_t p = H.ops_at + 4ull * k;
	*in = k < H.n_ops && p + 4 <= H.n;
	return *in ? gdc_ld32(rec + p) : 0u;
}
// 1: word k is an operation other than S and H
GDB_HD uint32_t gdm_round_lane(const uint8_t *rec, const GdcHead &H, uint32_t k, uint64_t *ref, uint32_t *bad)
{
	uint32_t in;
	const uint32_t w = gdm_word(rec, H, k, &in), op = w & 15u;
	if (!in) return 0;
	if (op > 8u) *bad |= 1u;
	*ref += gds_op_ref(w);
	return op != 4u && op != 5u;
}
// the round that starts at word b0 said m (bit l: lane l): *first (n_ops while none was seen) and *last1 (index behind the last; 0: none)
GDB_HD void gdm_round_mask(uint64_t m, uint32_t b0, uint32_t n_ops, uint32_t *first, uint32_t *last1)
{
	if (!m) return;
	if (*first == n_ops) *first = b0 + (uint32_t)__builtin_ctzll(m);
	*last1 = b0 + 64u - (uint32_t)__builtin_clzll(m);
}
GDB_HD uint64_t gdm_clip_lane(const uint8_t *rec, const GdcHead &H, uint32_t lo, uint32_t hi, uint32_t lane)
{
	uint64_t s = 0;
	for (uint32_t k = lo + lane; k < hi; k += 64) {
		uint32_t in;
		s += gdm_word(rec, H, k, &in) >> 4;
	}
	return s;
}
GDB_HD uint32_t gdm_key(int32_t refID, int32_t pos, uint32_t rev, uint64_t ref_sum, uint64_t clip, uint64_t *key)
{
	const int64_t u = rev ? (int64_t)pos + (int64_t)ref_sum - 1 + (int64_t)clip : (int64_t)pos - (int64_t)clip; // (the sums are below 2^59)
	*key = GDM_SENTINEL;
	if ((uint32_t)refID >= (1u << 30) || u < -((int64_t)1 << 32) || u > ((int64_t)1 << 32) - 2) return GDM_BAD_U;
	*key = (uint64_t)(uint32_t)refID << 34 | (uint64_t)(u + ((int64_t)1 << 32)) << 1 | (rev & 1u);
	return GDC_OK;
}

GDB_HD uint32_t gdm_q(uint32_t q) { return (q >= (uint32_t)GDM_MIN_Q && q != 0xffu) ? q : 0u; }
GDB_HD uint32_t gdm_qual_share(const uint8_t *rec, const GdcHead &H, uint32_t lane)
{
	const uint8_t *qp = rec + H.qual_at;
	const uint32_t n = H.l_seq, head = (4u - (uint32_t)((uintptr_t)qp & 3u)) & 3u, h = head < n ? head : n;
	uint32_t s = 0;
	if (lane < h) s += gdm_q(qp[lane]);
	const uint32_t words = (n - h) >> 2;
#pragma unroll 1
	for (uint32_t k = lane; k < words; k += 64) {
		const uint32_t w = gdc_ld32(qp + h + 4u * k);
		s += gdm_q(w & 0xffu) + gdm_q(w >> 8 & 0xffu) + gdm_q(w >> 16 & 0xffu) + gdm_q(w >> 24);
	}
	const uint32_t t0 = h + 4u * words;
	if (lane < n - t0) s += gdm_q(qp[t0 + lane]);
	return s;
}

// ---- the decision over the sorted entries ----------------------------------------------------------------------------------------------
GDB_HD uint32_t gdm_is_dup(const uint64_t *skey, uint64_t i) { return i > 0 && skey[i] == skey[i - 1] && skey[i] != GDM_SENTINEL; }
// the first index behind i whose key differs from skey[i] (skey[0, n) is sorted)
GDB_HD uint64_t gdm_group_end(const uint64_t *skey, uint64_t n, uint64_t i)
{
	const uint64_t v = skey[i];
	uint64_t lo = i, hi = n; // skey[lo] == v, skey[hi] != v (or hi == n)
	while (hi - lo > 1) {
		const uint64_t mid = lo + (hi - lo) / 2;
		if (skey[mid] == v) lo = mid;
		else hi = mid;
	}
	return hi;
}

// ---- the rewrite -----------------------------------------------------------------------------------------------------------------------
// rec: a record of which 20 bytes at least lie inside its buffer.  An eligible record takes dup as its bit 0x400; the flag it then carries
GDB_HD uint32_t gdm_apply(uint8_t *rec, uint32_t dup)
{
	const uint32_t flag = gds_le16(rec + 18);
	if (!gdm_eligible(flag, (int32_t)gds_le32(rec + 4), (int32_t)gds_le32(rec + 8))) return flag;
	const uint32_t nf = (flag & ~(uint32_t)GDM_DUP) | (dup ? (uint32_t)GDM_DUP : 0u);
	rec[19] = (uint8_t)(nf >> 8);
	return nf;
}
// bit `b` of a bitmap of 32-bit words
GDB_HD uint32_t gdm_bit(const uint32_t *bitmap, uint64_t b) { return bitmap[b >> 5] >> (b & 31u) & 1u; }
