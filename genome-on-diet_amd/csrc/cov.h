// Coverage and depth from BAM alignment records (include/gdiet_hip.h, "Coverage"): the statements of the accumulator, written once for the
// kernels (cov.hip.h), for the host emulator that runs them as loops over 64 lanes (tests/emul/cov_emul.cpp) and for the driver.  No HIP
// in here.  Like the sort pass (bam_sort.h, whose byte loads and GDS_FIXED layout it uses) it reads nothing but the records' own bytes.
//
// ONE WAVEFRONT PER RECORD, two passes over the operations of the real CIGAR (the record's words, or the CG:B:I array of a placeholder),
// lane l taking the words l, l + 64, ...:
//   gdc_head       the fixed fields, where the operations and the qualities are, and the CG array of a placeholder: wave-uniform.
//   gdc_op         one operation: its length, what it consumes of the reference and of the query, whether it is M = X.
//   PASS 1         validation only: every lane sums the reference and query lengths of its words (gdc_op), the sums are reduced, and
//   gdc_decide     says wave-uniformly whether the record is bad; gdc_summary_bits which of the ten summary counters it adds 1 to and
//                  whether it is counted.  A bad record ends here: it has touched nothing.
//   PASS 2         the scatter, per round of 64 operations: two exclusive wave scans (reference and query consumed; a shuffle ladder on
//                  the device, a loop on the host) with a wave-uniform carry from round to round give every lane the cursors of its
//                  operation, and a lane whose operation is M = X adds +1 / -1 to the difference array (gdc_scatter).
//   gdc_qual_share the quality sum of ONE run, spread over the wavefront: the round's runs are taken one after another, wave-uniformly
//                  (start and length of the run's lane by readlane), and lane l sums the bytes q + l, q + l + 64, ...: a HiFi run of
//                  thousands of bases is 64 lanes' work, not one lane's.  One wave reduction per record closes the sum.
// THE DIFFERENCE ARRAY is int32, total_len + 1 slots, the contigs back to back at base[rid] (64-bit: GRCh38 is above 2^32).  A run
// [r, r + len) of contig c adds +1 at base[c] + r and -1 at base[c] + r + len: a run that ends at its contig's end puts its -1 on slot 0
// of the next contig (or on the array's last slot), where the inclusive sum needs it -- the depth of that slot is then what the next
// contig's own runs make it.  After the sum (gdc_window_share reads it) slot i is the depth of position i as uint32.
// BOUNDS.  Every load is checked against the record's own end (H.n) and every add against [base[c], base[c] + len[c]]: a record that
// contradicts itself can lose counts, never touch a slot outside its contig.  No lane reads what another wrote: the adds are integer
// atomics, so their order cannot matter.
#pragma once
#include "bam_sort.h"

enum { GDC_OK = 0, GDC_BAD_REF, GDC_BAD_POS, GDC_BAD_OP, GDC_BAD_REF_END, GDC_BAD_QRY_END, GDC_BAD_CG, GDC_BAD_AUX, GDC_BAD_FIELDS };
// the summary's counters in the order of gdiet_cov_summary_t, and a contig's in the order of gdiet_cov_contig_t
enum { GDC_S_RECORDS = 0, GDC_S_UNMAPPED, GDC_S_SECONDARY, GDC_S_SUPPLEMENTARY, GDC_S_PRIMARY_MAPPED, GDC_S_REVERSE, GDC_S_EXCL_FLAG, GDC_S_EXCL_MAPQ, GDC_S_COUNTED, GDC_S_BAD, GDC_N_SUMMARY };
enum { GDC_C_READS = 0, GDC_C_COV, GDC_C_DEPTH, GDC_C_MAPQ, GDC_C_BASEQ, GDC_C_NBASEQ, GDC_N_CONTIG };

static inline const char *gdc_reason_text(uint32_t reason)
{
	static const char *const T[] = {"no error", "refID is not below n_ref", "a placed record with pos below 0", "an operation code above 8", "the reference end lies past the contig",
	                                "the query end lies past l_seq", "a placeholder CIGAR without a well-formed CG:B:I tag", "the aux fields leave the record",
	                                "the fields leave the record"};
	return T[reason <= GDC_BAD_FIELDS ? reason : 0];
}

// a 32-bit little-endian field at any alignment: a 4-byte memcpy, which gfx950 executes as one unaligned dword load (the kernel's
// registers are few: four byte loads per field would keep four of them busy each)
#if !defined(__BYTE_ORDER__) || __BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__
#error "cov.h reads little-endian fields with memcpy"
#endif
GDB_HD uint32_t gdc_ld32(const uint8_t *p)
{
	uint32_t w;
	memcpy(&w, p, 4);
	return w;
}

struct GdcHead {
	uint64_t n;       // the record's size (4 + block_size); 0: its fixed bytes or its block_size leave the buffer
	uint64_t ops_at;  // the real CIGAR: n_ops words from this offset of the record
	uint64_t qual_at;
	int32_t refID, pos;
	uint32_t n_ops, mapq, flag, l_seq, has_qual;
};

// the CG:B:I array of a placeholder: the aux fields from `at` on, types A c C s S i I f Z H B.  GDC_OK with ops_at / n_ops set.
GDB_HD uint32_t gdc_find_cg(const uint8_t *r, uint64_t n, uint64_t at, GdcHead *H)
{
	while (at < n) {
		if (n - at < 3) return GDC_BAD_AUX;
		const uint32_t t = r[at + 2];
		const bool cg = r[at] == 'C' && r[at + 1] == 'G';
		at += 3;
		uint64_t sz = 0;
		if (t == 'A' || t == 'c' || t == 'C') sz = 1;
		else if (t == 's' || t == 'S') sz = 2;
		else if (t == 'i' || t == 'I' || t == 'f') sz = 4;
		else if (t == 'Z' || t == 'H') {
			uint64_t z = at;
			while (z < n && r[z]) ++z;
			if (z >= n) return GDC_BAD_AUX;
			sz = z + 1 - at;
		} else if (t == 'B') {
			if (n - at < 5) return GDC_BAD_AUX;
			const uint32_t sub = r[at], cnt = gdc_ld32(r + at + 1);
			const uint32_t w = (sub == 'c' || sub == 'C') ? 1u : (sub == 's' || sub == 'S') ? 2u : (sub == 'i' || sub == 'I' || sub == 'f') ? 4u : 0u;
			if (!w || cnt > 0x7fffffffu) return GDC_BAD_AUX;
			sz = 5 + (uint64_t)w * cnt;
			if (cg) {
				if (sub != 'I' || n - at < sz) return GDC_BAD_CG;
				H->ops_at = at + 5, H->n_ops = cnt;
				return GDC_OK;
			}
		} else return GDC_BAD_AUX;
		if (cg) return GDC_BAD_CG; // a CG tag of another type
		if (n - at < sz) return GDC_BAD_AUX;
		at += sz;
	}
	return GDC_BAD_CG; // no CG tag
}

// The record at r, of which `avail` >= GDS_FIXED bytes lie inside the buffer, from the nine words w of its fixed bytes (the kernel loads them
// with one instruction, lane i word i, and hands them on as scalars).  GDC_OK, or why it is bad; H.n != 0 says the fixed fields were read.
GDB_HD uint32_t gdc_head_words(const uint8_t *r, uint64_t avail, const uint32_t *w, GdcHead *H)
{
	H->n = 0, H->ops_at = H->qual_at = 0, H->refID = H->pos = -1, H->n_ops = H->mapq = H->flag = H->l_seq = H->has_qual = 0;
	const uint32_t bs = w[0];
	if (bs < 32u || bs > 0x7ffffffbu || avail - 4 < bs) return GDC_BAD_FIELDS;
	const uint64_t n = (uint64_t)bs + 4;
	H->n = n, H->refID = (int32_t)w[1], H->pos = (int32_t)w[2], H->mapq = w[3] >> 8 & 0xffu, H->flag = w[4] >> 16; // w[3]: l_read_name, mapq, bin; w[4]: n_cigar_op, flag
	const uint32_t l_seq = w[5], n_cig = w[4] & 0xffffu;
	if (l_seq > 0x7fffffffu) return GDC_BAD_FIELDS;
	const uint64_t cig_at = GDS_FIXED + (uint64_t)(w[3] & 0xffu), qual_at = cig_at + 4ull * n_cig + (l_seq + 1u) / 2u, aux_at = qual_at + l_seq;
	if (aux_at > n) return GDC_BAD_FIELDS;
	H->l_seq = l_seq, H->ops_at = cig_at, H->n_ops = n_cig, H->qual_at = qual_at;
	H->has_qual = l_seq > 0 && r[qual_at] != 0xffu;
	if (n_cig == 2 && gdc_ld32(r + cig_at) == (l_seq << 4 | 4u) && (gdc_ld32(r + cig_at + 4) & 15u) == 3u) { // the placeholder of SAM specification 4.2.2
		H->n_ops = 0;
		return gdc_find_cg(r, n, aux_at, H);
	}
	return GDC_OK;
}
// The record that starts at buf + at, in a buffer of len bytes (the host's form: the emulator and tests of the statements)
GDB_HD uint32_t gdc_head(const uint8_t *buf, uint64_t len, uint64_t at, GdcHead *H)
{
	if (at > len || len - at < GDS_FIXED) {
		H->n = 0, H->ops_at = H->qual_at = 0, H->refID = H->pos = -1, H->n_ops = H->mapq = H->flag = H->l_seq = H->has_qual = 0;
		return GDC_BAD_FIELDS;
	}
	uint32_t w[GDS_FIXED / 4];
	for (int i = 0; i < GDS_FIXED / 4; ++i) w[i] = gdc_ld32(buf + at + 4 * i);
	return gdc_head_words(buf + at, len - at, w, H);
}

// operation k of the real CIGAR: 1 if it is M = X; its length, what it consumes of the reference and of the query; *bad |= 1 for a code above 8
GDB_HD uint32_t gdc_op(const uint8_t *rec, const GdcHead &H, uint32_t k, uint32_t *len, uint32_t *rl, uint32_t *ql, uint32_t *bad)
{
	*len = *rl = *ql = 0;
	const uint64_t p = H.ops_at + 4ull * k;
	if (k >= H.n_ops || p + 4 > H.n) return 0;
	const uint32_t w = gdc_ld32(rec + p), op = w & 15u, L = w >> 4;
	if (op > 8u) { *bad |= 1u; return 0; }
	const uint32_t m = op == 0u || op == 7u || op == 8u;
	*len = L;
	*rl = (m || op == 2u || op == 3u) ? L : 0u;
	*ql = (m || op == 1u || op == 4u) ? L : 0u;
	return m;
}

// PASS 1's verdict from the head's, the reduced sums and the contig table (clen[0, n_ref))
GDB_HD uint32_t gdc_decide(const GdcHead &H, uint32_t head_reason, uint32_t n_ref, const uint32_t *clen, uint64_t ref_sum, uint64_t qry_sum, uint32_t bad_op)
{
	if (head_reason) return head_reason;
	if (H.refID >= 0 && (uint32_t)H.refID >= n_ref) return GDC_BAD_REF;
	if (H.refID >= 0 && H.pos < 0) return GDC_BAD_POS;
	if (bad_op) return GDC_BAD_OP;
	if (H.refID >= 0 && (uint64_t)(uint32_t)H.pos + ref_sum > clen[H.refID]) return GDC_BAD_REF_END;
	if (H.l_seq > 0 && qry_sum > H.l_seq) return GDC_BAD_QRY_END;
	return GDC_OK;
}

// bit i: the record adds 1 to counter i of the summary; *counted: it goes through PASS 2
GDB_HD uint32_t gdc_summary_bits(const GdcHead &H, uint32_t reason, uint32_t excl_flags, uint32_t min_mapq, uint32_t *counted)
{
	uint32_t bits = 1u << GDC_S_RECORDS;
	const uint32_t f = H.flag;
	*counted = 0;
	if (H.n) {
		if (f & 4u) bits |= 1u << GDC_S_UNMAPPED;
		if (f & 0x100u) bits |= 1u << GDC_S_SECONDARY;
		if (f & 0x800u) bits |= 1u << GDC_S_SUPPLEMENTARY;
		if (!(f & 0x904u)) bits |= 1u << GDC_S_PRIMARY_MAPPED;
		if (!(f & 4u) && (f & 0x10u)) bits |= 1u << GDC_S_REVERSE;
	}
	if (reason) bits |= 1u << GDC_S_BAD;
	else if (f & excl_flags) bits |= 1u << GDC_S_EXCL_FLAG;
	else if (H.mapq < min_mapq) bits |= 1u << GDC_S_EXCL_MAPQ;
	else if (H.refID >= 0) bits |= 1u << GDC_S_COUNTED, *counted = 1;
	return bits;
}

// the run [r, r + len) of a contig of clen bases at base: add(slot, +1 / -1); the kernel's add is an atomic, the emulator's a plain one
template <class Add> GDB_HD void gdc_scatter(Add add, int32_t *diff, uint64_t base, uint32_t clen, uint64_t r, uint32_t len)
{
	if (len == 0 || r + len > clen) return;
	add(diff + base + r, 1);
	add(diff + base + r + len, -1);
}

// lane `lane` of 64: its share of the quality bytes of the run of len (below 2^28) query bases from query position q.  Only bases below
// l_seq are read, and gdc_head_words has seen that qual_at + l_seq lies inside the record: no load leaves it.  The share is below 2^30.
GDB_HD uint32_t gdc_qual_share(const uint8_t *rec, const GdcHead &H, uint32_t q, uint32_t len, uint32_t lane)
{
	if (q >= H.l_seq) return 0;
	const uint32_t lim = len < H.l_seq - q ? len : H.l_seq - q;
	const uint8_t *qp = rec + H.qual_at + q;
	uint32_t s = 0;
#pragma unroll 1
	for (uint32_t b = lane; b < lim; b += 64) s += qp[b];
	return s;
}

// ---- the window reduction over the summed array -------------------------------------------------------------------------------------------
// Window w of all (wbase[rid] <= w < wbase[rid + 1]: contig rid has ceil(len / window) of them): its positions [*beg, *end) of the array
GDB_HD uint32_t gdc_window_range(const uint64_t *base, const uint64_t *wbase, uint32_t n_ref, uint32_t window, uint64_t w, uint64_t *beg, uint64_t *end)
{
	uint32_t lo = 0, hi = n_ref; // the last rid with wbase[rid] <= w
	while (hi - lo > 1) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (wbase[mid] <= w) lo = mid;
		else hi = mid;
	}
	const uint64_t b = base[lo] + (w - wbase[lo]) * window, e = b + window;
	*beg = b < base[lo + 1] ? b : base[lo + 1], *end = e < base[lo + 1] ? e : base[lo + 1];
	return lo;
}
// lane `lane` of 64: its share of the positions with depth > 0 and of the depth sum of [beg, end)
GDB_HD void gdc_window_share(const uint32_t *depth, uint64_t beg, uint64_t end, uint32_t lane, uint32_t *cov, uint64_t *sum)
{
	uint32_t c = 0;
	uint64_t s = 0;
	for (uint64_t j = beg + lane; j < end; j += 64) {
		const uint32_t d = depth[j];
		s += d, c += d != 0u;
	}
	*cov = c, *sum = s;
}
