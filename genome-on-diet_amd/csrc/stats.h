// Read and alignment statistics from BAM alignment records (include/gdiet_hip.h, "Alignment statistics"): the statements of the
// accumulator, written once for the kernel (stats.hip.h), for the host emulator that runs them as loops over 64 lanes
// (tests/emul/stats_emul.cpp) and for the driver.  No HIP in here.  The record statements -- the head, the real CIGAR, PASS 1's verdict,
// the filter chain -- are coverage's (cov.h); the operation kinds, the runs and the reference base are the pileup's (pile.h).
//
// ONE WAVEFRONT PER RECORD, four records to a block, three passes:
//   PASS 1         coverage's validation.  gdt_classes says which summary counters the record adds 1 to and whether it is a READ, an
//                  ALIGNMENT, both or neither.  A bad record ends here: it has touched nothing.
//   READ pass      gdt_read_share: lane l takes the query indices l, l + 64, ...: the base by cycle, the quality by cycle, the quality
//                  histogram, and in registers the lane's A C G T and C G counts.  gdt_read_close, once per record: read_len, gc.
//   ALIGNMENT pass per round of 64 operations the two exclusive scans give every lane the cursors of its operation (gdp_op); every lane
//                  books its own I, D or clip (gdt_op_share), and the M = X runs of the round are taken one after another, wave-uniformly,
//                  their positions dealt over the 64 lanes (gdt_run_share): each lane reads its own SEQ nibble and its own reference base.
//                  gdt_aln_close, once per record: mapq, identity.
// THE CELLS.  Every counter is one cell of one array of GdtLayout::n_all cells: first the block tables [0, n_lds) -- gc, base_cycle,
// qual_cycle, base_qual, mapq, ins_len, del_len, subst, cmp_cycle, identity -- then read_len, then the summary.  In global memory a cell
// is uint64.  A block keeps the block tables as uint32 in local memory and flushes them into the global cells (the kernel's header says
// when); read_len and the summary are added to in global memory.  W::add(cell, v) is the add; W::add_hot(cell) adds 1 to a cell that many
// lanes of one instruction are likely to share (the device counts the lanes of a cell first and lets one of them add).
// WHAT STAYS IN REGISTERS.  The row `cycles` of the three per-cycle tables takes every cycle >= cycles -- 97 % of a 15 kb read -- so a
// lane counts its bases of that row in registers (GdtReadLane::tb tqn tqs, GdtAlnLane::tcn tcx); the wavefront reduces them once per
// record and the close adds the sums.  Matches, mismatches and the per-operation sums go the same way.
// WEIGHT.  gdt_weight(record) bounds by how much one record can raise any block-table cell: at most 254 * weight.
// BOUNDS.  Every load is checked against the record's own end (H.n) and l_seq, every reference load against the contig's length, every
// cell against its table (gdt_cell gives GDT_NO_CELL otherwise, which W::add drops): a record that contradicts itself can lose counts,
// never touch a cell outside its table.  No lane reads what another wrote: the adds are integer adds, so their order cannot matter.
#pragma once
#include "pile.h"

// the summary: coverage's ten counters, then these (gdiet_stats_summary_t)
enum {
	GDT_S_DUPLICATE = GDC_N_SUMMARY, GDT_S_QCFAIL, GDT_S_READS, GDT_S_READ_BASES, GDT_S_ALIGNED_BASES, GDT_S_MATCHES, GDT_S_MISMATCHES, GDT_S_OTHER_BASES,
	GDT_S_INS_EVENTS, GDT_S_INS_BASES, GDT_S_DEL_EVENTS, GDT_S_DEL_BASES, GDT_S_SOFT_CLIPPED, GDT_S_HARD_CLIPPED, GDT_S_NO_SEQ, GDT_S_NO_IDENTITY, GDT_N_SUMMARY
};
// the tables in the order of their cells; the first one is the only one that is not a block table (gdiet_hip_stats_table's `which`)
enum { GDT_T_GC = 0, GDT_T_BASE_CYCLE, GDT_T_QUAL_CYCLE, GDT_T_BASE_QUAL, GDT_T_MAPQ, GDT_T_INS_LEN, GDT_T_DEL_LEN, GDT_T_SUBST, GDT_T_CMP_CYCLE, GDT_T_IDENTITY, GDT_T_READ_LEN, GDT_T_SUMMARY, GDT_N_TABLES };
enum { GDT_MAX_BLOCKS = 1024 }; // of a launch: a block pays for its flush
enum { GDT_MAX_CYCLES = 1024, GDT_MAX_LEN = 1 << 20, GDT_MAX_INDEL = 4096, GDT_QUAL_BINS = 96 };
static const uint32_t GDT_NO_CELL = ~0u;
static const uint64_t GDT_DEFAULT_BOUND = 1ull << 24; // 254 * 2^24 < 2^32: the weight a block may hold between two flushes

struct GdtLayout {
	uint32_t off[GDT_N_TABLES], len[GDT_N_TABLES];
	uint32_t n_lds, n_all;
};
struct GdtOpt {
	uint32_t excl_flags, min_mapq, cycles, max_len, max_indel;
};

// the options are in range (the driver has refused anything else)
static inline GdtLayout gdt_layout(uint32_t cycles, uint32_t max_len, uint32_t max_indel)
{
	GdtLayout Y;
	const uint32_t n[GDT_N_TABLES] = {101, (cycles + 1) * 5, (cycles + 1) * 2, GDT_QUAL_BINS, 256, max_indel + 1, max_indel + 1, 25, (cycles + 1) * 2, 101, max_len + 1, GDT_N_SUMMARY};
	uint32_t at = 0;
	Y.n_lds = 0;
	for (int t = 0; t < GDT_N_TABLES; ++t) {
		if (t == GDT_T_READ_LEN) Y.n_lds = at;
		Y.off[t] = at, Y.len[t] = n[t], at += n[t];
	}
	Y.n_all = at;
	return Y;
}
// cell k of table t, or GDT_NO_CELL
GDB_HD uint32_t gdt_cell(const GdtLayout &Y, int t, uint64_t k) { return k < Y.len[t] ? Y.off[t] + (uint32_t)k : GDT_NO_CELL; }

// the base code of a SEQ nibble: 0..3 for A C G T, 4 for everything else; and its complement
GDB_HD uint32_t gdt_base_code(uint32_t nib) { return nib == 1u ? 0u : nib == 2u ? 1u : nib == 4u ? 2u : nib == 8u ? 3u : 4u; }
GDB_HD uint32_t gdt_complement(uint32_t code) { return code < 4u ? 3u - code : 4u; }

// bit i: the record adds 1 to counter i of the summary (i below GDT_S_READS); *is_read, *is_aln: the two populations
GDB_HD uint32_t gdt_classes(const GdcHead &H, uint32_t reason, uint32_t excl_flags, uint32_t min_mapq, uint32_t *is_read, uint32_t *is_aln)
{
	uint32_t bits = gdc_summary_bits(H, reason, excl_flags | 4u, min_mapq, is_aln);
	*is_read = 0;
	if (!reason && H.n) {
		if (H.flag & 0x400u) bits |= 1u << GDT_S_DUPLICATE;
		if (H.flag & 0x200u) bits |= 1u << GDT_S_QCFAIL;
		*is_read = (H.flag & (excl_flags | 0x900u)) == 0;
	}
	return bits;
}
// by how much a record can raise one block-table cell, divided by 254 (a quality byte): its bases or its operations, whichever are more
GDB_HD uint64_t gdt_weight(const GdcHead &H, uint32_t is_read, uint32_t is_aln)
{
	if (!is_read && !is_aln) return 0;
	return 1ull + (H.l_seq > H.n_ops ? H.l_seq : H.n_ops);
}

// the code of operation k of the real CIGAR if it is a clip (4 S, 5 H), else 0
GDB_HD uint32_t gdt_clip_code(const uint8_t *rec, const GdcHead &H, uint32_t k)
{
	const uint64_t p = H.ops_at + 4ull * k;
	if (k >= H.n_ops || p + 4 > H.n) return 0;
	const uint32_t op = gdc_ld32(rec + p) & 15u;
	return op == 4u || op == 5u ? op : 0u;
}
// lead, trail: the length of a hard clip that is the first / the last operation of the real CIGAR, else 0
GDB_HD void gdt_hard_ends(const uint8_t *rec, const GdcHead &H, uint32_t *lead, uint32_t *trail)
{
	*lead = *trail = 0;
	if (H.n_ops == 0) return;
	const uint64_t p0 = H.ops_at, p1 = H.ops_at + 4ull * (H.n_ops - 1);
	if (p0 + 4 <= H.n && (gdc_ld32(rec + p0) & 15u) == 5u) *lead = gdc_ld32(rec + p0) >> 4;
	if (p1 + 4 <= H.n && (gdc_ld32(rec + p1) & 15u) == 5u) *trail = gdc_ld32(rec + p1) >> 4;
}
// the row of query index qi (below l_seq) in a per-cycle table: its cycle in the read's original orientation, `cycles` for every cycle from there on
GDB_HD uint32_t gdt_cycle_row(const GdcHead &H, uint32_t lead, uint32_t trail, uint32_t cycles, uint32_t qi)
{
	const uint64_t c = H.flag & 0x10u ? (uint64_t)trail + (H.l_seq - 1u - qi) : (uint64_t)lead + qi;
	return c < cycles ? (uint32_t)c : cycles;
}
// SEQ nibble qi of the record; *ok = 0 if its byte lies outside the record
GDB_HD uint32_t gdt_nibble(const uint8_t *rec, const GdcHead &H, uint32_t qi, uint32_t *ok)
{
	const uint64_t at = H.qual_at - (H.l_seq + 1u) / 2u + (qi >> 1);
	*ok = qi < H.l_seq && at < H.n;
	return *ok ? rec[at] >> ((~qi & 1u) << 2) & 15u : 0u;
}

// ---- the READ pass ---------------------------------------------------------------------------------------------------------------------
struct GdtReadLane {
	uint32_t a, g;       // this lane's bases A C G T, and C G
	uint32_t tb[5], tqn; // its bases of row `cycles` by code; its quality bytes there
	uint64_t tqs;        // and their sum (a lane holds fewer than 2^25 bases)
};
GDB_HD void gdt_read_lane_clear(GdtReadLane *A) { A->a = A->g = A->tqn = 0, A->tqs = 0, A->tb[0] = A->tb[1] = A->tb[2] = A->tb[3] = A->tb[4] = 0; }

template <class W> GDB_HD void gdt_read_share(W &w, const GdtLayout &Y, const uint8_t *rec, const GdcHead &H, uint32_t lead, uint32_t trail, uint32_t cycles, uint32_t lane, GdtReadLane *A)
{
	const uint32_t rev = H.flag >> 4 & 1u;
#pragma unroll 1
	for (uint32_t qi = lane; qi < H.l_seq; qi += 64) {
		uint32_t ok;
		const uint32_t nib = gdt_nibble(rec, H, qi, &ok);
		if (!ok || H.qual_at + qi >= H.n) continue;
		const uint32_t stored = gdt_base_code(nib), code = rev ? gdt_complement(stored) : stored;
		const uint32_t row = gdt_cycle_row(H, lead, trail, cycles, qi);
		const bool tail = row == cycles;
		A->a += code < 4u, A->g += code == 1u || code == 2u;
		if (tail) {
#pragma unroll
			for (uint32_t c = 0; c < 5; ++c) A->tb[c] += code == c;
		} else w.add(gdt_cell(Y, GDT_T_BASE_CYCLE, 5ull * row + code), 1);
		if (!H.has_qual) continue;
		const uint32_t q = rec[H.qual_at + qi];
		if (tail) A->tqn += 1, A->tqs += q;
		else w.add(gdt_cell(Y, GDT_T_QUAL_CYCLE, 2ull * row), 1), w.add(gdt_cell(Y, GDT_T_QUAL_CYCLE, 2ull * row + 1), q);
		w.add_hot(gdt_cell(Y, GDT_T_BASE_QUAL, q < GDT_QUAL_BINS - 1u ? q : GDT_QUAL_BINS - 1u));
	}
}
// once per read, from the sums T of its lanes' registers
template <class W> GDB_HD void gdt_read_close(W &w, const GdtLayout &Y, const GdcHead &H, const GdtOpt &O, const GdtReadLane &T)
{
	w.add(gdt_cell(Y, GDT_T_READ_LEN, H.l_seq < O.max_len ? H.l_seq : O.max_len), 1);
	if (H.l_seq > 0 && T.a > 0) w.add(gdt_cell(Y, GDT_T_GC, (200ull * T.g + T.a) / (2ull * T.a)), 1);
#pragma unroll
	for (uint32_t c = 0; c < 5; ++c) w.add(gdt_cell(Y, GDT_T_BASE_CYCLE, 5ull * O.cycles + c), T.tb[c]);
	w.add(gdt_cell(Y, GDT_T_QUAL_CYCLE, 2ull * O.cycles), T.tqn), w.add(gdt_cell(Y, GDT_T_QUAL_CYCLE, 2ull * O.cycles + 1), T.tqs);
}

// ---- the ALIGNMENT pass -----------------------------------------------------------------------------------------------------------------
struct GdtAlnLane {
	uint32_t m, x, o;    // this lane's matches, mismatches and bases that are not comparable (a lane holds fewer than 2^25 bases)
	uint32_t tcn, tcx;   // its comparable bases and mismatches of row `cycles`
	uint32_t ie, de, db; // its I and D runs of length above 0; its deleted bases (below the contig's length)
	uint64_t ib, sc, hc; // its inserted, soft-clipped and hard-clipped bases
};
GDB_HD void gdt_aln_lane_clear(GdtAlnLane *A) { A->m = A->x = A->o = A->tcn = A->tcx = A->ie = A->de = A->db = 0, A->ib = A->sc = A->hc = 0; }

// a lane's own operation k, of kind `kind` (gdp_op) and length L: an indel into its histogram and the sums, a clip into the sums
template <class W> GDB_HD void gdt_op_share(W &w, const GdtLayout &Y, const uint8_t *rec, const GdcHead &H, uint32_t max_indel, uint32_t k, uint32_t kind, uint32_t L, GdtAlnLane *A)
{
	if (L == 0) return;
	if (kind == GDP_K_INS) w.add(gdt_cell(Y, GDT_T_INS_LEN, L < max_indel ? L : max_indel), 1), A->ie += 1, A->ib += L;
	else if (kind == GDP_K_DEL) w.add(gdt_cell(Y, GDT_T_DEL_LEN, L < max_indel ? L : max_indel), 1), A->de += 1, A->db += L;
	else if (kind == GDP_K_NONE) {
		const uint32_t clip = gdt_clip_code(rec, H, k);
		if (clip == 4u) A->sc += L;
		else if (clip == 5u) A->hc += L;
	}
}
// Lane `lane` of 64: its share of the M = X run of len bases at reference position s of the contig (clen bases, its first base is base
// seq_base of S) whose first query base is q.  Everything but `lane` is wave-uniform.  H.l_seq > 0.
template <class W> GDB_HD void gdt_run_share(W &w, const GdtLayout &Y, const uint8_t *rec, const GdcHead &H, const uint32_t *S, uint64_t seq_base, uint32_t clen, uint32_t lead, uint32_t trail,
                                             uint32_t cycles, uint32_t s, uint32_t len, uint32_t q, uint32_t lane, GdtAlnLane *A)
{
#pragma unroll 1
	for (uint32_t b = lane; b < len; b += 64) {
		const uint64_t qi = (uint64_t)q + b, p = (uint64_t)s + b;
		if (qi >= H.l_seq || p >= clen) continue; // (PASS 1 has seen the query end inside l_seq and the reference end inside the contig)
		uint32_t ok;
		const uint32_t rc = gdt_base_code(gdt_nibble(rec, H, (uint32_t)qi, &ok));
		if (!ok) continue;
		const uint32_t fc = gdp_ref_base(S, seq_base + p);
		w.add_hot(gdt_cell(Y, GDT_T_SUBST, 5u * fc + rc));
		const bool cmp = rc < 4u && fc < 4u, mis = cmp && rc != fc;
		A->m += cmp && !mis, A->x += mis, A->o += !cmp;
		if (!cmp) continue;
		const uint32_t row = gdt_cycle_row(H, lead, trail, cycles, (uint32_t)qi);
		if (row == cycles) A->tcn += 1, A->tcx += mis;
		else {
			w.add(gdt_cell(Y, GDT_T_CMP_CYCLE, 2ull * row), 1);
			if (mis) w.add(gdt_cell(Y, GDT_T_CMP_CYCLE, 2ull * row + 1), 1);
		}
	}
}

// what a record adds to the summary's counters from GDT_S_READS on
struct GdtRecord {
	uint64_t v[GDT_N_SUMMARY - GDT_S_READS];
};
GDB_HD void gdt_record_clear(GdtRecord *R)
{
#pragma unroll
	for (int i = 0; i < GDT_N_SUMMARY - GDT_S_READS; ++i) R->v[i] = 0;
}
// once per alignment, from the sums of its lanes' registers: the adds ...
template <class W> GDB_HD void gdt_aln_close(W &w, const GdtLayout &Y, const GdcHead &H, const GdtOpt &O, uint64_t m, uint64_t x, uint64_t tcn, uint64_t tcx, uint64_t ie, uint64_t de)
{
	w.add(gdt_cell(Y, GDT_T_MAPQ, H.mapq), 1);
	w.add(gdt_cell(Y, GDT_T_CMP_CYCLE, 2ull * O.cycles), tcn), w.add(gdt_cell(Y, GDT_T_CMP_CYCLE, 2ull * O.cycles + 1), tcx);
	const uint64_t den = m + x + ie + de;
	if (den) w.add(gdt_cell(Y, GDT_T_IDENTITY, 100ull * m / den), 1);
}
// ... and what it adds to the summary
GDB_HD void gdt_aln_record(const GdcHead &H, uint64_t m, uint64_t x, uint64_t o, uint64_t ie, uint64_t ib, uint64_t de, uint64_t db, uint64_t sc, uint64_t hc, GdtRecord *R)
{
	R->v[GDT_S_ALIGNED_BASES - GDT_S_READS] = m + x + o, R->v[GDT_S_MATCHES - GDT_S_READS] = m, R->v[GDT_S_MISMATCHES - GDT_S_READS] = x, R->v[GDT_S_OTHER_BASES - GDT_S_READS] = o;
	R->v[GDT_S_INS_EVENTS - GDT_S_READS] = ie, R->v[GDT_S_INS_BASES - GDT_S_READS] = ib, R->v[GDT_S_DEL_EVENTS - GDT_S_READS] = de, R->v[GDT_S_DEL_BASES - GDT_S_READS] = db;
	R->v[GDT_S_SOFT_CLIPPED - GDT_S_READS] = sc, R->v[GDT_S_HARD_CLIPPED - GDT_S_READS] = hc;
	R->v[GDT_S_NO_SEQ - GDT_S_READS] = H.l_seq == 0, R->v[GDT_S_NO_IDENTITY - GDT_S_READS] = m + x + ie + de == 0;
}
