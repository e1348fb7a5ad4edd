// One SAM line from one row of a flat record table: its size and its bytes, written once for the kernel (sam_encode.hip.h: one wavefront
// per line), for the host emulator that runs the same statements as loops over 64 lanes (tests/emul/sam_emul.cpp) and for the driver,
// which sizes the lines while it flattens them (sam_flatten.h).  The sibling of bam_record.h, whose helpers it uses.  No HIP in here: the
// one cross-lane step (gds_wave_scan) is a shuffle ladder in the device's compilation and a loop in the host's.
//
// WHAT A LINE IS.  The bytes gd_write_sam (map_host.h) appends for the same alignment, and the '\n' the batch formatter puts behind them:
//   QNAME \t FLAG \t RNAME \t POS \t MAPQ \t CIGAR \t*\t0\t0\t SEQ \t QUAL [RG] NM ms AS nn tp cm s1 [s2] de [SA] [cs|MD] [CG:B:I] rl [comment] \n
// and, for a read without alignments, QNAME \t 4 \t*\t0\t0\t*\t*\t0\t0\t SEQ \t QUAL [RG] rl [comment] \n.  The table row (GdsRec) holds the
// line's numbers and the places of everything variable:
//   * the read's name, SEQ and QUAL as ASCII in a text pool, as in bam_record.h;
//   * the alignment's CIGAR operations (len << 4 | op) in a pool of 32-bit words; the clips are two scalars and a letter;
//   * three byte blobs the host has laid out ready to copy, because only the host holds their text -- here they are SAM text:
//     [0] "\tRG:Z:<id>", [1] the SA tag of gd_write_sa_tag and the tag of gd_write_ds_tag, [2] "\t<comment>";
//   * the text of de:f: ("0", or "%.4f": at most 15 bytes), formatted by the host: no float is formatted on the device;
//   * RNAME as the record's rid: the index's contig names are one pool and an offset table, shared by all rows.
// HOW THE WORK IS SPLIT.  Per element, lane l takes the elements l, l + 64, ...: the name, RNAME, SEQ (reversed and complemented on the
// reverse strand: letters through the reference's comp_tab, keeping their case; every other byte unchanged), QUAL (reversed) and the
// blobs.  The CIGAR column is a run of elements of unequal width -- operation k is a decimal number and a letter -- so the place of an
// element is a prefix sum: every round of 64 operations takes an inclusive wave scan of the widths, a wave-uniform carry passes from round
// to round, and every lane then writes its own digits.  The clips are operations like the others (gds_clipped_op).  The same loop with
// other widths writes ",<word>" per operation of the CG:B:I tag.  The scalar fields (FLAG, POS, MAPQ, the fixed runs, the numeric tags
// with their "\tXX:i:" prefixes, the de text, "\trl:i:0", '\n') sit at places that follow from wave-uniform width arithmetic
// (gds_dec_width), and the lanes 0 .. width - 1 of a field each store one byte of it.  No lane reads what another lane wrote.
// SIZES are pure arithmetic on the row (gds_line_size).  The one quantity that needs the operations -- the text length of the CIGAR
// column, and of the CG:B:I list -- is summed by the host while it copies the CIGAR into the pool, and stored in the row.
// BOUNDS.  Every store is a byte store checked against the line's own end (GdbOut::end = GdsRec::size, through gdb_st): a row that
// disagrees with its size can lose bytes, never write outside its line.
// THE RULES are gd_write_sam's, not BAM's: a name of any length, a comment of any text, the CIGAR in the tag only under MM_F_LONG_CIGAR
// (with its placeholder <slen>S<re - rs>N), the difference tag in front of CG:B:I.
#pragma once
#include "bam_record.h"

struct GdsRec {
	uint64_t out;         // where the line starts in the stream
	uint64_t size;        // its bytes, the '\n' included (gds_line_size of the row)
	uint64_t name;        // text pool: l_name bytes
	uint64_t seq, qual;   // text pool: the first base / quality of the slice printed, in read order
	uint64_t cig;         // CIGAR pool: n_cig words
	uint64_t blob[3];     // blob pool
	uint64_t de[2];       // the text behind "\tde:f:", byte k in bits 8 (k & 7) .. of de[k >> 3]
	uint32_t blob_len[3];
	uint32_t de_len;      // <= 15
	uint32_t l_name;
	uint32_t flag, mapq;
	uint32_t rid, l_rname; // mapped: the contig and the length of its name
	int32_t pos;          // rs + 1
	uint32_t l_seq;       // bytes of SEQ
	uint32_t seq_star;    // SEQ and QUAL are "*" (a secondary record without -Y); l_seq is 0 then
	uint32_t rev;         // SEQ reversed and complemented, QUAL reversed
	uint32_t has_qual;    // 0: QUAL is "*"
	uint32_t n_cig, clip0, clip1, clip_ch; // the alignment's operations; clip lengths (0: none) and their letter ('S' or 'H')
	uint32_t cig_text;    // bytes of the CIGAR column when the operations are printed there: clips included
	uint32_t in_tag;      // the column holds the placeholder <ph_s>S<ph_n>N, and CG:B:I sits behind blob[1]
	int32_t ph_s, ph_n;
	uint32_t cg_text;     // in_tag: bytes of ",<word>" over all operations, clips included
	uint32_t mapped, has_p, has_s2; // tp cm s1 [s2] on every mapped record; the CIGAR, NM ms AS nn and de with has_p
	uint32_t tp;          // 'P' or 'S'
	int32_t nm, ms, as, cm, s1, s2;
	uint32_t nn;
};

// ---- decimal numbers as gd_fmt_int prints them; every number of a line is an int32 or a uint32, so |v| < 2^32 -------------------------
GDB_HD uint32_t gds_u32_width(uint32_t u)
{
	return u < 10u ? 1u : u < 100u ? 2u : u < 1000u ? 3u : u < 10000u ? 4u : u < 100000u ? 5u : u < 1000000u ? 6u : u < 10000000u ? 7u : u < 100000000u ? 8u : u < 1000000000u ? 9u : 10u;
}
GDB_HD uint32_t gds_dec_width(int64_t v) { return v < 0 ? 1u + gds_u32_width((uint32_t)(0 - (uint64_t)v)) : gds_u32_width((uint32_t)v); }
GDB_HD uint32_t gds_pow10(uint32_t d)
{
	return d == 0 ? 1u : d == 1 ? 10u : d == 2 ? 100u : d == 3 ? 1000u : d == 4 ? 10000u : d == 5 ? 100000u : d == 6 ? 1000000u : d == 7 ? 10000000u : d == 8 ? 100000000u : 1000000000u;
}
// up to eight bytes of fixed text in one 64-bit constant, byte k in bits 8 k ..
constexpr uint64_t gds_pack(const char *s, int from = 0)
{
	uint64_t v = 0;
	int n = 0;
	while (s[n]) ++n;
	for (int k = 0; k < 8 && from + k < n; ++k) v |= (uint64_t)(uint8_t)s[from + k] << (8 * k);
	return v;
}
GDB_HD uint32_t gds_byte(uint64_t lo, uint64_t hi, uint32_t k) { return (uint32_t)((k < 8u ? lo >> (8u * k) : hi >> (8u * (k - 8u))) & 255u); }
// a field of n <= 16 fixed bytes: lane k stores byte k
GDB_HD uint64_t gds_lit(const GdbOut &o, uint64_t at, uint32_t lane, uint64_t lo, uint64_t hi, uint32_t n)
{
	if (lane < n) gdb_st(o, at + lane, gds_byte(lo, hi, lane));
	return at + n;
}
// pre (p bytes, p <= 8) and the decimal text of v behind it: lane k stores byte k of the p + width bytes
GDB_HD uint64_t gds_int(const GdbOut &o, uint64_t at, uint32_t lane, uint64_t pre, uint32_t p, int64_t v)
{
	const uint32_t neg = v < 0 ? 1u : 0u, u = neg ? (uint32_t)(0 - (uint64_t)v) : (uint32_t)v, w = neg + gds_u32_width(u);
	if (lane < p) gdb_st(o, at + lane, gds_byte(pre, 0, lane));
	else if (lane < p + w) {
		const uint32_t k = lane - p;
		gdb_st(o, at + lane, neg && k == 0 ? (uint32_t)'-' : '0' + (u / gds_pow10(w - 1u - k)) % 10u);
	}
	return at + p + w;
}
GDB_HD uint64_t gds_tag_int(const GdbOut &o, uint64_t at, uint32_t lane, char a, char b, int64_t v)
{
	return gds_int(o, at, lane, (uint64_t)'\t' | (uint64_t)(uint8_t)a << 8 | (uint64_t)(uint8_t)b << 16 | (uint64_t)':' << 24 | (uint64_t)'i' << 32 | (uint64_t)':' << 40, 6, v);
}

// ---- the complement of gd_write_sam's put_seq: comp_tab on letters, which keep their case; any other byte as it is --------------------
struct GdsComp { uint64_t w[3]; }; // 26 letters as 5-bit offsets from 'A', twelve to a word
constexpr GdsComp gds_make_comp()
{
	const char comp[] = "TVGHEFCDIJMLKNOPQYSAABWXRZ";
	GdsComp t = {{0, 0, 0}};
	for (int l = 0; l < 26; ++l) t.w[l / 12] |= (uint64_t)(comp[l] - 'A') << (5 * (l % 12));
	return t;
}
GDB_HD uint32_t gds_comp(uint32_t c)
{
	constexpr GdsComp T = gds_make_comp();
	const uint32_t l = (c | 32u) - 'a';
	if (l >= 26u || c < 'A' || c >= 128u) return c;
	const uint64_t w = l < 12u ? T.w[0] : l < 24u ? T.w[1] : T.w[2];
	const uint32_t k = l < 12u ? l : l < 24u ? l - 12u : l - 24u;
	return (c & ~31u) + 1u + (uint32_t)((w >> (5u * k)) & 31u); // 'A' or 'a', whichever c is
}

// ---- the CIGAR with its clips as one run of operations ----------------------------------------------------------------------------------
GDB_HD uint32_t gds_ops(const GdsRec &r) { return r.n_cig + (r.clip0 ? 1u : 0u) + (r.clip1 ? 1u : 0u); }
GDB_HD uint32_t gds_clipped_op(const GdsRec &r, const uint32_t *cig, uint32_t k)
{
	const uint32_t lead = r.clip0 ? 1u : 0u, code = r.clip_ch == 'H' ? 5u : 4u;
	if (k < lead) return r.clip0 << 4 | code;
	if (k - lead < r.n_cig) return cig[r.cig + (k - lead)];
	return r.clip1 << 4 | code;
}
GDB_HD uint32_t gds_op_letter(uint32_t op)
{
	const uint32_t c = op & 15u;
	constexpr uint64_t K = gds_pack("MIDNSHP=");
	return c < 8u ? gds_byte(K, 0, c) : c == 8u ? (uint32_t)'X' : c == 9u ? (uint32_t)'B' : (uint32_t)'?';
}
// bytes of element k of a run over n operations: "<len><letter>" in the CIGAR column, ",<word>" in the CG:B:I list; 0 behind the run
GDB_HD uint32_t gds_run_width(const GdsRec &r, const uint32_t *cig, uint32_t k, uint32_t n, uint32_t list)
{
	if (k >= n) return 0;
	const uint32_t op = gds_clipped_op(r, cig, k);
	return 1u + gds_u32_width(list ? op : op >> 4);
}
// the inclusive prefix sum over the lanes of a wavefront of the widths of the elements base .. base + 63 (mine: this lane's), and their
// total.  On the device a ladder of six shuffles; on the host the same sums as a loop, so that the result cannot depend on lane order.
GDB_HD uint32_t gds_wave_scan(const GdsRec &r, const uint32_t *cig, uint32_t base, uint32_t n, uint32_t list, uint32_t lane, uint32_t mine, uint32_t *total)
{
#if defined(__HIP_DEVICE_COMPILE__)
	(void)r, (void)cig, (void)base, (void)n, (void)list;
	uint32_t s = mine;
#pragma unroll
	for (uint32_t d = 1; d < 64; d <<= 1) {
		const uint32_t t = __shfl_up(s, d, 64);
		if (lane >= d) s += t;
	}
	*total = (uint32_t)__builtin_amdgcn_readlane((int)s, 63);
	return s;
#else
	(void)mine;
	uint32_t s = 0, t = 0;
	for (uint32_t j = 0; j < 64; ++j) {
		const uint32_t w = gds_run_width(r, cig, base + j, n, list);
		t += w;
		if (j <= lane) s += w;
	}
	*total = t;
	return s;
#endif
}
GDB_HD uint64_t gds_run(const GdbOut &o, uint64_t at, const GdsRec &r, const uint32_t *cig, uint32_t list, uint32_t lane)
{
	const uint32_t n = gds_ops(r);
	for (uint32_t base = 0; base < n; base += 64) { // (sam_flatten.h refuses 2^31 operations: base cannot wrap)
		const uint32_t k = base + lane, w = gds_run_width(r, cig, k, n, list);
		uint32_t total;
		const uint32_t incl = gds_wave_scan(r, cig, base, n, list, lane, w, &total);
		if (w) {
			const uint32_t op = gds_clipped_op(r, cig, k);
			uint64_t p = at + incl; // one past the element
			if (!list) gdb_st(o, --p, gds_op_letter(op));
			uint32_t u = list ? op : op >> 4;
			do gdb_st(o, --p, '0' + u % 10u), u /= 10u; while (u);
			if (list) gdb_st(o, --p, ',');
		}
		at += total;
	}
	return at;
}

// ---- sizes --------------------------------------------------------------------------------------------------------------------------------
GDB_HD uint64_t gds_cigar_col_size(const GdsRec &r)
{
	if (!r.has_p) return 1; // "*"
	if (r.in_tag) return (uint64_t)gds_dec_width(r.ph_s) + 1 + gds_dec_width(r.ph_n) + 1;
	return r.cig_text;
}
GDB_HD uint64_t gds_num_tags_size(const GdsRec &r)
{
	if (!r.mapped) return 0;
	uint64_t n = 7 /* \ttp:A:P */ + (6 + gds_dec_width(r.cm)) + (6 + gds_dec_width(r.s1));
	if (r.has_s2) n += 6 + gds_dec_width(r.s2);
	if (r.has_p) n += (6 + gds_dec_width(r.nm)) + (6 + gds_dec_width(r.ms)) + (6 + gds_dec_width(r.as)) + (6 + gds_dec_width((int64_t)r.nn)) + 6 + r.de_len;
	return n;
}
GDB_HD uint64_t gds_line_size(const GdsRec &r)
{
	uint64_t n = (uint64_t)r.l_name + 1 + gds_dec_width((int64_t)r.flag);
	if (r.mapped) n += 1 + (uint64_t)r.l_rname + 1 + gds_dec_width(r.pos) + 1 + gds_dec_width((int64_t)r.mapq) + 1 + gds_cigar_col_size(r) + 7;
	else n += 15;
	n += r.seq_star ? 3 : (uint64_t)r.l_seq + 1 + (r.has_qual ? (uint64_t)r.l_seq : 1);
	n += (uint64_t)r.blob_len[0] + gds_num_tags_size(r) + r.blob_len[1];
	if (r.in_tag) n += 7 + (uint64_t)r.cg_text;
	return n + 7 /* \trl:i:0 */ + r.blob_len[2] + 1;
}

// Lane `lane` of the wavefront that writes line r at stream + r.out.  rname / rname_off: the contig names behind one another and where
// each starts.  Returns the number of bytes the line takes as the fields give it (the caller may compare it with r.size).
GDB_HD uint64_t gds_format(const GdsRec &r, const uint8_t *text, const uint32_t *cig, const uint8_t *blob, const uint8_t *rname, const uint64_t *rname_off, uint8_t *stream,
                           uint32_t lane)
{
	constexpr uint64_t K_MATE = gds_pack("\t*\t0\t0\t"), K_UN0 = gds_pack("\t*\t0\t0\t*\t*\t0\t0\t"), K_UN1 = gds_pack("\t*\t0\t0\t*\t*\t0\t0\t", 8), K_STARS = gds_pack("*\t*");
	constexpr uint64_t K_TP = gds_pack("\ttp:A:"), K_DE = gds_pack("\tde:f:"), K_CG = gds_pack("\tCG:B:I"), K_RL = gds_pack("\trl:i:0");
	GdbOut o;
	o.p = stream + r.out, o.end = r.size;
	uint64_t at = gdb_copy(o, 0, lane, text + r.name, r.l_name);
	at = gds_int(o, at, lane, '\t', 1, (int64_t)r.flag);
	if (r.mapped) {
		if (lane == 0) gdb_st(o, at, '\t');
		at = gdb_copy(o, at + 1, lane, rname + rname_off[r.rid], r.l_rname);
		at = gds_int(o, at, lane, '\t', 1, r.pos);
		at = gds_int(o, at, lane, '\t', 1, (int64_t)r.mapq);
		if (lane == 0) gdb_st(o, at, '\t');
		at += 1;
		if (!r.has_p) {
			if (lane == 0) gdb_st(o, at, '*');
			at += 1;
		} else if (r.in_tag) {
			at = gds_int(o, at, lane, 0, 0, r.ph_s);
			at = gds_int(o, at, lane, 'S', 1, r.ph_n);
			if (lane == 0) gdb_st(o, at, 'N');
			at += 1;
		} else
			at = gds_run(o, at, r, cig, 0, lane);
		at = gds_lit(o, at, lane, K_MATE, 0, 7);
	} else
		at = gds_lit(o, at, lane, K_UN0, K_UN1, 15);
	if (r.seq_star) at = gds_lit(o, at, lane, K_STARS, 0, 3);
	else {
		// SEQ: output base i is read base i, or the complement of read base l_seq - 1 - i on the reverse strand
		const uint8_t *sq = text + r.seq, *ql = text + r.qual;
		for (uint32_t i = lane; i < r.l_seq; i += 64) gdb_st(o, at + i, r.rev ? gds_comp(sq[r.l_seq - 1 - i]) : (uint32_t)sq[i]);
		at += r.l_seq;
		if (lane == 0) gdb_st(o, at, '\t');
		at += 1;
		if (r.has_qual) {
			for (uint32_t i = lane; i < r.l_seq; i += 64) gdb_st(o, at + i, ql[r.rev ? r.l_seq - 1 - i : i]);
			at += r.l_seq;
		} else {
			if (lane == 0) gdb_st(o, at, '*');
			at += 1;
		}
	}
	at = gdb_copy(o, at, lane, blob + r.blob[0], r.blob_len[0]);
	if (r.mapped) {
		if (r.has_p) {
			at = gds_tag_int(o, at, lane, 'N', 'M', r.nm);
			at = gds_tag_int(o, at, lane, 'm', 's', r.ms);
			at = gds_tag_int(o, at, lane, 'A', 'S', r.as);
			at = gds_tag_int(o, at, lane, 'n', 'n', (int64_t)r.nn);
		}
		at = gds_lit(o, at, lane, K_TP | (uint64_t)(r.tp & 255u) << 48, 0, 7);
		at = gds_tag_int(o, at, lane, 'c', 'm', r.cm);
		at = gds_tag_int(o, at, lane, 's', '1', r.s1);
		if (r.has_s2) at = gds_tag_int(o, at, lane, 's', '2', r.s2);
		if (r.has_p) {
			at = gds_lit(o, at, lane, K_DE, 0, 6);
			at = gds_lit(o, at, lane, r.de[0], r.de[1], r.de_len);
		}
	}
	at = gdb_copy(o, at, lane, blob + r.blob[1], r.blob_len[1]);
	if (r.in_tag) {
		at = gds_lit(o, at, lane, K_CG, 0, 7);
		at = gds_run(o, at, r, cig, 1, lane);
	}
	at = gds_lit(o, at, lane, K_RL, 0, 7);
	at = gdb_copy(o, at, lane, blob + r.blob[2], r.blob_len[2]);
	if (lane == 0) gdb_st(o, at, '\n');
	return at + 1;
}
