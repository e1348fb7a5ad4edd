// One BAM alignment record (SAM specification section 4.2) from one row of a flat record table: its size and its bytes, written once
// for the kernel (bam_encode.hip.h: one wavefront per record), for the host emulator that runs the same statements as loops over 64
// lanes (tests/emul/bam_emul.cpp) and for the driver, which sizes the records while it flattens them (bam_flatten.h).  No HIP in here.
//
// WHAT A RECORD IS.  A BAM record is defined as a fixed function of the SAM line gd_write_sam prints for the same alignment: the same
// clips, the same SEQ / QUAL slice and strand, the same tags in the same order.  The table row (GdbRec) holds the record's scalars and
// the places of everything variable:
//   * the read's name, SEQ and QUAL as ASCII in a text pool (SEQ is taken from the read's text, not from the nt4 batch, so IUPAC letters
//     keep their 4-bit codes);
//   * the alignment's CIGAR operations (already len << 4 | op) in a pool of 32-bit words; the clips are two scalars;
//   * three byte blobs the host has laid out ready to copy, because only the host holds their text: [0] RG:Z: (in front of the numeric
//     tags), [1] SA:Z: and the cs / MD string (behind de:f:), [2] the parsed tags of the read's comment (behind rl:i:0).
// HOW THE WORK IS SPLIT.  Everything per base and per operation is done by 64 lanes side by side, lane l taking the elements l, l + 64,
// ...: the name copy, the CIGAR with its clips (or the two placeholder operations), SEQ packed two bases to a byte with reversal and
// complement on the reverse strand, QUAL - 33 with reversal, the CG:B:I array and the blobs.  The fixed 36 bytes and the numeric tags
// (NM ms AS nn tp cm s1 s2 de rl) are per-record scalars: their places follow from wave-uniform arithmetic (gdb_int_width), and the
// lanes 0 .. size - 1 of a field each store one byte of it.  No lane reads what another lane wrote: the statements need no fence, and
// the order of the lanes cannot matter (the emulator runs them 0..63 and 63..0).
// SIZES are pure arithmetic on the row (gdb_block_size): the driver computes them and their prefix sum on the host while flattening, so
// one kernel writes every record at its final 64-bit offset and there is no counting pass.
// BOUNDS.  Records are not 4-byte aligned in the stream, so every store is a byte store, and every store is checked against the record's
// own end (GdbOut::end = 4 + block_size): a row whose fields disagree with its block_size can lose bytes, never write outside its
// record.  The offsets a row READS from are the host's (bam_flatten.h checks qs / qe against the read before it writes a row).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define GDB_HD __host__ __device__ __forceinline__
#else
#define GDB_HD static inline
#endif

enum { GDB_UNMAPPED_BIN = 4680, GDB_MAX_NAME = 254, GDB_MAX_OPS = 65535 };

struct GdbRec {
	uint64_t out;         // where the record (its block_size field) starts in the stream
	uint64_t name;        // text pool: l_name - 1 bytes (the NUL is written, not read)
	uint64_t seq, qual;   // text pool: the first base / quality of the slice printed, in read order
	uint64_t cig;         // CIGAR pool: n_cig words
	uint64_t blob[3];     // blob pool
	uint32_t blob_len[3];
	uint32_t block_size;  // bytes behind the block_size field
	int32_t refID, pos;
	uint32_t l_name;      // with the NUL
	uint32_t mapq, bin, flag;
	uint32_t n_op;        // n_cigar_op of the record: clips included; 2 when the CIGAR sits in the CG tag
	uint32_t l_seq;
	uint32_t rev;         // SEQ reversed and complemented, QUAL reversed
	uint32_t has_qual;    // 0: l_seq bytes of 0xff
	uint32_t n_cig, clip0, clip1, clip_op; // the alignment's operations; clip lengths (0: none) and their code (4 = S, 5 = H)
	uint32_t in_tag;      // more than 65 535 operations: the placeholder <l_seq>S<ref_len>N, and CG:B:I behind blob[1]
	uint32_t ref_len;     // reference length of the operations (the N of the placeholder)
	uint32_t mapped, has_p, has_s2; // numeric tags: tp cm s1 [s2] on every mapped record, NM ms AS nn and de with a CIGAR
	uint32_t tp;          // 'P' or 'S'
	int32_t nm, ms, as, cm, s1, s2;
	uint32_t nn;
	float de;
};

// reg2bin of the SAM specification (section 5.3)
GDB_HD uint32_t gdb_reg2bin(int64_t beg, int64_t end)
{
	--end;
	if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
	if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
	if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
	if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
	if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
	return 0;
}

// an integer tag: the smallest type that holds the value, signed types for negative values only
GDB_HD uint32_t gdb_int_width(int64_t v)
{
	if (v < 0) return v >= -128 ? 1u : v >= -32768 ? 2u : 4u;
	return v <= 255 ? 1u : v <= 65535 ? 2u : 4u;
}
GDB_HD uint32_t gdb_int_type(int64_t v)
{
	if (v < 0) return v >= -128 ? 'c' : v >= -32768 ? 's' : 'i';
	return v <= 255 ? 'C' : v <= 65535 ? 'S' : 'I';
}

// the 4-bit code of a base: the index of the upper-cased letter in "=ACMGRSVTWYHKDBN", 15 for anything else.  comp: of its complement
// (seq_comp_table of the reference restricted to letters, as gd_write_sam's put_seq applies it).  Two tables of 26 nibbles, built here
// from the two strings and held in four 64-bit constants: no memory is read.
struct GdbCodes { uint64_t fwd[2], rev[2]; };
constexpr GdbCodes gdb_make_codes()
{
	const char codes[] = "=ACMGRSVTWYHKDBN", comp[] = "TVGHEFCDIJMLKNOPQYSAABWXRZ";
	GdbCodes t = {{0, 0}, {0, 0}};
	for (int l = 0; l < 26; ++l) {
		uint64_t f = 15, r = 15;
		for (int k = 1; k < 16; ++k) {
			if (codes[k] == 'A' + l) f = (uint64_t)k;
			if (codes[k] == comp[l]) r = (uint64_t)k;
		}
		t.fwd[l >> 4] |= f << (4 * (l & 15)), t.rev[l >> 4] |= r << (4 * (l & 15));
	}
	return t;
}
GDB_HD uint32_t gdb_base_code(uint32_t c, uint32_t comp)
{
	constexpr GdbCodes T = gdb_make_codes();
	if (c == '=') return 0;
	const uint32_t l = (c | 32u) - 'a';
	if (l >= 26u || c < 'A') return 15;
	const uint64_t lo = comp ? T.rev[0] : T.fwd[0], hi = comp ? T.rev[1] : T.fwd[1];
	return (uint32_t)((l < 16u ? lo >> (4u * l) : hi >> (4u * (l - 16u))) & 15u);
}

// bytes of the numeric tags in front of blob[1] (NM ms AS nn | tp cm s1 [s2] | de) and of the CG tag
GDB_HD uint32_t gdb_num_tags_size(const GdbRec &r)
{
	if (!r.mapped) return 0;
	uint32_t n = 4 + (3 + gdb_int_width(r.cm)) + (3 + gdb_int_width(r.s1));
	if (r.has_s2) n += 3 + gdb_int_width(r.s2);
	if (r.has_p) n += (3 + gdb_int_width(r.nm)) + (3 + gdb_int_width(r.ms)) + (3 + gdb_int_width(r.as)) + (3 + gdb_int_width((int64_t)r.nn)) + 7;
	return n;
}
GDB_HD uint32_t gdb_cg_ops(const GdbRec &r) { return r.n_cig + (r.clip0 ? 1u : 0u) + (r.clip1 ? 1u : 0u); }
GDB_HD uint64_t gdb_block_size(const GdbRec &r)
{
	uint64_t n = 32 + (uint64_t)r.l_name + 4ull * r.n_op + (r.l_seq + 1ull) / 2 + r.l_seq;
	n += (uint64_t)r.blob_len[0] + gdb_num_tags_size(r) + r.blob_len[1];
	if (r.in_tag) n += 8 + 4ull * gdb_cg_ops(r);
	return n + 4 /* rl:i:0 as rl C 0 */ + r.blob_len[2];
}

// the record's bytes in the stream: p[0, end)
struct GdbOut { uint8_t *p; uint64_t end; };
GDB_HD void gdb_st(const GdbOut &o, uint64_t at, uint32_t v) { if (at < o.end) o.p[at] = (uint8_t)v; }
GDB_HD void gdb_st32(const GdbOut &o, uint64_t at, uint32_t v) { gdb_st(o, at, v), gdb_st(o, at + 1, v >> 8), gdb_st(o, at + 2, v >> 16), gdb_st(o, at + 3, v >> 24); }
// a field of n <= 64 bytes whose byte k is (k < 3 ? the tag's name and type : byte k - 3 of v): lane k stores byte k
GDB_HD uint64_t gdb_tag(const GdbOut &o, uint64_t at, uint32_t lane, char a, char b, uint32_t type, uint32_t v, uint32_t width)
{
	if (lane < 3 + width) gdb_st(o, at + lane, lane == 0 ? (uint32_t)a : lane == 1 ? (uint32_t)b : lane == 2 ? type : v >> (8 * (lane - 3)));
	return at + 3 + width;
}
GDB_HD uint64_t gdb_tag_int(const GdbOut &o, uint64_t at, uint32_t lane, char a, char b, int64_t v) { return gdb_tag(o, at, lane, a, b, gdb_int_type(v), (uint32_t)v, gdb_int_width(v)); }
GDB_HD uint64_t gdb_copy(const GdbOut &o, uint64_t at, uint32_t lane, const uint8_t *src, uint64_t n)
{
	for (uint64_t k = lane; k < n; k += 64) gdb_st(o, at + k, src[k]);
	return at + n;
}
// operation k of the CIGAR with its clips: [clip0] ops [clip1]
GDB_HD uint32_t gdb_clipped_op(const GdbRec &r, const uint32_t *cig, uint32_t k)
{
	const uint32_t lead = r.clip0 ? 1u : 0u;
	if (k < lead) return r.clip0 << 4 | r.clip_op;
	if (k - lead < r.n_cig) return cig[r.cig + (k - lead)];
	return r.clip1 << 4 | r.clip_op;
}

// Lane `lane` of the wavefront that writes record r at stream + r.out.  Returns the number of bytes the record takes (4 + block_size as
// the fields give it; the caller may compare it with r.block_size).
GDB_HD uint64_t gdb_encode(const GdbRec &r, const uint8_t *text, const uint32_t *cig, const uint8_t *blob, uint8_t *stream, uint32_t lane)
{
	GdbOut o;
	o.p = stream + r.out, o.end = 4ull + r.block_size;
	// the fixed 36 bytes: lane k stores byte k of nine words
	if (lane < 36) {
		const uint32_t w = lane >> 2;
		const uint32_t v = w == 0 ? r.block_size : w == 1 ? (uint32_t)r.refID : w == 2 ? (uint32_t)r.pos : w == 3 ? (r.bin << 16 | (r.mapq & 255u) << 8 | (r.l_name & 255u))
		                 : w == 4 ? (r.flag << 16 | (r.n_op & 0xffffu)) : w == 5 ? r.l_seq : w == 8 ? 0u : 0xffffffffu; // next_refID = next_pos = -1, tlen = 0
		gdb_st(o, lane, v >> (8 * (lane & 3)));
	}
	uint64_t at = 36;
	at = gdb_copy(o, at, lane, text + r.name, r.l_name - 1);
	if (lane == 0) gdb_st(o, at, 0);
	at += 1;
	if (r.in_tag) { // the placeholder BAM can hold: <l_seq>S<ref_len>N
		if (lane < 2) gdb_st32(o, at + 4 * lane, lane == 0 ? (r.l_seq << 4 | 4u) : (r.ref_len << 4 | 3u));
	} else
		for (uint32_t k = lane; k < r.n_op; k += 64) gdb_st32(o, at + 4ull * k, gdb_clipped_op(r, cig, k));
	at += 4ull * r.n_op;
	// SEQ: output base i is read base i, or the complement of read base l_seq - 1 - i on the reverse strand; two to a byte
	const uint8_t *sq = text + r.seq;
	for (uint32_t j = lane; j < (r.l_seq + 1) / 2; j += 64) {
		const uint32_t i0 = 2 * j, i1 = 2 * j + 1;
		const uint32_t c0 = gdb_base_code(sq[r.rev ? r.l_seq - 1 - i0 : i0], r.rev);
		const uint32_t c1 = i1 < r.l_seq ? gdb_base_code(sq[r.rev ? r.l_seq - 1 - i1 : i1], r.rev) : 0u;
		gdb_st(o, at + j, c0 << 4 | c1);
	}
	at += (r.l_seq + 1ull) / 2;
	const uint8_t *ql = text + r.qual;
	for (uint32_t i = lane; i < r.l_seq; i += 64) gdb_st(o, at + i, r.has_qual ? (uint32_t)ql[r.rev ? r.l_seq - 1 - i : i] - 33u : 0xffu);
	at += r.l_seq;
	at = gdb_copy(o, at, lane, blob + r.blob[0], r.blob_len[0]);
	if (r.mapped) {
		if (r.has_p) {
			at = gdb_tag_int(o, at, lane, 'N', 'M', r.nm);
			at = gdb_tag_int(o, at, lane, 'm', 's', r.ms);
			at = gdb_tag_int(o, at, lane, 'A', 'S', r.as);
			at = gdb_tag_int(o, at, lane, 'n', 'n', (int64_t)r.nn);
		}
		at = gdb_tag(o, at, lane, 't', 'p', 'A', r.tp, 1);
		at = gdb_tag_int(o, at, lane, 'c', 'm', r.cm);
		at = gdb_tag_int(o, at, lane, 's', '1', r.s1);
		if (r.has_s2) at = gdb_tag_int(o, at, lane, 's', '2', r.s2);
		if (r.has_p) {
			uint32_t bits;
			memcpy(&bits, &r.de, 4);
			at = gdb_tag(o, at, lane, 'd', 'e', 'f', bits, 4);
		}
	}
	at = gdb_copy(o, at, lane, blob + r.blob[1], r.blob_len[1]);
	if (r.in_tag) { // CG:B:I,<count>,<operations with their clips>
		const uint32_t n = gdb_cg_ops(r);
		if (lane < 8) gdb_st(o, at + lane, lane < 4 ? (uint32_t)"CGBI"[lane] : n >> (8 * (lane - 4)));
		at += 8;
		for (uint32_t k = lane; k < n; k += 64) gdb_st32(o, at + 4ull * k, gdb_clipped_op(r, cig, k));
		at += 4ull * n;
	}
	at = gdb_tag(o, at, lane, 'r', 'l', 'C', 0, 1);
	at = gdb_copy(o, at, lane, blob + r.blob[2], r.blob_len[2]);
	return at;
}
