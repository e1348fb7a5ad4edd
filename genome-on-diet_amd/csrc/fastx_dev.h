// The strict four-line FASTQ prefix of a block of the input, as the device finds it: the per-lane and per-record statements, written
// once for the kernels (fastx_dev.hip.h), for the host emulator that runs them as loops (tests/emul/fastx_dev_emul.cpp) and for the
// reader (fastx_reader.h), which turns the record table into its chunk.  No HIP in here.
//
// WHY A STRICT RECORD IS WHAT kseq_read RETURNS (LR/kseq.h:191-232).  Byte 0 of a block is a place where the sequential parser stands
// with last_char == 0: a block begins where the parse of the previous one ended, and after a FASTQ record kseq_read leaves last_char = 0.
// Let lines 4r .. 4r+3 be complete (each ends with '\n' inside the block), and let every record before r be strict, so that, by
// induction, the parser stands on the first byte of line 4r.  Then, for a strict record:
//   * kseq.h:195-199: the scan for '>' or '@' ends on the first byte it reads, because line 0 starts with '@'.
//   * :201: ks_getuntil(KS_SEP_SPACE) takes the name up to the first byte that isspace() accepts in the C locale -- ' ' or '\t'..'\r';
//     the '\n' of the line is such a byte, so the name never leaves line 0.  :202: if that byte was not '\n', the rest of the line is the
//     comment (ks_getuntil2 with KS_SEP_LINE); read_record of fastx_reader.h keeps it only when it is not empty.  No '\r' is in the line,
//     so nothing is trimmed from its end (kseq.h:141).
//   * :207-212: the sequence loop reads the first byte of the next line and stops on '>', '+' or '@'; an empty line is skipped.  Line 1
//     is not empty and starts with none of the three, so all of it is appended; the byte read next is the first of line 2, a '+': the
//     loop ends with exactly line 1 as the sequence, whatever else line 1 holds.
//   * :219: the rest of the '+' line is skipped up to its '\n'.
//   * :221: quality lines are appended while the quality string is shorter than the sequence.  Nothing has been appended when line 3
//     is read, and len(line 3) == len(line 1) >= 1, so line 3 is read whole -- its first byte is never looked at, a '@' or '+' there
//     means nothing -- and the loop ends after it.  :223-224: last_char = 0, the lengths agree, the record is returned.
// The parser has consumed exactly the four lines and stands, with last_char == 0, on the first byte of line 4(r+1): the induction
// step.  A record that is not strict is not claimed to be wrong: it, and everything behind it in the block, is left to that parser.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GDX_HD __host__ __device__ __forceinline__
#else
#define GDX_HD static inline
#endif

enum { GDX_TILE = 1024, GDX_LANE_BYTES = 16 }; // one wavefront: 64 lanes x one 16-byte load
static const uint32_t GDX_NONE = 0xffffffffu;

struct GdxRec { // one strict record; offsets into the block, lengths without the line ends
	uint32_t name_off, name_len;
	uint32_t comment_off, comment_len; // comment_off == GDX_NONE: no comment
	uint32_t seq_off, seq_len;
	uint32_t qual_off;                 // (its length is seq_len)
};

// bit j = (byte j of the lane's 16 bytes == c), for the j < valid bytes that lie inside the block: bytes past its end match nothing
GDX_HD uint32_t gdx_eq_mask16(const uint32_t w[4], uint32_t c, uint32_t valid)
{
	uint32_t m = 0;
	for (int k = 0; k < 4; ++k) {
		const uint32_t x = w[k] ^ (c * 0x01010101u);                                      // a zero byte where the byte is c
		const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu) >> 7; // bit 8j set iff byte j of x is zero (exact: no carry leaves a byte)
		m |= ((z | z >> 7 | z >> 14 | z >> 21) & 0xfu) << (4 * k);
	}
	return valid >= GDX_LANE_BYTES ? m : m & ((1u << valid) - 1u);
}
// bytes of the lane that starts at block offset `at` which lie inside a block of n bytes
GDX_HD uint32_t gdx_valid16(uint32_t at, uint32_t n) { return at >= n ? 0u : (n - at < GDX_LANE_BYTES ? n - at : (uint32_t)GDX_LANE_BYTES); }

// isspace() of the C locale, the delimiter of KS_SEP_SPACE (LR/kseq.h:113)
GDX_HD bool gdx_space(uint32_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

// Record r of a block b whose newline offsets are nl[0 .. 4r + 3]: fills R and returns whether the record is strict.  first_cr is the
// offset of the first '\r' of the block (anything >= the block's length if it has none): the record that holds it is not strict, and
// since only the FIRST record that is not strict matters (everything from it on is the host's), no later '\r' needs to be known.
GDX_HD bool gdx_record(const uint8_t *b, const uint32_t *nl, uint32_t r, uint32_t first_cr, GdxRec &R)
{
	const uint32_t s0 = r ? nl[4 * r - 1] + 1 : 0, e0 = nl[4 * r], e1 = nl[4 * r + 1], e2 = nl[4 * r + 2], e3 = nl[4 * r + 3];
	const uint32_t s1 = e0 + 1, s2 = e1 + 1, s3 = e2 + 1;
	R.name_off = s0 + 1, R.name_len = 0, R.comment_off = GDX_NONE, R.comment_len = 0;
	R.seq_off = s1, R.seq_len = e1 - s1, R.qual_off = s3;
	if (b[s0] != '@') return false; // (an empty line 0 has its '\n' here)
	uint32_t p = s0 + 1;
	while (p < e0 && !gdx_space(b[p])) ++p;
	R.name_len = p - (s0 + 1);
	if (p + 1 < e0) R.comment_off = p + 1, R.comment_len = e0 - (p + 1); // a delimiter other than the line's '\n', and a rest that is not empty
	const uint32_t c1 = b[s1];
	return b[s2] == '+' && e1 > s1 && e1 - s1 == e3 - s3 && c1 != '@' && c1 != '+' && c1 != '>' && first_cr > e3;
}

// seq_nt4_table (LR/sketch.c:11-18) without a table in memory: A/a 0, C/c 1, G/g 2, T/t/U/u 3, the raw codes 0-3 themselves, else 4
GDX_HD uint32_t gdx_nt4(uint32_t c)
{
	if (c < 4) return c;
	const uint32_t u = c & 0xdfu; // (a byte maps to 'A' here iff it is 'A' or 'a', and so on)
	return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : (u == 'T' || u == 'U') ? 3u : 4u;
}
// the host strings turn U / u into T / t (kseq2bseq, LR/bseq.c:71-73)
GDX_HD bool gdx_is_u(uint32_t c) { return (c & 0xdfu) == 'U'; }
