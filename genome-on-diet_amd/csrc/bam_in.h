// BAM input (SAM specification section 4.2), the reverse of bam_record.h: alignment records -> the reads the FASTQ reader would have
// returned for the FASTQ equivalent of the file (include/gdiet_hip.h, "BAM input", is the definition).  Three pieces, no HIP in here:
//   gdi_header / gdi_walk   the grammar.  Record starts follow from each other through block_size, so the walk is sequential -- and cheap:
//                           one look at the fixed 36 bytes of every record.  It yields one table row per kept record (GdiRow: where SEQ
//                           and QUAL stand in the block, l_seq, strand, and where the record's text goes: a prefix sum) and one host row
//                           (GdiHostRow: name and aux fields, which only the host turns into text).
//   gdi_unpack              the per-record statements, written once for the kernel (bam_in.hip.h: one wavefront per record), for the host
//                           emulator that runs them as loops over 64 lanes (tests/emul/bam_in_emul.cpp) and for the reader's host threads
//                           (fastx_reader.h), which run lane 0 with a stride of 1.
//   gdi_aux_scan / _text    aux fields checked against their record, and printed as SAM text (the comment of the read).
// HOW THE WORK IS SPLIT.  Lane l writes the text bytes l, l + 64, ...: base i of the output is nibble i of SEQ through a 16-letter table held
// in two 64-bit constants, or, on the reverse strand, the complement of nibble l_seq - 1 - i (the nibble's parity flips with l_seq's);
// quality i is QUAL[i] + 33, reversed likewise.  Lane 0 writes the two NULs.  No lane reads what another lane wrote: no fence, and the
// order of the lanes cannot matter.
// THE COMPLEMENT is the one the writer applies (gdb_base_code(., 1)): gdi_make_comp() derives the 16 nibbles from the writer's own table, and
// the static_assert below proves that they are the 4-bit reversal of the code (A=1 <-> T=8, C=2 <-> G=4, M=3 <-> K=12, ...; '=' and N
// stay), so this project's BAM output read back gives the reads that went in.
// BOUNDS.  Every store is checked against the record's own text range [dst, dst_end): a table that disagrees with itself can lose bytes,
// never write outside its record.  The ranges a row READS are checked by gdi_rows_inside before a table is used.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "bam_record.h"

#define GDI_HD GDB_HD

enum { GDI_REV = 1, GDI_NOQUAL = 2 };
struct GdiRow {
	uint32_t seq_off, qual_off; // in the block: (l_seq + 1) / 2 bytes of nibbles, l_seq bytes of qualities
	uint32_t l_seq, flags;
	uint64_t dst, dst_end;      // the record's text: seq NUL [qual NUL]
};
struct GdiHostRow {
	uint32_t name_off, l_name;  // in the block, with the NUL
	uint32_t aux_off, aux_len;  // in the block
	uint64_t name_dst;          // prefix sum of l_name
};

// the letters of the 16 codes, eight to a word
constexpr uint64_t gdi_letters(int half)
{
	const char codes[] = "=ACMGRSVTWYHKDBN";
	uint64_t w = 0;
	for (int k = 0; k < 8; ++k) w |= (uint64_t)(unsigned char)codes[8 * half + k] << (8 * k);
	return w;
}
// nibble k = the code of the complement of code k, from the writer's table (bam_record.h)
constexpr uint64_t gdi_make_comp()
{
	const char codes[] = "=ACMGRSVTWYHKDBN";
	const GdbCodes T = gdb_make_codes();
	uint64_t w = 0; // ('=' stays '=': gdb_base_code returns 0 for it on either strand)
	for (int k = 1; k < 16; ++k) {
		const int l = codes[k] - 'A';
		w |= ((T.rev[l >> 4] >> (4 * (l & 15))) & 15) << (4 * k);
	}
	return w;
}
constexpr uint64_t gdi_bit_reversal()
{
	uint64_t w = 0;
	for (uint64_t k = 0; k < 16; ++k) w |= ((k & 1) << 3 | (k & 2) << 1 | (k & 4) >> 1 | (k & 8) >> 3) << (4 * k);
	return w;
}
static_assert(gdi_make_comp() == gdi_bit_reversal(), "the writer's complement table is not the 4-bit reversal of the code");

GDI_HD uint32_t gdi_letter(uint32_t code)
{
	constexpr uint64_t lo = gdi_letters(0), hi = gdi_letters(1);
	return (uint32_t)((code < 8u ? lo >> (8u * code) : hi >> (8u * (code - 8u))) & 255u);
}
GDI_HD uint32_t gdi_comp(uint32_t code)
{
	constexpr uint64_t T = gdi_make_comp();
	return (uint32_t)(T >> (4u * code)) & 15u;
}
GDI_HD void gdi_st(uint8_t *text, uint64_t at, uint64_t end, uint32_t v) { if (at < end) text[at] = (uint8_t)v; }

// Lane `lane` of `stride` lanes (64 for a wavefront; the reader's host threads run lane 0 of 1) that write the text of row r.
GDI_HD void gdi_unpack(const GdiRow &r, const uint8_t *blk, uint8_t *text, uint32_t lane, uint32_t stride)
{
	const uint32_t n = r.l_seq, rev = r.flags & GDI_REV;
	const uint64_t end = r.dst_end;
	const uint8_t *sq = blk + r.seq_off;
	for (uint32_t k = lane; k < n; k += stride) {
		const uint32_t i = rev ? n - 1u - k : k;
		const uint32_t b = sq[i >> 1];
		const uint32_t c = (i & 1u) ? (b & 15u) : (b >> 4);
		gdi_st(text, r.dst + k, end, gdi_letter(rev ? gdi_comp(c) : c));
	}
	if (lane == 0) gdi_st(text, r.dst + n, end, 0);
	if (r.flags & GDI_NOQUAL) return;
	const uint8_t *ql = blk + r.qual_off;
	const uint64_t q0 = r.dst + n + 1ull;
	for (uint32_t k = lane; k < n; k += stride) gdi_st(text, q0 + k, end, ((uint32_t)ql[rev ? n - 1u - k : k] + 33u) & 255u);
	if (lane == 0) gdi_st(text, q0 + n, end, 0);
}

// every range the rows read lies inside a block of n bytes, and every text range inside [0, text_len)
static inline bool gdi_rows_inside(const GdiRow *rows, size_t n_rows, uint64_t n, uint64_t text_len)
{
	for (size_t k = 0; k < n_rows; ++k) {
		const GdiRow &r = rows[k];
		if ((uint64_t)r.seq_off + (r.l_seq + 1ull) / 2 > n) return false;
		if (!(r.flags & GDI_NOQUAL) && (uint64_t)r.qual_off + r.l_seq > n) return false;
		if (r.dst > r.dst_end || r.dst_end > text_len) return false;
	}
	return true;
}

static inline uint32_t gdi_le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
static inline uint32_t gdi_le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// The header of b[0, n): magic, l_text, text, n_ref, and l_name, name, l_ref per reference.  0: it ends at *end; 1: it runs past n;
// -1: it cannot be a header (why).
static inline int gdi_header(const uint8_t *b, uint64_t n, uint64_t *end, std::string &why)
{
	if (n < 12) return 1;
	const int32_t l_text = (int32_t)gdi_le32(b + 4);
	if (l_text < 0) { why = "BAM header: a negative l_text"; return -1; }
	uint64_t p = 8ull + (uint64_t)l_text;
	if (p + 4 > n) return 1;
	const int32_t n_ref = (int32_t)gdi_le32(b + p);
	if (n_ref < 0) { why = "BAM header: a negative n_ref"; return -1; }
	p += 4;
	for (int32_t k = 0; k < n_ref; ++k) {
		if (p + 4 > n) return 1;
		const int32_t l_name = (int32_t)gdi_le32(b + p);
		if (l_name < 0) { why = "BAM header: reference " + std::to_string(k) + ": a negative l_name"; return -1; }
		p += 8ull + (uint64_t)l_name;
		if (p > n) return 1;
	}
	*end = p;
	return 0;
}

static inline uint32_t gdi_aux_size(uint32_t t) { return t == 'A' || t == 'c' || t == 'C' ? 1u : t == 's' || t == 'S' ? 2u : t == 'i' || t == 'I' || t == 'f' ? 4u : 0u; }
// the aux fields a[0, n) are whole fields of known types
static inline bool gdi_aux_scan(const uint8_t *a, uint64_t n)
{
	uint64_t p = 0;
	while (p < n) {
		if (n - p < 4) return false; // tag, type and one byte of value at least
		const uint32_t t = a[p + 2];
		p += 3;
		if (const uint32_t w = gdi_aux_size(t)) {
			if (n - p < w) return false;
			p += w;
		} else if (t == 'Z' || t == 'H') {
			const void *z = memchr(a + p, 0, (size_t)(n - p));
			if (!z) return false;
			p = (uint64_t)((const uint8_t *)z - a) + 1;
		} else if (t == 'B') {
			if (n - p < 5) return false;
			const uint32_t w = gdi_aux_size(a[p]);
			const int32_t cnt = (int32_t)gdi_le32(a + p + 1);
			if (!w || a[p] == 'A' || cnt < 0) return false;
			p += 5;
			if ((n - p) / w < (uint64_t)cnt) return false;
			p += (uint64_t)w * (uint64_t)cnt;
		} else return false;
	}
	return true;
}

// the shortest decimal text, without an exponent, whose float32 is the value
static inline void gdi_f32_text(uint32_t bits, std::string &out)
{
	float v;
	memcpy(&v, &bits, 4);
	if (v != v) { out += "nan"; return; }
	if (v - v != 0) { out += v < 0 ? "-inf" : "inf"; return; }
	char buf[40];
	for (int p = 0; p < 9; ++p) {
		snprintf(buf, sizeof(buf), "%.*e", p, (double)v);
		if (strtof(buf, nullptr) == v) break;
	}
	const char *s = buf;
	if (*s == '-') out.push_back('-'), ++s;
	std::string d;
	for (; *s && *s != 'e'; ++s) if (*s != '.') d.push_back(*s);
	const long point = (*s == 'e' ? strtol(s + 1, nullptr, 10) : 0) + 1; // digits in front of the decimal point
	while (d.size() > 1 && d.back() == '0') d.pop_back();
	const long nd = (long)d.size();
	if (point <= 0) out += "0.", out.append((size_t)-point, '0'), out += d;
	else if (point >= nd) out += d, out.append((size_t)(point - nd), '0');
	else out.append(d, 0, (size_t)point), out.push_back('.'), out.append(d, (size_t)point, std::string::npos);
}
static inline void gdi_aux_value(uint32_t t, const uint8_t *p, std::string &out)
{
	char buf[24];
	long long v = 0;
	switch (t) {
	case 'c': v = (int8_t)p[0]; break;
	case 'C': v = p[0]; break;
	case 's': v = (int16_t)gdi_le16(p); break;
	case 'S': v = gdi_le16(p); break;
	case 'i': v = (int32_t)gdi_le32(p); break;
	case 'I': v = gdi_le32(p); break;
	default: gdi_f32_text(gdi_le32(p), out); return;
	}
	snprintf(buf, sizeof(buf), "%lld", v);
	out += buf;
}
// aux fields that passed gdi_aux_scan, as SAM text joined by tabs: integers print as i, floats as gdi_f32_text, A Z H verbatim, B as
// subtype and comma-separated values
static inline void gdi_aux_text(const uint8_t *a, uint64_t n, std::string &out)
{
	uint64_t p = 0;
	bool first = true;
	while (p + 4 <= n) {
		if (!first) out.push_back('\t');
		first = false;
		const uint32_t t = a[p + 2];
		out.push_back((char)a[p]), out.push_back((char)a[p + 1]), out.push_back(':');
		p += 3;
		if (t == 'A') out += "A:", out.push_back((char)a[p]), p += 1;
		else if (t == 'Z' || t == 'H') {
			out.push_back((char)t), out.push_back(':');
			const size_t l = strlen((const char *)a + p);
			out.append((const char *)a + p, l);
			p += l + 1;
		} else if (t == 'B') {
			const uint32_t sub = a[p], w = gdi_aux_size(sub), cnt = gdi_le32(a + p + 1);
			out += "B:", out.push_back((char)sub);
			p += 5;
			for (uint32_t k = 0; k < cnt; ++k, p += w) out.push_back(','), gdi_aux_value(sub, a + p, out);
		} else {
			out += t == 'f' ? "f:" : "i:";
			gdi_aux_value(t, a + p, out);
			p += gdi_aux_size(t);
		}
	}
}

// The records of b[from, fill), a stretch of the decompressed stream whose byte 0 stands at stream offset `base`; `ordinal` is the
// number of records in front of it (skipped ones count).  Walks whole records only: pos is where the first record starts that the
// stretch does not hold completely (the block's tail), or fill.  A malformed record ends the walk with bad = true and its message; the
// rows in front of it stand.  Records with FLAG 0x100 or 0x800 are checked like the others and give no row.  starts != NULL takes the
// start offset (in b) of every record the walk passed, those without a row included (the sort pass of bam_sort_driver.hip.h).
struct GdiWalk {
	std::vector<GdiRow> rows;
	std::vector<GdiHostRow> host;
	uint64_t text_len = 0, names_len = 0, n_seen = 0;
	size_t pos = 0;
	bool bad = false;
	std::string msg;
};
static inline void gdi_walk(const uint8_t *b, size_t from, size_t fill, bool with_qual, bool want_aux, uint64_t ordinal, uint64_t base, GdiWalk &W,
                            std::vector<uint64_t> *starts = nullptr)
{
	size_t pos = from;
	auto fail = [&](const std::string &what) {
		W.bad = true, W.msg = "BAM record " + std::to_string(ordinal + W.n_seen) + " at offset " + std::to_string(base + pos) + ": " + what;
	};
	for (;;) {
		const uint64_t rem = fill - pos;
		if (rem < 4) break;
		const int32_t bs_ = (int32_t)gdi_le32(b + pos);
		if (bs_ < 32) { fail("a block_size of " + std::to_string(bs_) + ", below the 32 fixed bytes"); break; }
		const uint64_t bs = (uint64_t)bs_;
		if (rem - 4 < bs) break;
		const uint8_t *r = b + pos + 4;
		const uint32_t l_name = r[8], n_op = gdi_le16(r + 12), flag = gdi_le16(r + 14);
		const int32_t l_seq = (int32_t)gdi_le32(r + 16);
		if (l_seq < 0) { fail("a negative l_seq"); break; }
		if (l_name == 0) { fail("l_read_name is 0"); break; }
		const uint64_t need = 32ull + l_name + 4ull * n_op + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq;
		if (need > bs) { fail("its fields take " + std::to_string(need) + " bytes, block_size is " + std::to_string(bs)); break; }
		if (r[32 + l_name - 1] != 0) { fail("a name without its NUL"); break; }
		if (want_aux && !gdi_aux_scan(r + need, bs - need)) { fail("an aux field runs past the record or has an unknown type"); break; }
		++W.n_seen;
		if (starts) starts->push_back(pos);
		const size_t at = pos + 4;
		pos += 4 + (size_t)bs;
		if (flag & 0x900u) continue; // secondary, supplementary
		GdiRow R;
		R.seq_off = (uint32_t)(at + 32 + l_name + 4 * (size_t)n_op), R.qual_off = R.seq_off + ((uint32_t)l_seq + 1) / 2;
		R.l_seq = (uint32_t)l_seq, R.flags = (flag & 0x10u) ? GDI_REV : 0;
		if (!with_qual || l_seq == 0 || b[R.qual_off] == 0xff) R.flags |= GDI_NOQUAL;
		R.dst = W.text_len, R.dst_end = R.dst + ((uint64_t)l_seq + 1) * ((R.flags & GDI_NOQUAL) ? 1 : 2);
		W.text_len = R.dst_end;
		GdiHostRow H;
		H.name_off = (uint32_t)(at + 32), H.l_name = l_name, H.aux_off = (uint32_t)(at + need), H.aux_len = (uint32_t)(bs - need);
		H.name_dst = W.names_len;
		W.names_len += l_name;
		W.rows.push_back(R), W.host.push_back(H);
	}
	W.pos = pos;
}
