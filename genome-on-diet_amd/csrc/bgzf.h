// BGZF (the blocked gzip htslib's bgzip writes; SAM/BAM specification, section 4.1) as the reader sees it: the member table of a byte
// range, found without inflating anything, the end-of-file marker, and the per-member check every route ends with.  Plain C++ + zlib;
// no HIP in here (the device's decoder is bgzf_inflate.h / bgzf_inflate.hip.h).
//
// A BGZF file is a series of gzip members, each at most 64 KiB on either side:
//   1f 8b 08 FLG(=04) MTIME(4) XFL OS XLEN(2) | extra subfields, one of them 'B' 'C' 02 00 BSIZE(2) | deflate stream | CRC32(4) ISIZE(4)
// BSIZE + 1 is the size of the whole member and ISIZE that of its output, so the boundaries of the members and the place of every
// member's output are known before a byte is inflated: members are independent deflate streams and can be inflated side by side.
// To the reference, which reads through zlib's gzread, such a file is ordinary multi-member gzip; the bytes are the same.
//
// WHAT IS ACCEPTED AS A MEMBER: the magic 1f 8b 08; FLG with FEXTRA (4) and without FHCRC / FNAME / FCOMMENT (they would move the start
// of the deflate stream; bgzip never sets them); a 'B' 'C' subfield with SLEN == 2, wherever it stands among the extra subfields;
// BSIZE + 1 large enough for header and trailer; ISIZE <= 65536.  Anything else is "not BGZF".
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include <zlib.h>

struct GdBgzfMember {
	uint64_t in_off;  // the deflate stream inside the range
	uint64_t out_off; // prefix sum of ISIZE over the members before this one
	uint32_t in_len;
	uint32_t isize, crc; // the trailer's claims
};

enum { GD_BGZF_MAX_ISIZE = 65536, GD_BGZF_EOF_LEN = 28 };
static const unsigned char GD_BGZF_EOF[GD_BGZF_EOF_LEN] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

static inline uint32_t gd_bgzf_le16(const unsigned char *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
static inline uint32_t gd_bgzf_le32(const unsigned char *p) { return gd_bgzf_le16(p) | gd_bgzf_le16(p + 2) << 16; }

enum { GD_BGZF_OK = 0, GD_BGZF_NOT_BGZF = -1 };

// Walks the members of p[0, n).  tab gets one entry per complete member, in order; *incomplete_from is the offset of a member the end of
// the range cuts off (in its header, its payload or its trailer), n when the range ends on a member boundary: the caller carries
// p[*incomplete_from, n) over to its next read.  Returns GD_BGZF_NOT_BGZF, with the offset in *bad_at and the reason in *why, at the
// first thing that is not a member; tab then holds the members in front of it.  No byte at or behind p + n is read.  max_out > 0 stops
// in front of the first member that would take the sum of ISIZE past max_out, unless it is the first: *incomplete_from is its offset,
// and *full says that this, not the end of the range, is what ended the walk.
static inline int gd_bgzf_scan(const unsigned char *p, size_t n, std::vector<GdBgzfMember> &tab, size_t *incomplete_from, size_t *bad_at, std::string *why,
                               uint64_t max_out = 0, bool *full = nullptr)
{
	tab.clear();
	if (full) *full = false;
	size_t at = 0;
	uint64_t out = 0;
	auto bad = [&](const char *what) {
		if (bad_at) *bad_at = at;
		if (why) *why = what;
		if (incomplete_from) *incomplete_from = at;
		return (int)GD_BGZF_NOT_BGZF;
	};
	while (at < n) {
		const unsigned char *h = p + at;
		const size_t left = n - at;
		static const unsigned char magic[3] = {0x1f, 0x8b, 0x08};
		if (memcmp(h, magic, left < 3 ? left : 3)) return bad("no gzip magic");
		if (left >= 4 && (!(h[3] & 4) || (h[3] & 0x1a))) return bad("a gzip member without the BGZF extra field");
		if (left < 12) break; // cut off inside the fixed header
		const size_t xlen = gd_bgzf_le16(h + 10);
		if (left < 12 + xlen) { // cut off inside the extra field: it may still prove itself no member
			if (xlen < 6) return bad("extra field too short for a BC subfield");
			break;
		}
		size_t x = 0, bsize = 0;
		bool found = false;
		while (x + 4 <= xlen) {
			const unsigned char *s = h + 12 + x;
			const size_t slen = gd_bgzf_le16(s + 2);
			if (x + 4 + slen > xlen) break;
			if (s[0] == 'B' && s[1] == 'C' && slen == 2) { bsize = gd_bgzf_le16(s + 4), found = true; break; }
			x += 4 + slen;
		}
		if (!found) return bad("no BC subfield in the extra field");
		const size_t total = bsize + 1;
		if (total < 12 + xlen + 8) return bad("BSIZE smaller than header and trailer");
		if (total > left) break; // cut off inside the payload or the trailer
		GdBgzfMember m;
		m.in_off = at + 12 + xlen, m.in_len = (uint32_t)(total - 12 - xlen - 8);
		m.crc = gd_bgzf_le32(h + total - 8), m.isize = gd_bgzf_le32(h + total - 4);
		if (m.isize > GD_BGZF_MAX_ISIZE) return bad("ISIZE above 65536");
		if (max_out && !tab.empty() && out + m.isize > max_out) { if (full) *full = true; break; }
		m.out_off = out, out += m.isize;
		tab.push_back(m);
		at += total;
	}
	if (incomplete_from) *incomplete_from = at;
	return GD_BGZF_OK;
}

// the first bytes of a file are the header of a BGZF member (all of its header must be there)
static inline bool gd_bgzf_first_is_member(const unsigned char *p, size_t n)
{
	if (n < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 0x08 || !(p[3] & 4) || (p[3] & 0x1a)) return false;
	const size_t xlen = gd_bgzf_le16(p + 10);
	if (n < 12 + xlen) return false;
	for (size_t x = 0; x + 4 <= xlen;) {
		const unsigned char *s = p + 12 + x;
		const size_t slen = gd_bgzf_le16(s + 2);
		if (x + 4 + slen > xlen) return false;
		if (s[0] == 'B' && s[1] == 'C' && slen == 2) return true;
		x += 4 + slen;
	}
	return false;
}
// the last 28 bytes of a file are the end-of-file member
static inline bool gd_bgzf_ends_with_marker(const unsigned char *p, size_t n) { return n >= GD_BGZF_EOF_LEN && !memcmp(p + n - GD_BGZF_EOF_LEN, GD_BGZF_EOF, GD_BGZF_EOF_LEN); }

// THE PER-MEMBER CHECK, whoever inflated: the length produced is ISIZE and the zlib crc32 of the bytes is the trailer's.
static inline bool gd_bgzf_check(const GdBgzfMember &m, size_t k, const unsigned char *out, uint32_t out_len, std::string *why)
{
	if (out_len != m.isize) {
		if (why) *why = "BGZF member " + std::to_string(k) + ": " + std::to_string(out_len) + " bytes inflated, ISIZE says " + std::to_string(m.isize);
		return false;
	}
	const uint32_t c = (uint32_t)crc32(crc32(0L, Z_NULL, 0), out, m.isize);
	if (c != m.crc) {
		if (why) *why = "BGZF member " + std::to_string(k) + ": CRC32 mismatch";
		return false;
	}
	return true;
}

// One member through zlib's raw inflate (the unattached reader's route); *out_len is what it produced.  z: an initialised stream or
// one with z->state == nullptr (initialised here); the caller calls inflateEnd.
static inline bool gd_bgzf_inflate_host(z_stream *z, const unsigned char *in, uint32_t in_len, unsigned char *out, uint32_t cap, uint32_t *out_len, size_t k, std::string *why)
{
	const int rc0 = z->state ? inflateReset(z) : inflateInit2(z, -15);
	if (rc0 != Z_OK) { if (why) *why = "zlib: cannot start a raw inflate"; return false; }
	unsigned char none = 0;
	z->next_in = const_cast<unsigned char *>(in), z->avail_in = in_len;
	z->next_out = cap ? out : &none, z->avail_out = cap;
	const int rc = inflate(z, Z_FINISH);
	*out_len = cap - z->avail_out;
	if (rc != Z_STREAM_END) {
		if (why) *why = "BGZF member " + std::to_string(k) + ": " + (rc == Z_BUF_ERROR ? "its deflate stream does not end within the member or overruns ISIZE" : z->msg ? z->msg : "invalid deflate stream");
		return false;
	}
	return true;
}
