// Coordinate order of BAM alignment records (include/gdiet_hip.h, "Sorted BAM output"): the statements of the sort pass, written once for
// the kernels (bam_sort.hip.h), for the host emulator that runs them as loops over 64 lanes (tests/emul/bam_sort_emul.cpp) and for the
// driver.  No HIP in here.  The pass reads nothing but the records' own bytes (SAM specification 4.2): it sorts any BAM records.
//
//   gds_key          the 64-bit sort key and the size of the record that starts at an offset of a buffer, from the record's fixed fields.
//                    Records are not aligned in a stream, so every field is assembled from byte loads.
//   gds_gather_lane  lane l of the 64 that move one record from its source offset to its sorted offset.
//   gds_ref_len_lane lane l's share of the reference length of the record's CIGAR field: the words l, l + 64, ...; the 64 shares add up.
//   gds_row          the 32-byte index row of a record at its sorted offset: what the .bai builder (bam_index.h) needs and nothing else,
//                    so the host never looks at a record's bytes again.
// HOW THE COPY IS DONE.  The destination decides: the first (4 - dst) & 3 bytes go as single bytes (lanes 0 .. 2), which brings the
// destination to a 4-byte boundary; from there lane l moves the 32-bit words l, l + 64, ... (the source of a word is wherever it is: the
// load is a 4-byte memcpy, which gfx950 executes as one unaligned dword load, the host as whatever it likes); the last 0 .. 3 bytes go as
// single bytes again.  A wavefront therefore stores 256 consecutive, aligned bytes per step whatever the pair of offsets is.
// BOUNDS.  Every load is checked against the source record's end and every store against the destination record's end (both are n
// here: the size the tables give the record).  A table that disagrees with itself can lose bytes, never touch a byte outside
// [src, src + n) and [dst, dst + n).  No lane reads what another lane wrote: no fence, and the order of the lanes cannot matter.
#pragma once
#include <stdint.h>
#include <string.h>
#include "bam_record.h"

#define GDS_HD GDB_HD

enum { GDS_FIXED = 36 }; // block_size and the 32 fixed bytes behind it

// 32 bytes, 16-byte aligned in its table
struct GdsRow {
	uint64_t key;
	uint64_t out;      // where the record starts in the sorted stream of records
	int32_t refID, pos;
	int32_t end;       // pos + max(reference length of the CIGAR field, 1)
	uint16_t bin, flag;
};
static_assert(sizeof(GdsRow) == 32, "an index row is 32 bytes");

GDS_HD uint32_t gds_le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
GDS_HD uint32_t gds_le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

GDS_HD uint64_t gds_key_of(int32_t refID, int32_t pos, uint32_t flag)
{
	return (uint64_t)(uint32_t)refID << 32 | (uint64_t)((uint32_t)(pos + 1u) << 1 | (flag >> 4 & 1u));
}

// The record that starts at buf + at, in a buffer of len bytes.  Returns its size (4 + block_size) and its key; 0 and the largest key if
// its fixed bytes or its block_size leave the buffer (the driver's walk has refused such a buffer before: this is the kernel's own guard).
GDS_HD uint32_t gds_key(const uint8_t *buf, uint64_t len, uint64_t at, uint64_t *key)
{
	*key = ~(uint64_t)0;
	if (at > len || len - at < GDS_FIXED) return 0;
	const uint8_t *r = buf + at;
	const uint32_t bs = gds_le32(r);
	if (bs < 32u || bs > 0x7ffffffbu || len - at - 4 < bs) return 0;
	*key = gds_key_of((int32_t)gds_le32(r + 4), (int32_t)gds_le32(r + 8), gds_le16(r + 18));
	return bs + 4u;
}

GDS_HD void gds_copy1(const uint8_t *src, uint8_t *dst, uint64_t k, uint64_t n) { if (k < n) dst[k] = src[k]; }
GDS_HD void gds_copy4(const uint8_t *src, uint8_t *dst, uint64_t k, uint64_t n)
{
	if (k + 4 > n) return;
	uint32_t w;
	memcpy(&w, src + k, 4);
	memcpy(dst + k, &w, 4);
}
// lane `lane` of 64: src[0, n) -> dst[0, n)
GDS_HD void gds_gather_lane(const uint8_t *src, uint8_t *dst, uint64_t n, uint32_t lane)
{
	const uint64_t head = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u, h = head < n ? head : n;
	if (lane < h) gds_copy1(src, dst, lane, n);
	const uint64_t words = (n - h) >> 2;
	for (uint64_t k = lane; k < words; k += 64) gds_copy4(src, dst, h + 4 * k, n);
	const uint64_t t0 = h + 4 * words;
	if (lane < n - t0) gds_copy1(src, dst, t0 + lane, n);
}

// the reference length of one CIGAR word: M D N = X consume the reference
GDS_HD uint32_t gds_op_ref(uint32_t w)
{
	const uint32_t op = w & 15u;
	return (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) ? w >> 4 : 0u;
}
// rec[0, n): a record whose fixed bytes are inside (n >= 36)
GDS_HD uint32_t gds_ref_len_lane(const uint8_t *rec, uint64_t n, uint32_t lane)
{
	const uint64_t at = GDS_FIXED + (uint64_t)rec[12];
	const uint32_t n_op = gds_le16(rec + 16);
	uint32_t sum = 0;
	for (uint32_t k = lane; k < n_op; k += 64) {
		const uint64_t p = at + 4ull * k;
		if (p + 4 <= n) sum += gds_op_ref(gds_le32(rec + p));
	}
	return sum;
}
GDS_HD GdsRow gds_row(const uint8_t *rec, uint64_t out, uint32_t ref_len)
{
	GdsRow r;
	r.refID = (int32_t)gds_le32(rec + 4), r.pos = (int32_t)gds_le32(rec + 8);
	r.bin = (uint16_t)gds_le16(rec + 14), r.flag = (uint16_t)gds_le16(rec + 18);
	r.key = gds_key_of(r.refID, r.pos, r.flag);
	r.out = out;
	r.end = (int32_t)((uint32_t)r.pos + (ref_len ? ref_len : 1u));
	return r;
}
