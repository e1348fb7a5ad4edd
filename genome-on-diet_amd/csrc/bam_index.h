// The BAI index (SAM specification 5.2) of a coordinate-sorted BAM file, built in one sequential pass over the index rows the gather
// kernel wrote (bam_sort.h: GdsRow, in file order) and the writer's member log.  Host only, no HIP.  The rules are those of
// include/gdiet_hip.h, "Sorted BAM output":
//   * a record covers [pos, pos + max(ref_len, 1)) -- the row's [pos, end); the windows of the linear index are taken from
//     max(pos, 0) >> 14 to (max(end, 1) - 1) >> 14;
//   * its bin is the bin it carries; a chunk is a maximal stretch of consecutive records of one reference with one bin, from the first
//     record's start to the last record's end; bins ascend, pseudo-bin 37450 comes last for every reference that has a record;
//   * ioffset[w] is the start of the first record covering window w, an uncovered window takes the value of the next covered one;
//   * records with refID outside [0, n_ref) are counted in n_no_coor and nothing else.
// A virtual offset is member_file_offset << 16 | offset_in_member; the stream offset x lies in the first member m with x < in_end[m];
// the end of the stream is the file offset behind the last data member (where the end-of-file member goes) << 16.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>
#include "bam_sort.h"

struct GdxMember { uint64_t in_bytes, file_bytes; }; // one BGZF member of the output, in file order (the writer's log)

enum { GDX_PSEUDO_BIN = 37450, GDX_MAX_REF_LEN = 1 << 29 };

struct GdxVoffs {
	std::vector<uint64_t> in_end, file_at; // prefix sums of the log, over the members that hold input
	uint64_t file_end = 0;                 // the file offset behind the last member that holds input: where the end-of-file member starts
	size_t m = 0;                          // the cursor: offsets are asked for in ascending order
	explicit GdxVoffs(const std::vector<GdxMember> &log)
	{
		uint64_t in = 0, file = 0;
		for (const GdxMember &g : log) {
			if (g.in_bytes) file_at.push_back(file), in += g.in_bytes, in_end.push_back(in), file_end = file + g.file_bytes; // (an empty member holds no offset)
			file += g.file_bytes;
		}
	}
	uint64_t at(uint64_t x)
	{
		if (m > 0 && x < in_end[m - 1]) m = 0; // (not ascending: start again)
		while (m < in_end.size() && x >= in_end[m]) ++m;
		if (m == in_end.size()) return file_end << 16;
		return file_at[m] << 16 | (x - (m ? in_end[m - 1] : 0));
	}
};

static inline void gdx_put32(std::string &o, uint32_t v) { for (int k = 0; k < 4; ++k) o.push_back((char)(v >> (8 * k))); }
static inline void gdx_put64(std::string &o, uint64_t v) { for (int k = 0; k < 8; ++k) o.push_back((char)(v >> (8 * k))); }

// rows[0, n) in file order; the record of row i ends where that of row i + 1 starts, the last at records_len; `base` is the stream offset
// of the first record (the header's length).  Returns the bytes of the .bai file.
static inline std::string gdx_bai_build(const GdsRow *rows, uint64_t n, uint32_t n_ref, uint64_t base, uint64_t records_len, const std::vector<GdxMember> &log, uint64_t *n_no_coor_out = nullptr)
{
	std::string o("BAI\1", 4);
	gdx_put32(o, n_ref);
	GdxVoffs V(log);
	uint64_t i = 0, n_no_coor = 0;
	// (a row of an earlier reference than the one in turn is out of coordinate order: counted as unplaced; the sorter never produces one)
	for (uint32_t ref = 0; ref < n_ref; ++ref) {
		std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;
		std::vector<uint64_t> lin;
		std::vector<bool> have;
		uint64_t first = 0, last = 0, n_map = 0, n_unmap = 0, n_here = 0;
		uint32_t prev_bin = ~0u;
		while (i < n && rows[i].refID >= 0 && (uint32_t)rows[i].refID < ref) ++i, ++n_no_coor;
		for (; i < n && rows[i].refID == (int32_t)ref; ++i) {
			const GdsRow &r = rows[i];
			const uint64_t beg = V.at(base + r.out);
			const uint64_t end = V.at(base + (i + 1 < n ? rows[i + 1].out : records_len));
			if (!n_here++) first = beg;
			last = end;
			(r.flag & 4u) ? ++n_unmap : ++n_map;
			if (r.bin != prev_bin) bins[r.bin].push_back(std::make_pair(beg, end)), prev_bin = r.bin;
			else bins[r.bin].back().second = end;
			const int64_t p0 = r.pos > 0 ? r.pos : 0, p1 = (r.end > 1 ? (int64_t)r.end : 1) - 1;
			const uint64_t w0 = (uint64_t)(p0 >> 14), w1 = (uint64_t)((p1 < p0 ? p0 : p1) >> 14);
			if (lin.size() <= w1) lin.resize(w1 + 1, 0), have.resize(w1 + 1, false);
			for (uint64_t w = w0; w <= w1; ++w)
				if (!have[w]) have[w] = true, lin[w] = beg;
		}
		gdx_put32(o, n_here ? (uint32_t)bins.size() + 1 : 0);
		for (const auto &b : bins) {
			gdx_put32(o, b.first), gdx_put32(o, (uint32_t)b.second.size());
			for (const auto &c : b.second) gdx_put64(o, c.first), gdx_put64(o, c.second);
		}
		if (n_here) {
			gdx_put32(o, GDX_PSEUDO_BIN), gdx_put32(o, 2);
			gdx_put64(o, first), gdx_put64(o, last), gdx_put64(o, n_map), gdx_put64(o, n_unmap);
		}
		for (size_t w = lin.size(); w-- > 0;)
			if (!have[w]) lin[w] = w + 1 < lin.size() ? lin[w + 1] : 0;
		gdx_put32(o, (uint32_t)lin.size());
		for (uint64_t v : lin) gdx_put64(o, v);
	}
	n_no_coor += n - i;
	gdx_put64(o, n_no_coor);
	if (n_no_coor_out) *n_no_coor_out = n_no_coor;
	return o;
}
