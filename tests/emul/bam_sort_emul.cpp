// Stand-alone host run of the coordinate sort of BAM records, meant to be built with -fsanitize=address,undefined: the statements of
// bam_key_kernel and bam_gather_kernel (bam_sort.h) as loops over records and over 64 lanes, on exact-size copies of every buffer, so
// that a read or a store outside them is a sanitizer report; the merge plan (bam_sorter.h: gdq_plan_chunks) and the index builder
// (bam_index.h: gdx_bai_build).  std::stable_sort and a running sum stand for hipCUB's radix sort and scan.
//
//   bam_sort_emul sort <in.records> <out.sorted> <out.rows>
//       one pass over one buffer.  Every record is gathered with the lanes running 0..63 and 63..0, with the destination buffer at each of
//       the four alignments mod 4, and over two different fills (every byte must be written).
//   bam_sort_emul merge <in.records> <records per run> <chunk bytes> <out.sorted> <out.rows>
//       the records cut into runs in input order, every run sorted as above, the runs' keys concatenated and sorted stably, the plan,
//       and per chunk the runs' ranges laid side by side and gathered.  Prints the plan: "CHUNK j0 j1 bytes", then one
//       "RUN r lo hi byte_lo byte_hi" per run.
//   bam_sort_emul bai <in.rows> <n_ref> <base> <records_len> <log.txt> <out.bai>
//       the index of the rows; log.txt holds one "<input bytes> <file bytes>" per member.  Prints n_no_coor.
//   bam_sort_emul sorter ...  the sorter itself over these loops: see run_sorter below.
// Exit status 0; 2 usage / file errors; 3 malformed records or a refused plan (the reason goes to stderr); 7 two runs of the same gather
// differ, a byte was left unwritten or written outside the record, or a guard refused a record of a consistent table.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <fstream>
#include <iostream>
#include <memory>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>
#include "bam_in.h"
#include "bam_index.h"
#include "bam_sorter.h"

static bool read_file(const char *path, std::string &out)
{
	std::ifstream f(path, std::ios::binary);
	if (!f) { perror(path); return false; }
	std::stringstream ss;
	ss << f.rdbuf();
	out = ss.str();
	return true;
}
static bool write_file(const char *path, const void *p, size_t n)
{
	FILE *fo = fopen(path, "wb");
	if (!fo) { perror(path); return false; }
	const bool ok = n == 0 || fwrite(p, 1, n, fo) == n;
	return fclose(fo) == 0 && ok;
}
static std::unique_ptr<uint8_t[]> exact(const std::string &s)
{
	std::unique_ptr<uint8_t[]> p(new uint8_t[s.size()]);
	if (!s.empty()) memcpy(p.get(), s.data(), s.size());
	return p;
}

// the statements of bam_gather_kernel for the table (src, psize, dst) over in[0, in_len): out[0, out_len) and one row per record
// (rows' offsets are dst + row_base).  0 or 7.
static int gather(const uint8_t *in, uint64_t in_len, const std::vector<uint64_t> &src, const std::vector<uint64_t> &psize, const std::vector<uint64_t> &dst, uint64_t out_len,
                  uint64_t row_base, std::string &out, std::vector<GdsRow> &rows)
{
	const size_t n = src.size();
	std::string first;
	std::vector<GdsRow> first_rows;
	for (int variant = 0; variant < 9; ++variant) { // 4 alignments x 2 lane orders, then another fill
		const int shift = variant < 8 ? variant >> 1 : 0, down = variant & 1;
		const uint8_t fill = variant < 8 ? 0xA5 : 0x5A;
		std::unique_ptr<uint8_t[]> buf(new uint8_t[out_len + shift]); // (new[] returns 16-byte aligned memory: shift is the alignment mod 4)
		for (uint64_t k = 0; k < out_len + shift; ++k) buf[k] = fill;
		uint8_t *o = buf.get() + shift;
		std::vector<GdsRow> rw(n);
		for (size_t j = 0; j < n; ++j) {
			const uint64_t s = src[j], d = dst[j], sz = psize[j];
			if (sz < GDS_FIXED || s > in_len || in_len - s < sz || d > out_len || out_len - d < sz) return 7; // the kernel's own guard
			uint32_t ref_len = 0;
			for (uint32_t i = 0; i < 64; ++i) {
				const uint32_t lane = down ? 63 - i : i;
				gds_gather_lane(in + s, o + d, sz, lane);
				ref_len += gds_ref_len_lane(in + s, sz, lane);
			}
			rw[j] = gds_row(in + s, d + row_base, ref_len);
		}
		for (int k = 0; k < shift; ++k)
			if (buf[k] != fill) return 7;
		const std::string got((const char *)o, out_len);
		if (variant == 0) first = got, first_rows = rw;
		else if (got != first || (n && memcmp(rw.data(), first_rows.data(), sizeof(GdsRow) * n) != 0)) return 7;
	}
	out = first, rows = first_rows;
	return 0;
}

// one pass over one buffer: bam_key_kernel's statement per record, a stable sort, bam_permute_kernel's, a running sum, the gather
static int sort_table(const std::string &data, const std::vector<uint64_t> &start, std::string &out, std::vector<GdsRow> &rows, std::vector<uint64_t> &keys, std::vector<uint32_t> &sizes)
{
	const auto in = exact(data);
	const size_t n = start.size();
	std::vector<uint64_t> key(n);
	std::vector<uint32_t> size(n), idx(n);
	for (size_t k = 0; k < n; ++k) {
		size[k] = gds_key(in.get(), data.size(), start[k], &key[k]);
		if (!size[k]) return 7;
		idx[k] = (uint32_t)k;
	}
	std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
	std::vector<uint64_t> src(n), psize(n), dst(n);
	uint64_t sum = 0;
	keys.resize(n), sizes.resize(n);
	for (size_t j = 0; j < n; ++j) src[j] = start[idx[j]], psize[j] = size[idx[j]], dst[j] = sum, sum += psize[j], keys[j] = key[idx[j]], sizes[j] = size[idx[j]];
	if (sum != data.size()) return 7;
	return gather(in.get(), data.size(), src, psize, dst, data.size(), 0, out, rows);
}

static int sort_pass(const std::string &data, std::string &out, std::vector<GdsRow> &rows, std::vector<uint64_t> &keys, std::vector<uint32_t> &sizes)
{
	GdiWalk W;
	std::vector<uint64_t> start;
	gdi_walk((const uint8_t *)data.data(), 0, data.size(), false, false, 0, 0, W, &start);
	if (W.bad || W.pos != data.size()) { fprintf(stderr, "%s\n", W.bad ? W.msg.c_str() : "the input ends inside a record"); return 3; }
	return sort_table(data, start, out, rows, keys, sizes);
}

static int run_sort(const char *in_path, const char *out_path, const char *rows_path)
{
	std::string data, out;
	if (!read_file(in_path, data)) return 2;
	std::vector<GdsRow> rows;
	std::vector<uint64_t> keys;
	std::vector<uint32_t> sizes;
	const int rc = sort_pass(data, out, rows, keys, sizes);
	if (rc) return rc;
	for (size_t j = 0; j < rows.size(); ++j)
		if (rows[j].key != keys[j]) return 7;
	return write_file(out_path, out.data(), out.size()) && write_file(rows_path, rows.data(), sizeof(GdsRow) * rows.size()) ? 0 : 2;
}

static int run_merge(const char *in_path, uint64_t per_run, uint64_t chunk_bytes, const char *out_path, const char *rows_path)
{
	std::string data;
	if (!read_file(in_path, data) || per_run == 0) return 2;
	GdiWalk W;
	std::vector<uint64_t> start;
	gdi_walk((const uint8_t *)data.data(), 0, data.size(), false, false, 0, 0, W, &start);
	if (W.bad || W.pos != data.size()) { fprintf(stderr, "%s\n", W.bad ? W.msg.c_str() : "the input ends inside a record"); return 3; }
	start.push_back(data.size());
	// the runs: sorted spools with their keys and sizes
	std::vector<std::string> spool;
	std::vector<uint64_t> all_keys, run_n;
	std::vector<uint32_t> all_sizes;
	std::vector<std::vector<uint64_t>> rec_at; // per run: where record i starts in the spool
	for (size_t k = 0; k + 1 < start.size(); k += per_run) {
		const size_t k1 = std::min(start.size() - 1, k + (size_t)per_run);
		std::string out;
		std::vector<GdsRow> rows;
		std::vector<uint64_t> keys;
		std::vector<uint32_t> sizes;
		const int rc = sort_pass(data.substr(start[k], start[k1] - start[k]), out, rows, keys, sizes);
		if (rc) return rc;
		std::vector<uint64_t> at;
		for (const GdsRow &r : rows) at.push_back(r.out);
		spool.push_back(out), run_n.push_back(keys.size()), rec_at.push_back(at);
		all_keys.insert(all_keys.end(), keys.begin(), keys.end()), all_sizes.insert(all_sizes.end(), sizes.begin(), sizes.end());
	}
	const size_t n = all_keys.size(), R = spool.size();
	std::vector<uint32_t> order(n);
	std::iota(order.begin(), order.end(), 0u);
	std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return all_keys[a] < all_keys[b]; });
	std::vector<GdqChunk> plan;
	std::string why;
	if (!gdq_plan_chunks(order.data(), all_sizes.data(), n, run_n, chunk_bytes, plan, why)) { fprintf(stderr, "%s\n", why.c_str()); return 3; }
	std::vector<uint64_t> base(R + 1, 0);
	for (size_t r = 0; r < R; ++r) base[r + 1] = base[r] + run_n[r];
	std::string merged;
	std::vector<GdsRow> merged_rows;
	for (const GdqChunk &c : plan) {
		printf("CHUNK %llu %llu %llu\n", (unsigned long long)c.j0, (unsigned long long)c.j1, (unsigned long long)c.bytes);
		std::string side; // the runs' ranges side by side, as they are read from the spools
		std::vector<uint64_t> side_at(R);
		for (size_t r = 0; r < R; ++r) {
			const GdqRange &g = c.run[r];
			printf("RUN %zu %llu %llu %llu %llu\n", r, (unsigned long long)g.lo, (unsigned long long)g.hi, (unsigned long long)g.byte_lo, (unsigned long long)g.byte_hi);
			if (g.byte_hi > spool[r].size() || g.byte_lo > g.byte_hi) return 7;
			side_at[r] = side.size(), side += spool[r].substr(g.byte_lo, g.byte_hi - g.byte_lo);
		}
		if (side.size() != c.bytes) return 7;
		std::vector<uint64_t> src, psize, dst;
		uint64_t sum = 0;
		for (uint64_t j = c.j0; j < c.j1; ++j) {
			const uint64_t g = order[j];
			const size_t r = c.run_of[(size_t)(j - c.j0)];
			src.push_back(side_at[r] + rec_at[r][g - base[r]] - c.run[r].byte_lo), psize.push_back(all_sizes[g]), dst.push_back(sum), sum += all_sizes[g];
		}
		const auto in = exact(side);
		std::string out;
		std::vector<GdsRow> rows;
		const int rc = gather(in.get(), side.size(), src, psize, dst, c.bytes, merged.size(), out, rows);
		if (rc) return rc;
		merged += out, merged_rows.insert(merged_rows.end(), rows.begin(), rows.end());
	}
	return write_file(out_path, merged.data(), merged.size()) && write_file(rows_path, merged_rows.data(), sizeof(GdsRow) * merged_rows.size()) ? 0 : 2;
}

static int run_bai(const char *rows_path, uint32_t n_ref, uint64_t base, uint64_t records_len, const char *log_path, const char *out_path)
{
	std::string raw;
	if (!read_file(rows_path, raw) || raw.size() % sizeof(GdsRow)) return 2;
	const size_t n = raw.size() / sizeof(GdsRow);
	std::unique_ptr<GdsRow[]> rows(new GdsRow[n]);
	if (n) memcpy(rows.get(), raw.data(), raw.size());
	std::ifstream lf(log_path);
	if (!lf) { perror(log_path); return 2; }
	std::vector<GdxMember> log;
	unsigned long long a, b;
	while (lf >> a >> b) log.push_back(GdxMember{a, b});
	uint64_t n_no_coor = 0;
	const std::string bai = gdx_bai_build(rows.get(), n, n_ref, base, records_len, log, &n_no_coor);
	printf("%llu\n", (unsigned long long)n_no_coor);
	return write_file(out_path, bai.data(), bai.size()) ? 0 : 2;
}

// ---- the sorter (GdqSorter) over an executor that runs the loops above in host memory ---------------------------------------------------
struct HostEx {
	std::string run, res;
	std::vector<GdsRow> rows;
	int append(const void *batch, uint64_t at, std::string &)
	{
		run.resize((size_t)at);
		run += *(const std::string *)batch;
		return 0;
	}
	int done(int rc, const uint8_t *front, size_t fl, const std::string &out, std::string &why)
	{
		if (rc) { why = "the emulated pass failed with " + std::to_string(rc); return -1; }
		res.assign((const char *)front, fl), res += out;
		return 0;
	}
	int sort_run(const uint64_t *start, uint64_t n, uint64_t bytes, const uint8_t *front, size_t fl, std::string &why)
	{
		std::string out;
		std::vector<uint64_t> keys;
		std::vector<uint32_t> sizes;
		if (bytes != run.size()) { why = "the run buffer holds another number of bytes"; return -1; }
		return done(sort_table(run, std::vector<uint64_t>(start, start + n), out, rows, keys, sizes), front, fl, out, why);
	}
	int order(const uint64_t *keys, uint64_t n, uint32_t *order, std::string &)
	{
		std::iota(order, order + n, 0u);
		std::stable_sort(order, order + n, [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
		return 0;
	}
	int gather(const uint8_t *side, uint64_t side_len, const uint64_t *src, const uint64_t *psize, const uint64_t *dst, uint64_t n, uint64_t bytes, const uint8_t *front, size_t fl,
	           std::string &why)
	{
		const auto in = exact(std::string((const char *)side, side_len));
		std::string out;
		return done(::gather(in.get(), side_len, std::vector<uint64_t>(src, src + n), std::vector<uint64_t>(psize, psize + n), std::vector<uint64_t>(dst, dst + n), bytes, 0, out, rows),
		            front, fl, out, why);
	}
	int fetch_rows(GdsRow *r, uint64_t n, std::string &why)
	{
		if (n != rows.size()) { why = "another number of rows"; return -1; }
		std::copy(rows.begin(), rows.end(), r);
		return 0;
	}
	int fetch(uint64_t from, uint64_t n, uint8_t *dst, std::string &why)
	{
		if (from + n > res.size()) { why = "a fetch outside the result"; return -1; }
		if (n) memcpy(dst, res.data() + from, n);
		return 0;
	}
	const void *resident() const { return res.data(); }
	void seconds(double *a, double *b) { *a = *b = 0; }
};
// stands for the device's deflater: members from an input "resident" in host memory, by zlib at level 1
struct HostResidentDeflater : GdBgzfDeflater {
	int deflate(const unsigned char *in, size_t in_len, unsigned char *out, size_t out_cap, size_t *out_len, std::string &why) override
	{
		*out_len = 0;
		for (size_t at = 0; at < in_len; at += GD_BGZF_MEMBER_IN) {
			if (out_cap - *out_len < GD_BGZF_SLOT) { why = "the output is too small"; return -1; }
			const size_t m = gd_bgzf_member_host(in + at, (uint32_t)std::min<size_t>(GD_BGZF_MEMBER_IN, in_len - at), out + *out_len, 1);
			if (!m) { why = "zlib failed"; return -1; }
			*out_len += m;
		}
		return 0;
	}
	int deflate_resident(const void *d_in, size_t in_len, unsigned char *out, size_t out_cap, size_t *out_len, std::string &why) override
	{
		return deflate((const unsigned char *)d_in, in_len, out, out_cap, out_len, why);
	}
};

//   bam_sort_emul sorter <in.records> <records per batch> <run bytes> <chunk bytes> <tmp dir> <header file> <device 0|1> <out.bam>
//       GdqSorter over the loops above: the records go in in batches, <out.bam> and <out.bam>.bai come out.  Prints
//       "records runs spooled_bytes chunks members n_no_coor".  Exit status 4: open refused (the reason goes to stderr), 5: add or close failed.
static int run_sorter(const char *in_path, uint64_t per_batch, uint64_t run_bytes, uint64_t chunk_bytes, const char *tmp, const char *header_path, bool device, const char *out_path)
{
	std::string data, header;
	if (!read_file(in_path, data) || !read_file(header_path, header) || per_batch == 0) return 2;
	GdiWalk W;
	std::vector<uint64_t> start;
	gdi_walk((const uint8_t *)data.data(), 0, data.size(), false, false, 0, 0, W, &start);
	if (W.bad || W.pos != data.size()) { fprintf(stderr, "%s\n", W.bad ? W.msg.c_str() : "the input ends inside a record"); return 3; }
	start.push_back(data.size());
	GdqSorter<HostEx> q;
	if (q.open(out_path, (const uint8_t *)header.data(), header.size(), device, 1, 2, run_bytes, chunk_bytes, tmp, true,
	           device ? std::shared_ptr<GdBgzfDeflater>(std::make_shared<HostResidentDeflater>()) : std::shared_ptr<GdBgzfDeflater>())) {
		fprintf(stderr, "%s\n", q.msg.c_str());
		(void)q.close();
		return 4;
	}
	int rc = 0;
	for (size_t k = 0; k + 1 < start.size() && !rc; k += per_batch) {
		const size_t k1 = std::min(start.size() - 1, k + (size_t)per_batch);
		const std::string batch = data.substr(start[k], start[k1] - start[k]);
		std::vector<uint64_t> rec_out;
		for (size_t i = k; i < k1; ++i) rec_out.push_back(start[i] - start[k]);
		rc = q.add(&batch, batch.size(), rec_out.data(), rec_out.size());
	}
	if (q.close() || rc) { fprintf(stderr, "%s\n", q.msg.c_str()); return 5; }
	const GdqStats &s = q.st;
	printf("%lld %lld %lld %lld %lld %lld\n", (long long)s.records, (long long)s.runs, (long long)s.spooled_bytes, (long long)s.chunks, (long long)s.members, (long long)s.n_no_coor);
	return 0;
}

int main(int argc, char **argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "sort" && argc == 5) return run_sort(argv[2], argv[3], argv[4]);
	if (mode == "merge" && argc == 7) return run_merge(argv[2], strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10), argv[5], argv[6]);
	if (mode == "bai" && argc == 8) return run_bai(argv[2], (uint32_t)strtoul(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10), strtoull(argv[5], nullptr, 10), argv[6], argv[7]);
	if (mode == "sorter" && argc == 10)
		return run_sorter(argv[2], strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10), strtoull(argv[5], nullptr, 10), argv[6], argv[7], argv[8][0] == '1', argv[9]);
	fprintf(stderr, "usage: bam_sort_emul sort <in> <out> <rows> | merge <in> <records per run> <chunk bytes> <out> <rows> | bai <rows> <n_ref> <base> <records_len> <log> <out> | sorter <in> <records per batch> <run bytes> <chunk bytes> <tmp dir> <header> <device> <out.bam>\n");
	return 2;
}
