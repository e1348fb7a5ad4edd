// The host's plan of the merge of several sorted runs of BAM records into one coordinate-sorted stream.  Host only, no HIP.
//
// Every run is sorted by the key of bam_sort.h, and a run's sorted keys and record sizes stay in host memory.  The runs' key arrays
// concatenated in run order and sorted once, stably, give the global order: a permutation of the global record numbers (run 0's records
// first).  It is stable over (run, index in run), hence over input order.  gdq_plan_chunks cuts that order into chunks: a chunk is the
// longest prefix of what is left that holds at most chunk_bytes, and always at least one record.  Because every run is sorted and the
// global sort is stable, the records a chunk takes from one run are one contiguous range of that run, so a chunk is read from the
// runs' spools with one sequential read per run, the ranges are laid side by side, and bam_gather_kernel moves the records into their
// final order with the source offsets this plan gives.
//
// GdqSorter is the sorter itself, with everything the device does behind an executor (a template parameter, as in ksw_plan.h /
// map_plan.h: the driver's executor runs kernels, a test's may run the emulator's loops):
//   add     the batch is encoded into the resident run buffer at the run's fill mark (Ex::append); when it would not fit in run_bytes the
//           run is SEALED first.  A batch larger than run_bytes is a run of its own.
//   seal    the device pass over the run (Ex::sort_run), the sorted run down to the host and into a spool file of its own in tmp_dir,
//           created and unlinked at once, written sequentially, uncompressed.  The run's sorted keys and record sizes stay: 12 bytes
//           per record.
//   markdup (off by default; bam_markdup.h): a spooled run's entries {key, score} are taken from the resident sorted run at its seal and
//           stay on the host, 12 more bytes per record.  At close one run is marked where it is; several runs: the entries are laid out
//           in output order behind Ex::order, ONE decision covers the whole file (groups span runs and chunks) and gives a bitmap by
//           place, and every chunk is rewritten with its slice of the bitmap between its gather and its emit.
//   close   one run that was never spooled: its sorted buffer is the output stream as it is.  Several runs: one stable device sort of the
//           concatenated keys (Ex::order), the plan, and per chunk the ranges read from the spools, laid side by side, gathered
//           (Ex::gather).  The stream -- header, then records -- goes through the BGZF writer core (GdBgzfOut), from the resident buffer
//           on the device route; the writer's member log and the gather's index rows give the .bai (bam_index.h).
// After a failure (a short spool or output write, a device failure) the sorter refuses everything but its close, which frees the spools
// and removes a partial .bai.
#pragma once
#include <errno.h>
#include <fcntl.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <algorithm>
#include <chrono>
#include <string>
#include <type_traits>
#include <vector>
#include "bam_index.h"
#include "bam_markdup.h"
#include "bgzf_out.h"

struct GdqRange { uint64_t lo = 0, hi = 0, byte_lo = 0, byte_hi = 0; }; // records [lo, hi) of a run: bytes [byte_lo, byte_hi) of its spool
struct GdqChunk {
	uint64_t j0 = 0, j1 = 0, bytes = 0; // places [j0, j1) of the global order
	std::vector<GdqRange> run;          // one range per run (lo == hi: none)
	std::vector<uint32_t> run_of;       // the run of the record at place j0 + k
};

// order[0, n): the global order (global record numbers); size[g]: bytes of record g; run_n[r]: records of run r (their sum is n).
// false with why: the order is no permutation that keeps every run's own order.
static inline bool gdq_plan_chunks(const uint32_t *order, const uint32_t *size, uint64_t n, const std::vector<uint64_t> &run_n, uint64_t chunk_bytes, std::vector<GdqChunk> &out,
                                   std::string &why)
{
	out.clear();
	const size_t R = run_n.size();
	std::vector<uint64_t> base(R + 1, 0);
	for (size_t r = 0; r < R; ++r) base[r + 1] = base[r] + run_n[r];
	if (base[R] != n) { why = "merge plan: the runs hold " + std::to_string(base[R]) + " records, the order " + std::to_string(n); return false; }
	std::vector<uint64_t> next(R, 0), next_byte(R, 0); // per run: the record the order must take next, and where it starts in the spool
	uint64_t j = 0;
	while (j < n) {
		GdqChunk c;
		c.j0 = j, c.run.resize(R);
		for (size_t r = 0; r < R; ++r) c.run[r].lo = c.run[r].hi = next[r], c.run[r].byte_lo = c.run[r].byte_hi = next_byte[r];
		for (; j < n; ++j) {
			const uint64_t g = order[j];
			if (g >= n) { why = "merge plan: place " + std::to_string(j) + " names record " + std::to_string(g); return false; }
			const uint64_t sz = size[g];
			if (j > c.j0 && (c.bytes + sz > chunk_bytes || c.bytes + sz < c.bytes)) break;
			const size_t r = (size_t)(std::upper_bound(base.begin(), base.end(), g) - base.begin()) - 1;
			if (g - base[r] != next[r]) { why = "merge plan: place " + std::to_string(j) + " takes record " + std::to_string(g - base[r]) + " of run " + std::to_string(r) + " out of turn"; return false; }
			c.run_of.push_back((uint32_t)r);
			++next[r], next_byte[r] += sz, c.bytes += sz;
			c.run[r].hi = next[r], c.run[r].byte_hi = next_byte[r];
		}
		c.j1 = j;
		out.push_back(c);
	}
	return true;
}

struct GdqStats {
	int64_t records = 0, runs = 0, spooled_bytes = 0, chunks = 0, members = 0, n_no_coor = 0;
	double seconds[5] = {0, 0, 0, 0, 0}; // key + sort | gather (both the device's, from the lane's events) | spool write | spool read | compress and write (wall)
};

// l_ref of every reference of a BAM header (magic, l_text, text, n_ref, {l_name, name, l_ref}); false: not a header
static inline bool gdq_header_refs(const uint8_t *h, size_t n, std::vector<std::pair<std::string, uint32_t>> &refs)
{
	auto le32 = [&](size_t at) { return (uint32_t)h[at] | (uint32_t)h[at + 1] << 8 | (uint32_t)h[at + 2] << 16 | (uint32_t)h[at + 3] << 24; };
	if (n < 12 || memcmp(h, "BAM\1", 4) != 0) return false;
	size_t p = 8 + (size_t)le32(4);
	if (p + 4 > n) return false;
	const uint32_t n_ref = le32(p);
	p += 4;
	for (uint32_t k = 0; k < n_ref; ++k) {
		if (p + 4 > n) return false;
		const uint32_t l_name = le32(p);
		if (l_name == 0 || p + 8 + (size_t)l_name > n) return false;
		refs.push_back(std::make_pair(std::string((const char *)h + p + 4, l_name - 1), le32(p + 4 + l_name)));
		p += 8 + (size_t)l_name;
	}
	return p == n;
}

// Ex (all return 0, or -1 with why set; "resident result" = [front | records in order] in device memory, with the records' rows):
//   int append(const void *batch, uint64_t at, std::string &why)        the batch's records encoded into the run buffer at byte `at`
//   int sort_run(const uint64_t *start, uint64_t n, uint64_t bytes, const uint8_t *front, size_t front_len, std::string &why)
//                                                                       the device pass over the run buffer -> resident result
//   int order(const uint64_t *keys, uint64_t n, uint32_t *order, std::string &why)     stable sort of keys: order[j] = index of the j-th
//   int gather(const uint8_t *side, uint64_t side_len, const uint64_t *src, const uint64_t *psize, const uint64_t *dst, uint64_t n,
//              uint64_t bytes, const uint8_t *front, size_t front_len, std::string &why)                        -> resident result
//   int fetch_rows(GdsRow *rows, uint64_t n, std::string &why)          the rows of the resident result (out = offset behind front)
//   int fetch(uint64_t from, uint64_t n_bytes, uint8_t *dst, std::string &why)         bytes [from, from + n_bytes) of the resident result
//   const void *resident()                                              the device address of the resident result
//   void seconds(double *key_sort, double *gather)                      the device's time so far
// An executor that marks duplicates (bam_markdup.h) has four more; GdqSorter reaches them only where GdqHasDup finds them, so an executor
// without them sorts as before and refuses set_markdup:
//   int dup_keys(uint64_t n, uint64_t *key, uint32_t *score, std::string &why)     the entries of the resident result's n records, in its order
//   int dup_decide(const uint64_t *key, const uint32_t *score, uint64_t n, uint32_t *bitmap, GdmStats *st, std::string &why)
//                                                                       entries in output order -> bit j: the record at place j is a duplicate
//   int dup_apply(const uint32_t *bitmap, uint32_t bit0, uint64_t n, std::string &why)  record k of the resident result takes bit bit0 + k
//   int dup_mark_resident(uint64_t n, GdmStats *st, std::string &why)   all three over the resident result alone
// A bad record (bam_markdup.h) fails dup_keys / dup_mark_resident with its text.
template <class Ex, class = void> struct GdqHasDup : std::false_type {};
template <class Ex> struct GdqHasDup<Ex, std::void_t<decltype(&Ex::dup_keys), decltype(&Ex::dup_decide), decltype(&Ex::dup_apply), decltype(&Ex::dup_mark_resident)>> : std::true_type {};

template <class Ex>
struct GdqSorter {
	Ex ex;
	GdBgzfOut w;
	std::string path, tmp_dir;
	bool device_route = false, want_index = true, failed = false;
	bool opened = false; // open() succeeded: only then is there a file to end and an index to write
	std::string msg;
	uint64_t run_bytes = 512ull << 20, chunk_bytes = 256ull << 20;
	uint64_t header_len = 0, records_len = 0; // of the output stream
	uint32_t n_ref = 0;
	// the open run
	uint64_t fill = 0;
	std::vector<uint64_t> start;
	// the sealed runs
	struct Run { int fd = -1; uint64_t n = 0, bytes = 0; };
	std::vector<Run> runs;
	std::vector<uint64_t> keys;   // of all sealed runs, in run order
	std::vector<uint32_t> sizes;
	std::vector<GdsRow> rows;     // of the output, for the index
	std::vector<std::pair<uint64_t, uint64_t>> log;
	std::vector<uint8_t> host;    // a run or a chunk on its way
	GdqStats st;
	// duplicate marking (off: nothing below is touched and the executor is asked for nothing more)
	bool markdup = false, added = false;
	std::vector<uint64_t> dup_key;   // {key, score} of all sealed runs, in run order: 12 more bytes per record
	std::vector<uint32_t> dup_score;
	GdmStats dup;

	int fail(const std::string &what) { if (!failed) failed = true, msg = what; return -1; }
	static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

	// the header goes into the stream at once.  0, -1 (msg), -2: a parameter (msg)
	int open(const char *out_path, const uint8_t *header, size_t n_header, bool on_device, int level, int threads, uint64_t run_b, uint64_t chunk_b, const char *tmp, bool index,
	         std::shared_ptr<GdBgzfDeflater> dev)
	{
		std::vector<std::pair<std::string, uint32_t>> refs;
		if (!gdq_header_refs(header, n_header, refs)) { fail("the header is no BAM header"); return -2; }
		for (const auto &r : refs)
			if (index && r.second > (uint32_t)GDX_MAX_REF_LEN) { fail("contig " + r.first + " is longer than 2^29: the BAI index cannot hold it (CSI is out of scope)"); return -2; }
		path = out_path, device_route = on_device, want_index = index, n_ref = (uint32_t)refs.size();
		if (run_b) run_bytes = run_b;
		if (chunk_b) chunk_bytes = chunk_b;
		tmp_dir = tmp && *tmp ? std::string(tmp) : (path.find('/') == std::string::npos ? std::string(".") : path.substr(0, path.rfind('/') + 1));
		if (::access(tmp_dir.c_str(), W_OK | X_OK) != 0) { fail("tmp_dir " + tmp_dir + ": " + strerror(errno)); return -2; }
		const int fd = ::open(out_path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
		if (fd < 0) { fail(path + ": " + strerror(errno)); return -2; }
		w.fd = fd, w.level = level, w.threads = threads < 1 ? 1 : threads, w.dev = dev, w.member_log = &log;
		header_len = n_header;
		opened = true;
		if (w.write(header, n_header)) return fail("output: " + w.msg);
		return 0;
	}

	// 0; -1: records have been added, or the executor cannot mark
	int set_markdup(bool on)
	{
		if (added || (on && !GdqHasDup<Ex>::value)) return -1;
		markdup = on;
		return 0;
	}

	int spool_new(Run &r)
	{
		std::string name = tmp_dir + (tmp_dir.back() == '/' ? "" : "/") + "gdiet_sort_XXXXXX";
		r.fd = ::mkstemp(&name[0]);
		if (r.fd < 0) return fail("spool " + name + ": " + strerror(errno));
		(void)::unlink(name.c_str()); // nothing is left behind whatever happens
		return 0;
	}
	int spool_write(int fd, const uint8_t *p, size_t n)
	{
		while (n) {
			const ssize_t k = ::write(fd, p, n);
			if (k < 0 && errno == EINTR) continue;
			if (k <= 0) return fail(k < 0 ? std::string("spool write: ") + strerror(errno) : std::string("spool write: short write"));
			p += k, n -= (size_t)k;
		}
		return 0;
	}
	int spool_read(int fd, uint64_t at, uint8_t *p, size_t n)
	{
		while (n) {
			const ssize_t k = ::pread(fd, p, n, (off_t)at);
			if (k < 0 && errno == EINTR) continue;
			if (k <= 0) return fail(k < 0 ? std::string("spool read: ") + strerror(errno) : std::string("spool read: the spool is short"));
			p += k, n -= (size_t)k, at += (uint64_t)k;
		}
		return 0;
	}

	// the resident result of n records and `bytes` bytes behind the writer's tail goes into the stream; its rows are kept for the index
	int emit(uint64_t n, uint64_t bytes, size_t front_len)
	{
		std::string why;
		const size_t r0 = rows.size();
		rows.resize(r0 + n);
		if (n && ex.fetch_rows(rows.data() + r0, n, why)) return fail(why);
		for (size_t k = r0; k < rows.size(); ++k) {
			if (rows[k].out == ~(uint64_t)0) return fail("BAM sort: a record outside its buffers");
			rows[k].out += records_len;
		}
		if (!want_index) rows.resize(r0);
		records_len += bytes;
		const double t0 = now();
		if (device_route) { // every whole member is compressed where it is; the rest comes down as the next tail
			const uint64_t total = front_len + bytes, whole = total / GD_BGZF_MEMBER_IN * GD_BGZF_MEMBER_IN;
			std::vector<unsigned char> next_tail((size_t)(total - whole));
			if (!next_tail.empty() && ex.fetch(whole, total - whole, next_tail.data(), why)) return fail(why);
			if (w.members_resident(ex.resident(), (size_t)whole)) return fail("output: " + (w.msg.empty() ? std::string("the writer refused") : w.msg));
			w.tail.swap(next_tail);
		} else {
			host.resize((size_t)bytes);
			if (bytes && ex.fetch(front_len, bytes, host.data(), why)) return fail(why);
			if (w.write(host.data(), (size_t)bytes)) return fail("output: " + w.msg);
		}
		st.seconds[4] += now() - t0;
		return 0;
	}
	const uint8_t *front(size_t *len) { *len = device_route ? w.tail.size() : 0; return device_route ? w.tail.data() : nullptr; }

	// the open run: sorted; spooled, or (final and alone) straight into the stream
	int seal(bool last)
	{
		if (start.empty()) return 0;
		std::string why;
		const uint64_t n = start.size(), bytes = fill;
		const bool direct = last && runs.empty();
		size_t fl = 0;
		const uint8_t *f = direct ? front(&fl) : nullptr;
		if (ex.sort_run(start.data(), n, bytes, f, fl, why)) return fail(why);
		++st.runs;
		start.clear(), fill = 0;
		if constexpr (GdqHasDup<Ex>::value) {
			if (markdup && direct && ex.dup_mark_resident(n, &dup, why)) return fail(why);
			if (markdup && !direct) {
				const size_t d0 = dup_key.size();
				dup_key.resize(d0 + (size_t)n), dup_score.resize(d0 + (size_t)n);
				if (ex.dup_keys(n, dup_key.data() + d0, dup_score.data() + d0, why)) return fail(why);
			}
		}
		if (direct) return emit(n, bytes, fl);
		std::vector<GdsRow> rr((size_t)n);
		host.resize((size_t)bytes);
		if (ex.fetch_rows(rr.data(), n, why) || ex.fetch(0, bytes, host.data(), why)) return fail(why);
		Run r;
		r.n = n, r.bytes = bytes;
		if (spool_new(r)) return -1;
		runs.push_back(r);
		const double t0 = now();
		if (spool_write(r.fd, host.data(), (size_t)bytes)) return -1;
		st.seconds[2] += now() - t0, st.spooled_bytes += (int64_t)bytes;
		for (uint64_t k = 0; k < n; ++k) {
			if (rr[k].out == ~(uint64_t)0) return fail("BAM sort: a record outside its buffers");
			keys.push_back(rr[k].key), sizes.push_back((uint32_t)((k + 1 < n ? rr[k + 1].out : bytes) - rr[k].out));
		}
		return 0;
	}

	// n records of `bytes` bytes; batch is what Ex::append takes.  0, -1, -2 (a parameter)
	int add(const void *batch, uint64_t bytes, const uint64_t *rec_out, uint64_t n)
	{
		if (failed) return -1;
		added = true;
		if (n == 0) return 0;
		if ((uint64_t)st.records + n >= ((uint64_t)1 << 31)) { fail("2^31 records or more in one file"); return -2; } // (the merge's one sort counts them in an int)
		if (fill && fill + bytes > run_bytes && seal(false)) return -1;
		std::string why;
		if (ex.append(batch, fill, why)) return fail(why);
		for (uint64_t k = 0; k < n; ++k) start.push_back(fill + rec_out[k]);
		fill += bytes, st.records += (int64_t)n;
		return 0;
	}

	int merge()
	{
		std::string why;
		const uint64_t n = keys.size();
		std::vector<uint32_t> order((size_t)n);
		if (ex.order(keys.data(), n, order.data(), why)) return fail(why);
		std::vector<uint64_t> run_n, base(1, 0);
		for (const Run &r : runs) run_n.push_back(r.n), base.push_back(base.back() + r.n);
		std::vector<GdqChunk> plan;
		if (!gdq_plan_chunks(order.data(), sizes.data(), n, run_n, chunk_bytes, plan, why)) return fail(why);
		std::vector<uint32_t> bitmap; // by place: the one decision over the whole file, taken before the first chunk is streamed
		if constexpr (GdqHasDup<Ex>::value)
			if (markdup) {
				std::vector<uint64_t> ek((size_t)n);
				std::vector<uint32_t> es((size_t)n);
				for (uint64_t j = 0; j < n; ++j) ek[(size_t)j] = dup_key[order[(size_t)j]], es[(size_t)j] = dup_score[order[(size_t)j]];
				bitmap.assign((size_t)((n + 31) / 32) + 1, 0u);
				if (ex.dup_decide(ek.data(), es.data(), n, bitmap.data(), &dup, why)) return fail(why);
			}
		std::vector<uint64_t> src, psize, dst, side_at(runs.size());
		std::vector<std::vector<uint64_t>> at(runs.size()); // per run: where the records of the chunk's range start in the side-by-side buffer
		for (const GdqChunk &c : plan) {
			host.resize((size_t)c.bytes);
			uint64_t fillc = 0;
			const double t0 = now();
			for (size_t r = 0; r < runs.size(); ++r) {
				const GdqRange &g = c.run[r];
				side_at[r] = fillc;
				if (g.byte_hi > g.byte_lo && spool_read(runs[r].fd, g.byte_lo, host.data() + fillc, (size_t)(g.byte_hi - g.byte_lo))) return -1;
				at[r].resize((size_t)(g.hi - g.lo));
				uint64_t o = fillc;
				for (uint64_t i = g.lo; i < g.hi; ++i) at[r][(size_t)(i - g.lo)] = o, o += sizes[(size_t)(base[r] + i)];
				fillc += g.byte_hi - g.byte_lo;
			}
			st.seconds[3] += now() - t0;
			const uint64_t m = c.j1 - c.j0;
			src.resize((size_t)m), psize.resize((size_t)m), dst.resize((size_t)m);
			uint64_t sum = 0;
			for (uint64_t j = c.j0; j < c.j1; ++j) {
				const uint64_t g = order[(size_t)j];
				const size_t r = c.run_of[(size_t)(j - c.j0)];
				src[(size_t)(j - c.j0)] = at[r][(size_t)(g - base[r] - c.run[r].lo)], psize[(size_t)(j - c.j0)] = sizes[(size_t)g], dst[(size_t)(j - c.j0)] = sum, sum += sizes[(size_t)g];
			}
			size_t fl = 0;
			const uint8_t *f = front(&fl);
			if (ex.gather(host.data(), c.bytes, src.data(), psize.data(), dst.data(), m, c.bytes, f, fl, why)) return fail(why);
			if constexpr (GdqHasDup<Ex>::value)
				if (markdup && ex.dup_apply(bitmap.data() + (c.j0 >> 5), (uint32_t)(c.j0 & 31u), m, why)) return fail(why);
			if (emit(m, c.bytes, fl)) return -1;
			++st.chunks;
		}
		return 0;
	}

	// the rest of the stream, the end-of-file member, the index.  Frees the spools either way.
	int close()
	{
		if (!opened) return 0; // (open refused: nothing was created, nothing is left to free but the object)
		if (!failed) {
			if (runs.empty()) (void)seal(true);
			else if (!seal(false)) (void)merge();
		}
		for (Run &r : runs)
			if (r.fd >= 0) ::close(r.fd), r.fd = -1;
		const std::string bai = path + ".bai";
		if (!failed) {
			const double t0 = now();
			if (w.close()) fail("output: " + w.msg);
			st.seconds[4] += now() - t0;
		}
		if (!failed && want_index) {
			std::vector<GdxMember> ml;
			for (const auto &m : log) ml.push_back(GdxMember{m.first, m.second});
			uint64_t nnc = 0;
			const std::string b = gdx_bai_build(rows.data(), rows.size(), n_ref, header_len, records_len, ml, &nnc);
			st.n_no_coor = (int64_t)nnc;
			const int fd = ::open(bai.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
			if (fd < 0) fail(bai + ": " + strerror(errno));
			else {
				if (spool_write(fd, (const uint8_t *)b.data(), b.size())) msg = bai + ": " + msg;
				if (::close(fd) != 0 && !failed) fail(bai + ": " + strerror(errno));
			}
		}
		if (failed && want_index && !path.empty()) (void)::unlink(bai.c_str());
		st.members = (int64_t)log.size();
		ex.seconds(&st.seconds[0], &st.seconds[1]);
		return failed ? -1 : 0;
	}
};
