// Driver of the coordinate sort of BAM records (bam_sort.hip.h) and its kernel-level boundary gdiet_hip_bam_sort_records.  Included by
// gdiet_hip.hip behind bam_driver.hip.h (needs gdiet_ctx, GdLane, GdStreamMem, err_mark.h, the BAM-input walker of bam_in.h).
//
// One pass over one buffer of whole uncompressed records and the table of their start offsets: bam_key_kernel, hipCUB's stable radix
// sort of (key -> index), bam_permute_kernel, hipCUB's exclusive scan of the permuted sizes, bam_gather_kernel.  hipCUB is called as the
// index builder calls it (map_index_dev.hip.h): the temp-size query, then the run.  Everything runs on the lane gdiet_ctx::bsort with
// stream-ordered allocations; not on the encoder's lane, so that a caller that sorts never holds bam.mu.
#pragma once
#include <hipcub/hipcub.hpp>
#include "bam_sort.hip.h"
#include "bam_index.h"
#include "bam_sorter.h"
#include "bam_markdup_driver.hip.h"

// The pass, enqueued on s: d_in[0, len) and d_start[0, n) are resident; d_out[0, len) takes the sorted records and d_rows[0, n) their
// index rows.  The caller holds bsort.mu, owns mem and synchronises.  0, or -1 with why.
static int gd_bam_sort_pass(gdiet_ctx *ctx, GdStreamMem &mem, const uint8_t *d_in, uint64_t len, const uint64_t *d_start, uint64_t n, uint8_t *d_out, GdsRow *d_rows, std::string &why)
{
	GdLane &L = ctx->bsort;
	hipStream_t s = L.stream;
	hipError_t e = hipSuccess;
	auto fail = [&](hipError_t err, const char *what) {
		why = std::string("BAM sort: ") + what + ": " + hipGetErrorString(err);
		return -1;
	};
	if (n == 0) return 0;
	if (n > 0x7fffffffull) { why = "BAM sort: 2^31 records or more in one pass"; return -1; }
	uint64_t *d_key0, *d_key1, *d_src, *d_psize, *d_dst;
	uint32_t *d_idx0, *d_idx1, *d_size;
	void *d_tmp;
	if ((e = mem.alloc(&d_key0, 8 * n)) != hipSuccess || (e = mem.alloc(&d_key1, 8 * n)) != hipSuccess) return fail(e, "keys");
	if ((e = mem.alloc(&d_idx0, 4 * n)) != hipSuccess || (e = mem.alloc(&d_idx1, 4 * n)) != hipSuccess) return fail(e, "indices");
	if ((e = mem.alloc(&d_size, 4 * n)) != hipSuccess || (e = mem.alloc(&d_psize, 8 * n)) != hipSuccess) return fail(e, "sizes");
	if ((e = mem.alloc(&d_src, 8 * n)) != hipSuccess || (e = mem.alloc(&d_dst, 8 * n)) != hipSuccess) return fail(e, "offsets");
	size_t b1 = 0, b2 = 0;
	if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, b1, d_key0, d_key1, d_idx0, d_idx1, (int)n, 0, 64, s)) != hipSuccess) return fail(e, "sort size");
	if ((e = hipcub::DeviceScan::ExclusiveSum(nullptr, b2, d_psize, d_dst, (int)n, s)) != hipSuccess) return fail(e, "scan size");
	if ((e = mem.alloc((uint8_t **)&d_tmp, std::max<size_t>(std::max(b1, b2), 16))) != hipSuccess) return fail(e, "scratch");
	const dim3 per_thread((unsigned)((n + 255) / 256)), per_wave((unsigned)((n + 3) / 4));
	(void)hipEventRecord(L.ev[0], s);
	hipLaunchKernelGGL(bam_key_kernel, per_thread, dim3(256), 0, s, d_in, len, d_start, n, d_key0, d_idx0, d_size);
	if ((e = hipGetLastError()) != hipSuccess) return fail(e, "key launch");
	if ((e = hipcub::DeviceRadixSort::SortPairs(d_tmp, b1, d_key0, d_key1, d_idx0, d_idx1, (int)n, 0, 64, s)) != hipSuccess) return fail(e, "sort");
	hipLaunchKernelGGL(bam_permute_kernel, per_thread, dim3(256), 0, s, (const uint32_t *)d_idx1, d_start, (const uint32_t *)d_size, n, d_src, d_psize);
	if ((e = hipGetLastError()) != hipSuccess) return fail(e, "permute launch");
	if ((e = hipcub::DeviceScan::ExclusiveSum(d_tmp, b2, d_psize, d_dst, (int)n, s)) != hipSuccess) return fail(e, "scan");
	(void)hipEventRecord(L.ev[1], s);
	hipLaunchKernelGGL(bam_gather_kernel, per_wave, dim3(256), 0, s, d_in, len, (const uint64_t *)d_src, (const uint64_t *)d_psize, (const uint64_t *)d_dst, n, d_out, len, d_rows);
	if ((e = hipGetLastError()) != hipSuccess) return fail(e, "gather launch");
	(void)hipEventRecord(L.ev[2], s);
	return 0;
}

extern "C" int64_t gdiet_hip_bam_sort_records(gdiet_ctx *ctx, const void *recs, size_t len, void *out, void *rows, size_t rows_cap, int64_t *n_rec)
{
	if (!ctx || (!recs && len) || !n_rec) return GDIET_E_PARAM;
	*n_rec = 0;
	gd_err_clear();
	auto fail = [&](int rc, const std::string &what) { return (int64_t)gd_err_fail(ctx, rc, "gdiet_hip_bam_sort_records: " + what); };
	if (len >= ((size_t)1 << 31)) return fail(GDIET_E_PARAM, "2 GiB of records or more");
	GdiWalk W;
	std::vector<uint64_t> start;
	gdi_walk((const uint8_t *)recs, 0, len, false, false, 0, 0, W, &start);
	if (W.bad) return fail(GDIET_E_PARAM, W.msg);
	if (W.pos != len) return fail(GDIET_E_PARAM, "offset " + std::to_string(W.pos) + ": the range ends inside a record");
	const size_t n = start.size();
	*n_rec = (int64_t)n;
	if (!out && !rows) return (int64_t)len; // sizes first
	if (!out || !rows) return fail(GDIET_E_PARAM, "out and rows go together");
	if (rows_cap / sizeof(GdsRow) < n) return fail(GDIET_E_PARAM, std::to_string(n) + " records take " + std::to_string(n * sizeof(GdsRow)) + " bytes of rows, rows holds " + std::to_string(rows_cap));
	if (n == 0) return 0;
	GdLane &L = ctx->bsort;
	std::lock_guard<std::mutex> lk(L.mu);
	std::string why;
	if (L.ready(ctx->device, 3, "BAM sort", why)) return fail(GDIET_E_HIP, why);
	hipStream_t s = L.stream;
	hipError_t e = hipSuccess;
	GdStreamMem mem(s);
	uint8_t *d_in, *d_out;
	uint64_t *d_start;
	GdsRow *d_rows;
	auto hip_fail = [&](hipError_t err, const char *what) {
		mem.fail();
		return fail(GDIET_E_HIP, std::string("BAM sort: ") + what + ": " + hipGetErrorString(err));
	};
	if ((e = mem.alloc(&d_in, len + 16)) != hipSuccess || (e = mem.alloc(&d_out, len + 16)) != hipSuccess) return hip_fail(e, "records");
	if ((e = mem.alloc(&d_start, 8 * n)) != hipSuccess) return hip_fail(e, "starts");
	if ((e = mem.alloc(&d_rows, sizeof(GdsRow) * n)) != hipSuccess) return hip_fail(e, "rows");
	if ((e = hipMemcpyAsync(d_in, recs, len, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e, "records copy");
	if ((e = hipMemcpyAsync(d_start, start.data(), 8 * n, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e, "starts copy");
	if (gd_bam_sort_pass(ctx, mem, d_in, len, d_start, n, d_out, d_rows, why)) { mem.fail(); return fail(GDIET_E_HIP, why); }
	if ((e = hipMemcpyAsync(out, d_out, len, hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(e, "records copy down");
	if ((e = hipMemcpyAsync(rows, d_rows, sizeof(GdsRow) * n, hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(e, "rows copy down");
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(e, "kernels");
	for (int i = 0; i < 2; ++i) { // (for measurements: key + sort + scan, gather)
		float ms = 0;
		if (hipEventElapsedTime(&ms, L.ev[i], L.ev[i + 1]) == hipSuccess) L.ms[i] += ms;
	}
	const GdsRow *r = (const GdsRow *)rows;
	for (size_t k = 0; k < n; ++k)
		if (r[k].out == ~(uint64_t)0) return fail(GDIET_E_HIP, "BAM sort: place " + std::to_string(k) + ": a record outside its buffers");
	return (int64_t)len;
}

// ---- the sorter (bam_sorter.h) on the device ---------------------------------------------------------------------------------------------
// The executor of GdqSorter: two buffers in stream-ordered memory that live as long as the sorter -- the run buffer the encode kernel
// fills, and the resident result [the writer's tail | records in order] the sort pass or a chunk's gather writes and the deflate
// kernel reads -- and the result's index rows.  Every call takes bsort.mu for its own duration; append() takes bam.mu instead (the encode
// kernel runs on the encoder's lane, as in gdiet_hip_bam_batch_into), so a spill never holds the encoder's mutex.
struct GdqDevice {
	gdiet_ctx *ctx = nullptr;
	uint8_t *d_run = nullptr, *d_res = nullptr;
	GdsRow *d_rows = nullptr;
	size_t run_cap = 0, res_cap = 0, rows_cap = 0, front_len = 0;
	uint64_t res_bytes = 0; // of the records of the resident result, behind front_len
	GdAccumSet acc; // gdiet_hip_bam_sort_set_coverage / _set_pileup / _set_stats: every appended batch is scattered from the run buffer, on the encoder's lane

	// p[0, cap) -> at least `need` bytes, the first `keep` bytes kept.  The caller holds bsort.mu and has made the stream.
	template <class T> hipError_t grow(T **p, size_t *cap, size_t need, size_t keep)
	{
		if (*cap >= need) return hipSuccess;
		hipStream_t s = ctx->bsort.stream;
		const size_t want = need + (need >> 3) + 64;
		void *q = nullptr;
		hipError_t e = hipMallocAsync(&q, want, s);
		if (e != hipSuccess) return e;
		if (*p && keep && (e = hipMemcpyAsync(q, *p, keep, hipMemcpyDeviceToDevice, s)) != hipSuccess) { (void)hipFreeAsync(q, s); return e; }
		if (*p) (void)hipFreeAsync(*p, s);
		*p = (T *)q, *cap = want;
		return hipStreamSynchronize(s); // (the encoder's stream writes into the run buffer next)
	}
	static int bad(std::string &why, const char *what, hipError_t e)
	{
		why = std::string("BAM sorter: ") + what + ": " + hipGetErrorString(e);
		return -1;
	}
	int append(const void *batch, uint64_t at, std::string &why)
	{
		const GdbPart &P = *(const GdbPart *)batch;
		{
			std::lock_guard<std::mutex> lk(ctx->bsort.mu);
			if (ctx->bsort.ready(ctx->device, 3, "BAM sorter", why)) return -1;
			const hipError_t e = grow(&d_run, &run_cap, (size_t)(at + P.bytes) + 16, (size_t)at);
			if (e != hipSuccess) return bad(why, "run buffer", e);
		}
		std::lock_guard<std::mutex> lk(ctx->bam.mu);
		GdLane &L = ctx->bam;
		if (L.ready(ctx->device, 4, "device BAM encoder", why)) return -1;
		GdAccumHold held; // (nothing without an attached accumulator)
		if (held.take(acc, why)) return -1;
		hipStream_t s = L.stream;
		hipError_t e = hipSuccess;
		GdStreamMem mem(s);
		uint8_t *d_text, *d_blob;
		uint32_t *d_cig;
		GdbRec *d_rec;
		auto fail = [&](hipError_t err, const char *what) { mem.fail(); return bad(why, what, err); };
		const size_t n = P.rec.size();
		if ((n + 3) / 4 > 0x7fffffffull) { why = "BAM sorter: too many records for one launch"; return -1; }
		if ((e = mem.alloc(&d_text, P.text.size() + 16)) != hipSuccess) return fail(e, "read text");
		if ((e = mem.alloc(&d_blob, P.blob.size() + 16)) != hipSuccess) return fail(e, "tag blobs");
		if ((e = mem.alloc(&d_cig, sizeof(uint32_t) * P.cig.size() + 16)) != hipSuccess) return fail(e, "CIGAR pool");
		if ((e = mem.alloc(&d_rec, sizeof(GdbRec) * n + 16)) != hipSuccess) return fail(e, "record table");
		(void)hipEventRecord(L.ev[0], s);
		if (!P.text.empty() && (e = hipMemcpyAsync(d_text, P.text.data(), P.text.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "read text copy");
		if (!P.blob.empty() && (e = hipMemcpyAsync(d_blob, P.blob.data(), P.blob.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "tag blobs copy");
		if (!P.cig.empty() && (e = hipMemcpyAsync(d_cig, P.cig.data(), sizeof(uint32_t) * P.cig.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "CIGAR pool copy");
		if (n && (e = hipMemcpyAsync(d_rec, P.rec.data(), sizeof(GdbRec) * n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "record table copy");
		(void)hipEventRecord(L.ev[1], s);
		if (n) {
			hipLaunchKernelGGL(bam_encode_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, (const GdbRec *)d_rec, (uint64_t)n, (const uint8_t *)d_text, (const uint32_t *)d_cig,
			                   (const uint8_t *)d_blob, d_run + at, (uint64_t)P.bytes);
			if ((e = hipGetLastError()) != hipSuccess) return fail(e, "encode launch");
		}
		(void)hipEventRecord(L.ev[2], s);
		if (gd_accum_enqueue_all(held, s, d_run + at, P, why)) { mem.fail(); return -1; } // before the run is sorted or moved
		if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "encode kernel");
		if (gd_accum_verdict_all(held, why)) return -1;
		for (int i = 0; i < 2; ++i) {
			float ms = 0;
			if (hipEventElapsedTime(&ms, L.ev[i], L.ev[i + 1]) == hipSuccess) L.ms[i] += ms;
		}
		return 0;
	}
	// the result's buffers for n records of `bytes` bytes behind `front`; the caller holds bsort.mu
	int result(uint64_t n, uint64_t bytes, const uint8_t *front, size_t fl, std::string &why)
	{
		hipError_t e = hipSuccess;
		if ((e = grow(&d_res, &res_cap, fl + (size_t)bytes + 16, 0)) != hipSuccess) return bad(why, "result buffer", e);
		if ((e = grow(&d_rows, &rows_cap, sizeof(GdsRow) * (size_t)n + 16, 0)) != hipSuccess) return bad(why, "rows", e);
		if (fl && (e = hipMemcpyAsync(d_res, front, fl, hipMemcpyHostToDevice, ctx->bsort.stream)) != hipSuccess) return bad(why, "tail copy", e);
		front_len = fl, res_bytes = bytes;
		return 0;
	}
	void time_pass()
	{
		GdLane &L = ctx->bsort;
		for (int i = 0; i < 2; ++i) {
			float ms = 0;
			if (hipEventElapsedTime(&ms, L.ev[i], L.ev[i + 1]) == hipSuccess) L.ms[i] += ms;
		}
	}
	int sort_run(const uint64_t *start, uint64_t n, uint64_t bytes, const uint8_t *front, size_t fl, std::string &why)
	{
		GdLane &L = ctx->bsort;
		std::lock_guard<std::mutex> lk(L.mu);
		if (L.ready(ctx->device, 3, "BAM sorter", why)) return -1;
		if (bytes > run_cap) { why = "BAM sorter: the run is larger than its buffer"; return -1; }
		if (result(n, bytes, front, fl, why)) return -1;
		hipStream_t s = L.stream;
		GdStreamMem mem(s);
		uint64_t *d_start;
		hipError_t e = hipSuccess;
		if ((e = mem.alloc(&d_start, 8 * (size_t)n + 16)) != hipSuccess) return bad(why, "starts", e);
		if ((e = hipMemcpyAsync(d_start, start, 8 * (size_t)n, hipMemcpyHostToDevice, s)) != hipSuccess) { mem.fail(); return bad(why, "starts copy", e); }
		if (gd_bam_sort_pass(ctx, mem, d_run, bytes, d_start, n, d_res + fl, d_rows, why)) { mem.fail(); return -1; }
		if ((e = hipStreamSynchronize(s)) != hipSuccess) { mem.fail(); return bad(why, "sort pass", e); }
		time_pass();
		return 0;
	}
	int order(const uint64_t *keys, uint64_t n, uint32_t *order_out, std::string &why)
	{
		if (n == 0) return 0;
		if (n > 0x7fffffffull) { why = "BAM sorter: 2^31 records or more in one merge"; return -1; }
		GdLane &L = ctx->bsort;
		std::lock_guard<std::mutex> lk(L.mu);
		if (L.ready(ctx->device, 3, "BAM sorter", why)) return -1;
		hipStream_t s = L.stream;
		GdStreamMem mem(s);
		hipError_t e = hipSuccess;
		auto fail = [&](hipError_t err, const char *what) { mem.fail(); return bad(why, what, err); };
		uint64_t *d_k0, *d_k1;
		uint32_t *d_i0, *d_i1;
		void *d_tmp;
		std::vector<uint32_t> iota((size_t)n);
		for (uint64_t k = 0; k < n; ++k) iota[(size_t)k] = (uint32_t)k;
		if ((e = mem.alloc(&d_k0, 8 * (size_t)n)) != hipSuccess || (e = mem.alloc(&d_k1, 8 * (size_t)n)) != hipSuccess) return fail(e, "merge keys");
		if ((e = mem.alloc(&d_i0, 4 * (size_t)n)) != hipSuccess || (e = mem.alloc(&d_i1, 4 * (size_t)n)) != hipSuccess) return fail(e, "merge indices");
		size_t b = 0;
		if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, b, d_k0, d_k1, d_i0, d_i1, (int)n, 0, 64, s)) != hipSuccess) return fail(e, "merge sort size");
		if ((e = mem.alloc((uint8_t **)&d_tmp, std::max<size_t>(b, 16))) != hipSuccess) return fail(e, "merge scratch");
		if ((e = hipMemcpyAsync(d_k0, keys, 8 * (size_t)n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "merge keys copy");
		if ((e = hipMemcpyAsync(d_i0, iota.data(), 4 * (size_t)n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "merge indices copy");
		(void)hipEventRecord(L.ev[0], s);
		if ((e = hipcub::DeviceRadixSort::SortPairs(d_tmp, b, d_k0, d_k1, d_i0, d_i1, (int)n, 0, 64, s)) != hipSuccess) return fail(e, "merge sort");
		(void)hipEventRecord(L.ev[1], s);
		if ((e = hipMemcpyAsync(order_out, d_i1, 4 * (size_t)n, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "order copy");
		if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "merge sort");
		float ms = 0;
		if (hipEventElapsedTime(&ms, L.ev[0], L.ev[1]) == hipSuccess) L.ms[0] += ms;
		return 0;
	}
	int gather(const uint8_t *side, uint64_t side_len, const uint64_t *src, const uint64_t *psize, const uint64_t *dst, uint64_t n, uint64_t bytes, const uint8_t *front, size_t fl,
	           std::string &why)
	{
		GdLane &L = ctx->bsort;
		std::lock_guard<std::mutex> lk(L.mu);
		if (L.ready(ctx->device, 3, "BAM sorter", why)) return -1;
		if (n == 0 || (n + 3) / 4 > 0x7fffffffull) { why = "BAM sorter: a chunk of no or too many records"; return -1; }
		if (result(n, bytes, front, fl, why)) return -1;
		hipStream_t s = L.stream;
		GdStreamMem mem(s);
		hipError_t e = hipSuccess;
		auto fail = [&](hipError_t err, const char *what) { mem.fail(); return bad(why, what, err); };
		uint8_t *d_side;
		uint64_t *d_tab; // src, psize, dst
		if ((e = mem.alloc(&d_side, (size_t)side_len + 16)) != hipSuccess) return fail(e, "chunk");
		if ((e = mem.alloc(&d_tab, 24 * (size_t)n)) != hipSuccess) return fail(e, "chunk tables");
		if ((e = hipMemcpyAsync(d_side, side, (size_t)side_len, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "chunk copy");
		if ((e = hipMemcpyAsync(d_tab, src, 8 * (size_t)n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "chunk tables copy");
		if ((e = hipMemcpyAsync(d_tab + n, psize, 8 * (size_t)n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "chunk tables copy");
		if ((e = hipMemcpyAsync(d_tab + 2 * n, dst, 8 * (size_t)n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "chunk tables copy");
		(void)hipEventRecord(L.ev[1], s);
		hipLaunchKernelGGL(bam_gather_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, (const uint8_t *)d_side, side_len, (const uint64_t *)d_tab, (const uint64_t *)(d_tab + n),
		                   (const uint64_t *)(d_tab + 2 * n), n, d_res + fl, bytes, d_rows);
		if ((e = hipGetLastError()) != hipSuccess) return fail(e, "gather launch");
		(void)hipEventRecord(L.ev[2], s);
		if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "gather");
		float ms = 0;
		if (hipEventElapsedTime(&ms, L.ev[1], L.ev[2]) == hipSuccess) L.ms[1] += ms;
		return 0;
	}
	// ---- duplicate marking (bam_markdup_driver.hip.h) over the resident result of n records -------------------------------------------
	// the entries {key, score} of its records, in its order, down to the host
	int dup_keys(uint64_t n, uint64_t *key, uint32_t *score, std::string &why)
	{
		if (n == 0) return 0;
		GdLane &L = ctx->bsort;
		std::lock_guard<std::mutex> lk(L.mu);
		if (L.ready(ctx->device, 3, "BAM sorter", why)) return -1;
		hipStream_t s = L.stream;
		GdStreamMem mem(s);
		hipError_t e = hipSuccess;
		auto fail = [&](hipError_t err, const char *what) { mem.fail(); return bad(why, what, err); };
		uint64_t *d_key;
		uint32_t *d_score;
		if ((e = mem.alloc(&d_key, 8 * (size_t)n)) != hipSuccess || (e = mem.alloc(&d_score, 4 * (size_t)n)) != hipSuccess) return fail(e, "duplicate entries");
		if (gd_dup_keys_dev(ctx, mem, d_res + front_len, res_bytes, nullptr, d_rows, n, d_key, d_score, nullptr, why)) { mem.fail(); return -1; }
		if ((e = hipMemcpyAsync(key, d_key, 8 * (size_t)n, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "duplicate entries copy down");
		if ((e = hipMemcpyAsync(score, d_score, 4 * (size_t)n, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "duplicate entries copy down");
		if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "duplicate entries copy down");
		return 0;
	}
	// the entries of the whole file in output order -> the bitmap by place ((n + 31) / 32 words) and the counts
	int dup_decide(const uint64_t *key, const uint32_t *score, uint64_t n, uint32_t *bitmap, GdmStats *st, std::string &why)
	{
		*st = GdmStats();
		if (n == 0) return 0;
		GdLane &L = ctx->bsort;
		std::lock_guard<std::mutex> lk(L.mu);
		if (L.ready(ctx->device, 3, "BAM sorter", why)) return -1;
		hipStream_t s = L.stream;
		GdStreamMem mem(s);
		hipError_t e = hipSuccess;
		auto fail = [&](hipError_t err, const char *what) { mem.fail(); return bad(why, what, err); };
		uint64_t *d_key;
		uint32_t *d_score, *d_idx, *d_bitmap, *d_st, h_st[4] = {0, 0, 0, 0};
		const size_t words = (size_t)((n + 31) / 32);
		std::vector<uint32_t> iota((size_t)n);
		for (uint64_t k = 0; k < n; ++k) iota[(size_t)k] = (uint32_t)k;
		if ((e = mem.alloc(&d_key, 8 * (size_t)n)) != hipSuccess || (e = mem.alloc(&d_score, 4 * (size_t)n)) != hipSuccess || (e = mem.alloc(&d_idx, 4 * (size_t)n)) != hipSuccess)
			return fail(e, "duplicate entries");
		if ((e = mem.alloc(&d_bitmap, 4 * words + 16)) != hipSuccess) return fail(e, "duplicate bitmap");
		if ((e = hipMemcpyAsync(d_key, key, 8 * (size_t)n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "duplicate entries copy");
		if ((e = hipMemcpyAsync(d_score, score, 4 * (size_t)n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "duplicate entries copy");
		if ((e = hipMemcpyAsync(d_idx, iota.data(), 4 * (size_t)n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "duplicate entries copy");
		if (gd_dup_decide_dev(ctx, mem, d_key, d_score, d_idx, n, d_bitmap, &d_st, why)) { mem.fail(); return -1; }
		if ((e = hipMemcpyAsync(bitmap, d_bitmap, 4 * words, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "duplicate bitmap copy down");
		if ((e = hipMemcpyAsync(h_st, d_st, 16, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "duplicate counters copy down");
		if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "duplicate decision");
		gd_dup_stats(h_st, n, st);
		return 0;
	}
	// record k of the resident result takes bit bit0 + k of bitmap (bit0 below 32)
	int dup_apply(const uint32_t *bitmap, uint32_t bit0, uint64_t n, std::string &why)
	{
		if (n == 0) return 0;
		GdLane &L = ctx->bsort;
		std::lock_guard<std::mutex> lk(L.mu);
		if (L.ready(ctx->device, 3, "BAM sorter", why)) return -1;
		hipStream_t s = L.stream;
		GdStreamMem mem(s);
		hipError_t e = hipSuccess;
		auto fail = [&](hipError_t err, const char *what) { mem.fail(); return bad(why, what, err); };
		const size_t words = (size_t)((bit0 + n + 31) / 32);
		uint32_t *d_bitmap;
		if ((e = mem.alloc(&d_bitmap, 4 * words + 16)) != hipSuccess) return fail(e, "duplicate bitmap");
		if ((e = hipMemcpyAsync(d_bitmap, bitmap, 4 * words, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "duplicate bitmap copy");
		hipLaunchKernelGGL(dup_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_res + front_len, res_bytes, (const uint64_t *)nullptr, d_rows, n, (const uint32_t *)d_bitmap, bit0);
		if ((e = hipGetLastError()) != hipSuccess) return fail(e, "duplicate apply launch");
		if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "duplicate apply");
		return 0;
	}
	// one run that is the whole file: key pass, decision and rewrite where the records are
	int dup_mark_resident(uint64_t n, GdmStats *st, std::string &why)
	{
		*st = GdmStats();
		if (n == 0) return 0;
		GdLane &L = ctx->bsort;
		std::lock_guard<std::mutex> lk(L.mu);
		if (L.ready(ctx->device, 3, "BAM sorter", why)) return -1;
		GdStreamMem mem(L.stream);
		if (gd_dup_mark_dev(ctx, mem, d_res + front_len, res_bytes, nullptr, d_rows, n, st, why)) { mem.fail(); return -1; }
		return 0;
	}
	int down(void *dst, const void *d_src, size_t n, const char *what, std::string &why)
	{
		GdLane &L = ctx->bsort;
		std::lock_guard<std::mutex> lk(L.mu);
		hipError_t e = hipMemcpyAsync(dst, d_src, n, hipMemcpyDeviceToHost, L.stream);
		if (e == hipSuccess) e = hipStreamSynchronize(L.stream);
		return e == hipSuccess ? 0 : bad(why, what, e);
	}
	int fetch_rows(GdsRow *rows, uint64_t n, std::string &why) { return down(rows, d_rows, sizeof(GdsRow) * (size_t)n, "rows copy down", why); }
	int fetch(uint64_t from, uint64_t n_bytes, uint8_t *dst, std::string &why) { return down(dst, d_res + from, (size_t)n_bytes, "records copy down", why); }
	const void *resident() const { return d_res; }
	void seconds(double *key_sort, double *gather_s)
	{
		std::lock_guard<std::mutex> lk(ctx->bsort.mu);
		*key_sort = 1e-3 * (ctx->bsort.ms[0] - ms0[0]), *gather_s = 1e-3 * (ctx->bsort.ms[1] - ms0[1]);
	}
	double ms0[2] = {0, 0}; // the lane's sums when the sorter was opened
	void free_all()
	{
		if (!ctx) return;
		std::lock_guard<std::mutex> lk(ctx->bsort.mu);
		hipStream_t s = ctx->bsort.stream;
		if (s) (void)hipStreamSynchronize(s);
		for (void *p : {(void *)d_run, (void *)d_res, (void *)d_rows})
			if (p) (void)hipFreeAsync(p, s);
		d_run = d_res = nullptr, d_rows = nullptr, run_cap = res_cap = rows_cap = 0;
	}
};

struct gdiet_bam_sorter {
	GdqSorter<GdqDevice> q;
	gdiet_ctx *ctx = nullptr;
	GdbPart part; // the flattened batch on its way into the run buffer (swapped with the context's pool, so both keep their pages)
};

static int gd_bsq_fail(gdiet_bam_sorter *h, int rc, const char *who)
{
	return gd_err_fail(h->ctx, rc, std::string(who) + ": " + (h->q.msg.empty() ? std::string("used after an error") : h->q.msg));
}

extern "C" int gdiet_hip_bam_sort_open(gdiet_ctx *ctx, const char *path, const void *header, size_t header_len, int bgzf_device, int level, int threads, uint64_t run_bytes,
                                       uint64_t chunk_bytes, const char *tmp_dir, int want_index, gdiet_bam_sorter **out)
{
	if (!ctx || !path || !header || !out || level < -1 || level > 9) return GDIET_E_PARAM;
	*out = nullptr;
	gd_err_clear();
	gdiet_bam_sorter *h = new gdiet_bam_sorter();
	h->ctx = ctx, h->q.ex.ctx = ctx;
	{
		std::lock_guard<std::mutex> lk(ctx->bsort.mu);
		h->q.ex.ms0[0] = ctx->bsort.ms[0], h->q.ex.ms0[1] = ctx->bsort.ms[1];
	}
	const int rc = h->q.open(path, (const uint8_t *)header, header_len, bgzf_device != 0, level, threads, run_bytes, chunk_bytes, tmp_dir, want_index != 0,
	                         bgzf_device ? std::shared_ptr<GdBgzfDeflater>(std::make_shared<GdBzdExecutor>(ctx)) : std::shared_ptr<GdBgzfDeflater>());
	*out = h; // also when open refused: the handle then takes nothing but its close, which frees it
	if (rc) return gd_bsq_fail(h, rc == -2 ? GDIET_E_PARAM : (h->q.w.dev_error ? GDIET_E_HIP : GDIET_E_PARAM), "gdiet_hip_bam_sort_open");
	return GDIET_OK;
}

extern "C" int gdiet_hip_bam_sort_add(gdiet_bam_sorter *h, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs, const char *const *quals,
                                      const char *const *comments, const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs, int64_t opt_flag)
{
	if (!h || !gd_bam_args_ok(h->ctx, ix, n_reads, qnames, seqs, lens, n_regs, regs)) return GDIET_E_PARAM;
	gd_err_clear();
	if (h->q.failed) return gd_bsq_fail(h, GDIET_E_PARAM, "gdiet_hip_bam_sort_add");
	gdiet_ctx *ctx = h->ctx;
	{
		std::lock_guard<std::mutex> lk(ctx->bam.mu);
		GdbPart &P = gd_bam_pool(ctx).all;
		std::string why;
		const int rc = gd_bam_flatten(ctx, ix, n_reads, qnames, seqs, quals, comments, lens, n_regs, regs, opt_flag, P, why);
		if (rc) return why.empty() ? rc : gd_err_fail(ctx, rc, "gdiet_hip_bam_sort_add: " + why);
		std::swap(P, h->part);
	}
	const GdbPart &P = h->part;
	std::vector<uint64_t> rec_out(P.rec.size());
	for (size_t k = 0; k < P.rec.size(); ++k) rec_out[k] = P.rec[k].out; // record starts: no walk
	const int rc = h->q.add(&P, P.bytes, rec_out.data(), P.rec.size());
	if (rc) return gd_bsq_fail(h, rc == -2 ? GDIET_E_PARAM : GDIET_E_HIP, "gdiet_hip_bam_sort_add");
	return GDIET_OK;
}

extern "C" int gdiet_hip_bam_sort_set_coverage(gdiet_bam_sorter *h, gdiet_coverage *cov)
{
	return h ? gd_accum_attach(h->ctx, h->q.ex.acc, GD_ACC_COV, cov, "gdiet_hip_bam_sort_set_coverage", "sorter") : GDIET_E_PARAM;
}
extern "C" int gdiet_hip_bam_sort_set_pileup(gdiet_bam_sorter *h, gdiet_pileup *pile)
{
	return h ? gd_accum_attach(h->ctx, h->q.ex.acc, GD_ACC_PILE, pile, "gdiet_hip_bam_sort_set_pileup", "sorter") : GDIET_E_PARAM;
}

extern "C" int gdiet_hip_bam_sort_set_stats(gdiet_bam_sorter *h, gdiet_stats *stats)
{
	return h ? gd_accum_attach(h->ctx, h->q.ex.acc, GD_ACC_STATS, stats, "gdiet_hip_bam_sort_set_stats", "sorter") : GDIET_E_PARAM;
}

extern "C" int gdiet_hip_bam_sort_set_markdup(gdiet_bam_sorter *h, int on)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	if (h->q.failed) return gd_bsq_fail(h, GDIET_E_PARAM, "gdiet_hip_bam_sort_set_markdup");
	if (h->q.set_markdup(on != 0)) return gd_err_fail(h->ctx, GDIET_E_PARAM, "gdiet_hip_bam_sort_set_markdup: the sorter has taken records: duplicate marking is chosen before the first add");
	return GDIET_OK;
}

extern "C" int gdiet_hip_bam_sort_close_dup(gdiet_bam_sorter *h, gdiet_bam_sort_stats_t *stats, gdiet_dup_stats_t *dup_stats)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	const int rc = h->q.close();
	if (stats) {
		const GdqStats &s = h->q.st;
		stats->records = s.records, stats->runs = s.runs, stats->spooled_bytes = s.spooled_bytes, stats->chunks = s.chunks, stats->members = s.members, stats->n_no_coor = s.n_no_coor;
		for (int i = 0; i < 5; ++i) stats->seconds[i] = s.seconds[i];
	}
	gd_dup_stats_out(h->q.dup, dup_stats);
	const int code = rc ? gd_bsq_fail(h, h->q.w.dev_error ? GDIET_E_HIP : GDIET_E_PARAM, "gdiet_hip_bam_sort_close") : GDIET_OK;
	h->q.ex.free_all();
	delete h;
	return code;
}
extern "C" int gdiet_hip_bam_sort_close(gdiet_bam_sorter *h, gdiet_bam_sort_stats_t *stats) { return gdiet_hip_bam_sort_close_dup(h, stats, nullptr); }
