// Driver of duplicate marking (bam_markdup.hip.h) and its kernel-level boundary gdiet_hip_bam_markdup_records.  Included by
// bam_sort_driver.hip.h in front of the sorter's executor, whose dup_* methods end here (needs gdiet_ctx, GdLane, GdStreamMem, err_mark.h).
//
// THE KEY PASS writes one entry {key, score} per record of a resident buffer, in the buffer's order.  THE DECISION takes entries in output
// order and gives a bitmap by place: hipCUB's stable radix sort by descending score (values: the places), dup_permute_kernel for the keys
// in that order, hipCUB's stable radix sort by key, dup_decide_kernel.  hipCUB is called as the sort pass calls it: the temp-size query,
// then the run.  THE REWRITE is dup_apply_kernel over a resident buffer and its slice of the bitmap.  Everything runs on the lane
// gdiet_ctx::bsort with stream-ordered allocations; the caller holds bsort.mu, owns mem, and the functions synchronise where they hand a
// verdict or counts to the host.
// DEVICE MEMORY of the decision, per record: key 8 + score 4 + place 4 (the entries), score 4 + place 4 (after the first sort), key 8
// (permuted) + key 8 + place 4 (after the second sort) = 44 bytes, one bit of the bitmap, and hipCUB's scratch.
#pragma once
#include <hipcub/hipcub.hpp>
#include "bam_markdup.hip.h"
#include "bam_starts.h"

// 0; -1 with why: the device failed; -2 with why: a bad record (the text names the first one and its reason)
static int gd_dup_keys_dev(gdiet_ctx *ctx, GdStreamMem &mem, const uint8_t *d_recs, uint64_t len, const uint64_t *d_start, const GdsRow *d_rows, uint64_t n, uint64_t *d_key,
                           uint32_t *d_score, uint32_t *d_idx, std::string &why)
{
	hipStream_t s = ctx->bsort.stream;
	hipError_t e = hipSuccess;
	auto fail = [&](hipError_t err, const char *what) {
		why = std::string("duplicate marking: ") + what + ": " + hipGetErrorString(err);
		return -1;
	};
	if (n == 0) return 0;
	if ((n + 3) / 4 > 0x7fffffffull) { why = "duplicate marking: too many records for one launch"; return -1; }
	uint64_t *d_bad, h_bad = ~(uint64_t)0;
	if ((e = mem.alloc(&d_bad, 8)) != hipSuccess) return fail(e, "cell");
	if ((e = hipMemsetAsync(d_bad, 0xff, 8, s)) != hipSuccess) return fail(e, "cell");
	hipLaunchKernelGGL(dup_key_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, d_recs, len, d_start, d_rows, n, d_key, d_score, d_idx, d_bad);
	if ((e = hipGetLastError()) != hipSuccess) return fail(e, "key launch");
	if ((e = hipMemcpyAsync(&h_bad, d_bad, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "cell copy down");
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "key kernel");
	if (h_bad == ~(uint64_t)0) return 0;
	why = "duplicate marking: record " + std::to_string(h_bad >> 8) + " of the buffer: " + gdm_reason_text((uint32_t)(h_bad & 0xff));
	return -2;
}

// d_key / d_score / d_idx[0, n): the entries in output order and their places 0 .. n - 1 (the two sorts use them up); d_bitmap takes
// (n + 31) / 32 words.  Enqueued; *d_st_out (eligible, duplicates, max_group) is the caller's to copy down behind it.  0, or -1 with why
static int gd_dup_decide_dev(gdiet_ctx *ctx, GdStreamMem &mem, uint64_t *d_key, uint32_t *d_score, uint32_t *d_idx, uint64_t n, uint32_t *d_bitmap, uint32_t **d_st_out, std::string &why)
{
	hipStream_t s = ctx->bsort.stream;
	hipError_t e = hipSuccess;
	auto fail = [&](hipError_t err, const char *what) {
		why = std::string("duplicate marking: ") + what + ": " + hipGetErrorString(err);
		return -1;
	};
	uint32_t *d_st;
	if ((e = mem.alloc(&d_st, 16)) != hipSuccess || (e = hipMemsetAsync(d_st, 0, 16, s)) != hipSuccess) return fail(e, "counters");
	*d_st_out = d_st;
	if (n == 0) return 0;
	if (n > 0x7fffffffull) { why = "duplicate marking: 2^31 records or more in one decision"; return -1; }
	uint64_t *d_pkey, *d_skey;
	uint32_t *d_score1, *d_idx1, *d_idx2;
	void *d_tmp;
	if ((e = mem.alloc(&d_score1, 4 * n)) != hipSuccess || (e = mem.alloc(&d_idx1, 4 * n)) != hipSuccess || (e = mem.alloc(&d_idx2, 4 * n)) != hipSuccess) return fail(e, "sorted places");
	if ((e = mem.alloc(&d_pkey, 8 * n)) != hipSuccess || (e = mem.alloc(&d_skey, 8 * n)) != hipSuccess) return fail(e, "sorted keys");
	size_t b1 = 0, b2 = 0;
	if ((e = hipcub::DeviceRadixSort::SortPairsDescending(nullptr, b1, d_score, d_score1, d_idx, d_idx1, (int)n, 0, 32, s)) != hipSuccess) return fail(e, "score sort size");
	if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, b2, d_pkey, d_skey, d_idx1, d_idx2, (int)n, 0, 64, s)) != hipSuccess) return fail(e, "key sort size");
	if ((e = mem.alloc((uint8_t **)&d_tmp, std::max<size_t>(std::max(b1, b2), 16))) != hipSuccess) return fail(e, "scratch");
	if ((e = hipMemsetAsync(d_bitmap, 0, 4 * (size_t)((n + 31) / 32), s)) != hipSuccess) return fail(e, "bitmap");
	const dim3 per_thread((unsigned)((n + 255) / 256));
	if ((e = hipcub::DeviceRadixSort::SortPairsDescending(d_tmp, b1, d_score, d_score1, d_idx, d_idx1, (int)n, 0, 32, s)) != hipSuccess) return fail(e, "score sort");
	hipLaunchKernelGGL(dup_permute_kernel, per_thread, dim3(256), 0, s, (const uint32_t *)d_idx1, (const uint64_t *)d_key, n, d_pkey);
	if ((e = hipGetLastError()) != hipSuccess) return fail(e, "permute launch");
	if ((e = hipcub::DeviceRadixSort::SortPairs(d_tmp, b2, d_pkey, d_skey, d_idx1, d_idx2, (int)n, 0, 64, s)) != hipSuccess) return fail(e, "key sort");
	hipLaunchKernelGGL(dup_decide_kernel, per_thread, dim3(256), 0, s, (const uint64_t *)d_skey, (const uint32_t *)d_idx2, n, d_bitmap, d_st);
	if ((e = hipGetLastError()) != hipSuccess) return fail(e, "decide launch");
	return 0;
}

static void gd_dup_stats(const uint32_t *h_st, uint64_t n, GdmStats *st)
{
	st->examined = (int64_t)n, st->eligible = h_st[0], st->duplicates = h_st[1], st->max_group = h_st[2];
}

// Key pass, decision and rewrite over one resident buffer: d_recs[0, len) holds n records that start at d_rows[k].out or d_start[k].
// Synchronised when it returns.  0, -1 (device), -2 (a bad record: nothing was rewritten)
static int gd_dup_mark_dev(gdiet_ctx *ctx, GdStreamMem &mem, uint8_t *d_recs, uint64_t len, const uint64_t *d_start, GdsRow *d_rows, uint64_t n, GdmStats *st, std::string &why)
{
	hipStream_t s = ctx->bsort.stream;
	hipError_t e = hipSuccess;
	auto fail = [&](hipError_t err, const char *what) {
		why = std::string("duplicate marking: ") + what + ": " + hipGetErrorString(err);
		return -1;
	};
	*st = GdmStats();
	if (n == 0) return 0;
	uint64_t *d_key;
	uint32_t *d_score, *d_idx, *d_bitmap, *d_st, h_st[4] = {0, 0, 0, 0};
	if ((e = mem.alloc(&d_key, 8 * n)) != hipSuccess || (e = mem.alloc(&d_score, 4 * n)) != hipSuccess || (e = mem.alloc(&d_idx, 4 * n)) != hipSuccess) return fail(e, "entries");
	if ((e = mem.alloc(&d_bitmap, 4 * (size_t)((n + 31) / 32) + 16)) != hipSuccess) return fail(e, "bitmap");
	int rc = gd_dup_keys_dev(ctx, mem, d_recs, len, d_start, d_rows, n, d_key, d_score, d_idx, why);
	if (rc) return rc;
	if (gd_dup_decide_dev(ctx, mem, d_key, d_score, d_idx, n, d_bitmap, &d_st, why)) return -1;
	hipLaunchKernelGGL(dup_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_recs, len, d_start, d_rows, n, (const uint32_t *)d_bitmap, 0u);
	if ((e = hipGetLastError()) != hipSuccess) return fail(e, "apply launch");
	if ((e = hipMemcpyAsync(h_st, d_st, 16, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "counters copy down");
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "kernels");
	gd_dup_stats(h_st, n, st);
	return 0;
}

static void gd_dup_stats_out(const GdmStats &s, gdiet_dup_stats_t *o)
{
	if (o) o->examined = s.examined, o->eligible = s.eligible, o->duplicates = s.duplicates, o->max_group = s.max_group;
}

extern "C" int64_t gdiet_hip_bam_markdup_records(gdiet_ctx *ctx, const void *recs, size_t len, void *out, gdiet_dup_stats_t *dup_stats)
{
	if (!ctx || (!recs && len) || (!out && len)) return GDIET_E_PARAM;
	gd_err_clear();
	auto fail = [&](int rc, const std::string &what) { return (int64_t)gd_err_fail(ctx, rc, "gdiet_hip_bam_markdup_records: " + what); };
	GdmStats st;
	gd_dup_stats_out(st, dup_stats);
	if (len >= ((size_t)1 << 31)) return fail(GDIET_E_PARAM, "2 GiB of records or more");
	std::vector<uint64_t> start;
	std::string why;
	if (gd_record_starts(recs, len, start, why)) return fail(GDIET_E_PARAM, why);
	const size_t n = start.size();
	if (n == 0) return 0;
	GdLane &L = ctx->bsort;
	std::lock_guard<std::mutex> lk(L.mu);
	if (L.ready(ctx->device, 3, "duplicate marking", why)) return fail(GDIET_E_HIP, why);
	hipStream_t s = L.stream;
	hipError_t e = hipSuccess;
	GdStreamMem mem(s);
	uint8_t *d_in;
	uint64_t *d_start;
	auto hip_fail = [&](hipError_t err, const char *what) {
		mem.fail();
		return fail(GDIET_E_HIP, std::string("duplicate marking: ") + what + ": " + hipGetErrorString(err));
	};
	if ((e = mem.alloc(&d_in, len + 16)) != hipSuccess) return hip_fail(e, "records");
	if ((e = mem.alloc(&d_start, 8 * n)) != hipSuccess) return hip_fail(e, "starts");
	if ((e = hipMemcpyAsync(d_in, recs, len, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e, "records copy");
	if ((e = hipMemcpyAsync(d_start, start.data(), 8 * n, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e, "starts copy");
	const int rc = gd_dup_mark_dev(ctx, mem, d_in, len, d_start, nullptr, n, &st, why);
	if (rc) { mem.fail(); return fail(rc == -2 ? GDIET_E_PARAM : GDIET_E_HIP, why); }
	if ((e = hipMemcpyAsync(out, d_in, len, hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(e, "records copy down");
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(e, "records copy down");
	gd_dup_stats_out(st, dup_stats);
	return (int64_t)len;
}
