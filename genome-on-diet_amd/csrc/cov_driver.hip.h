// Driver of the coverage accumulator (cov.hip.h) and its entry points gdiet_hip_cov_*.  Included by gdiet_hip.hip behind bam_driver.hip.h
// (needs gdiet_ctx, gdiet_index, GdLane, GdStreamMem, err_mark.h, the BAM flattening and the encoder's driver).
//
// The accumulator owns the difference array (plain hipMalloc: it lives as long as the handle, 4 bytes per reference base) and one small
// table: the contigs' bases and lengths, the counters, the cell of the first bad record.  Records reach it on three routes, which end
// in the same kernel on whatever stream holds the records:
//   gdiet_hip_cov_add_bam   host records: a walk for the starts, upload, scatter; on the lane gdiet_ctx::cov
//   gdiet_hip_cov_add       a mapped batch: flattened and encoded by the BAM encoder's driver, scattered from the resident records on the
//                           encoder's lane; nothing comes down
//   attached                gdiet_hip_bgzf_out_write_bam and the sorter's append call gd_cov_enqueue on the records they have just
//                           encoded, on the encoder's lane, before the records are compressed or sorted; the starts are GdbRec::out
// Every route synchronises its stream before it returns, so finish (on the lane cov) needs no event.  One producer at a time:
// gdiet_coverage::mu is held from the enqueue to the verdict.  Lock order: bam.mu, then the accumulator's, then cov.mu of the context.
#pragma once
#include <hipcub/hipcub.hpp>
#include "cov.hip.h"
#include "bam_flatten.h"

enum { GDC_DEFAULT_WINDOW = 65536, GDC_MAX_BLOCKS = 8192 };
static const uint64_t GDC_DEFAULT_CHUNK = 1ull << 28, GDC_MAX_CHUNK = 1ull << 30;

struct gdiet_coverage {
	std::mutex mu;
	gdiet_ctx *ctx = nullptr; // NULL once the context has been destroyed: the arrays went with it
	uint32_t n_ref = 0, window = 0, win_eff = GDC_DEFAULT_WINDOW;
	uint64_t total = 0, n_win = 0;
	std::vector<uint32_t> clen;
	std::vector<uint64_t> base, wbase; // n_ref + 1 each
	int32_t *d_diff = nullptr;
	uint64_t *d_tab = nullptr; // base | contig counters | summary | first bad | wbase | lengths
	GdcDev D;
	uint64_t h_first_bad = ~(uint64_t)0;
	bool poisoned = false, finished = false;
	std::vector<gdiet_cov_contig_t> contigs;
	gdiet_cov_summary_t summary;
	std::vector<uint32_t> win_cov;
	std::vector<uint64_t> win_sum;
	const uint64_t *d_wbase() const { return d_tab + (n_ref + 1) + (uint64_t)GDC_N_CONTIG * n_ref + GDC_N_SUMMARY + 1; }
};
static_assert(sizeof(gdiet_cov_contig_t) == 8 * GDC_N_CONTIG && sizeof(gdiet_cov_summary_t) == 8 * GDC_N_SUMMARY, "the counters are the structs of the header");

static int gd_cov_fail(gdiet_coverage *h, int rc, const char *who, const std::string &what) { return gd_err_fail(h ? h->ctx : nullptr, rc, std::string(who) + ": " + what); }

// 0, or -1 with why: the accumulator takes no more records
static int gd_cov_usable(gdiet_coverage *h, std::string &why)
{
	if (!h->ctx || !h->d_diff) { why = "coverage: the context has been destroyed"; return -1; }
	if (h->poisoned) { why = "coverage: used after a bad record"; return -1; }
	if (h->finished) { why = "coverage: finished, the accumulator is read-only"; return -1; }
	return 0;
}

// The starts of the host records recs[0, len) of an add_bam call (coverage's and the pileup's): nothing but block_size is looked at here,
// the kernel validates the rest.  0, or -1 with why: nothing was seen
static int gd_record_starts(const void *recs, size_t len, std::vector<uint64_t> &start, std::string &why)
{
	const uint8_t *b = (const uint8_t *)recs;
	size_t pos = 0;
	while (len - pos >= 4) {
		const int32_t bs = (int32_t)gds_le32(b + pos);
		if (bs < 32) {
			why = "BAM record " + std::to_string(start.size()) + " at offset " + std::to_string(pos) + ": a block_size of " + std::to_string(bs) + ", below the 32 fixed bytes";
			return -1;
		}
		if (len - pos - 4 < (size_t)bs) break;
		start.push_back(pos);
		pos += 4 + (size_t)bs;
	}
	if (pos != len) { why = "offset " + std::to_string(pos) + ": the range ends inside a record"; return -1; }
	if (start.size() > 0x7fffffffull) { why = "2^31 records or more in one call"; return -1; }
	return 0;
}

// The scatter of the n records at d_recs[0, bytes) whose starts are h_start[0, n), enqueued on s with the allocations of mem; the caller
// holds h->mu, keeps h_start alive until it has synchronised s, and then asks gd_cov_verdict.  0, or -1 with why (the device failed).
static int gd_cov_enqueue(gdiet_coverage *h, hipStream_t s, GdStreamMem &mem, const uint8_t *d_recs, uint64_t bytes, const uint64_t *h_start, uint64_t n, std::string &why)
{
	hipError_t e = hipSuccess;
	auto fail = [&](hipError_t err, const char *what) {
		why = std::string("coverage: ") + what + ": " + hipGetErrorString(err);
		return -1;
	};
	h->h_first_bad = ~(uint64_t)0;
	if (n == 0) return 0;
	uint64_t *d_start;
	if ((e = mem.alloc(&d_start, 8 * (size_t)n + 16)) != hipSuccess) return fail(e, "starts");
	if ((e = hipMemcpyAsync(d_start, h_start, 8 * (size_t)n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "starts copy");
	if ((e = hipMemsetAsync(h->D.first_bad, 0xff, 8, s)) != hipSuccess) return fail(e, "cell");
	const uint64_t blocks = std::min<uint64_t>((n + 3) / 4, GDC_MAX_BLOCKS);
	hipLaunchKernelGGL(cov_scatter_kernel, dim3((unsigned)blocks), dim3(256), 0, s, d_recs, bytes, (const uint64_t *)d_start, n, h->D);
	if ((e = hipGetLastError()) != hipSuccess) return fail(e, "scatter launch");
	if ((e = hipMemcpyAsync(&h->h_first_bad, h->D.first_bad, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "cell copy down");
	return 0;
}
// after the stream has been synchronised: 0, or GDIET_E_PARAM with why naming the call's first bad record (the accumulator is poisoned)
static int gd_cov_verdict(gdiet_coverage *h, std::string &why)
{
	if (h->h_first_bad == ~(uint64_t)0) return 0;
	h->poisoned = true;
	why = "coverage: record " + std::to_string(h->h_first_bad >> 8) + " of the call: " + gdc_reason_text((uint32_t)(h->h_first_bad & 0xff));
	h->h_first_bad = ~(uint64_t)0;
	return GDIET_E_PARAM;
}

// ---- the attached routes (declared in bam_driver.hip.h) -------------------------------------------------------------------------------
static int gd_cov_hold(gdiet_coverage *h, std::string &why)
{
	h->mu.lock();
	if (gd_cov_usable(h, why)) { h->mu.unlock(); return -1; }
	return 0;
}
static void gd_cov_release(gdiet_coverage *h) { h->mu.unlock(); }
// the records of P, encoded at d_recs[0, P.bytes): their starts are GdbRec::out, so nothing is walked
static int gd_cov_enqueue_part(gdiet_coverage *h, hipStream_t s, const uint8_t *d_recs, const GdbPart &P, std::vector<uint64_t> &starts, std::string &why)
{
	starts.resize(P.rec.size());
	for (size_t k = 0; k < P.rec.size(); ++k) starts[k] = P.rec[k].out;
	GdStreamMem mem(s); // (the table is freed behind the kernel, in stream order)
	return gd_cov_enqueue(h, s, mem, d_recs, P.bytes, starts.data(), starts.size(), why);
}
extern "C" int gdiet_hip_bgzf_out_set_coverage(gdiet_bgzf_out *w, gdiet_coverage *cov)
{
	if (!w) return GDIET_E_PARAM;
	gd_err_clear();
	if (cov && (!w->ctx || cov->ctx != w->ctx)) return gd_err_fail(w->ctx, GDIET_E_PARAM, "gdiet_hip_bgzf_out_set_coverage: the writer and the accumulator need one context");
	w->cov = cov;
	return GDIET_OK;
}

static void gd_cov_free_arrays(gdiet_coverage *h) // the caller holds h->mu
{
	if (h->d_diff) (void)hipFree(h->d_diff);
	if (h->d_tab) (void)hipFree(h->d_tab);
	h->d_diff = nullptr, h->d_tab = nullptr;
}
// gdiet_hip_destroy: the arrays of the accumulators still open go with the context; their handles take nothing but close from then on
static void gd_cov_orphan_all(gdiet_ctx *ctx)
{
	std::vector<void *> open;
	{
		std::lock_guard<std::mutex> lk(ctx->cov_reg_mu);
		open.swap(ctx->cov_open);
	}
	for (void *p : open) {
		gdiet_coverage *h = (gdiet_coverage *)p;
		std::lock_guard<std::mutex> lk(h->mu);
		gd_cov_free_arrays(h);
		h->ctx = nullptr;
	}
}

extern "C" int gdiet_hip_cov_open(gdiet_ctx *ctx, const gdiet_index *ix, uint32_t excl_flags, uint32_t min_mapq, uint32_t window, gdiet_coverage **out)
{
	if (!ctx || !ix || !out) return GDIET_E_PARAM;
	*out = nullptr;
	gd_err_clear();
	const char *who = "gdiet_hip_cov_open";
	gdiet_coverage *h = new gdiet_coverage();
	h->ctx = ctx, h->window = window, h->win_eff = window ? window : (uint32_t)GDC_DEFAULT_WINDOW;
	const size_t n_ref = ix->h.seq.size();
	h->n_ref = (uint32_t)n_ref;
	h->clen.resize(n_ref), h->base.assign(n_ref + 1, 0), h->wbase.assign(n_ref + 1, 0);
	for (size_t i = 0; i < n_ref; ++i) {
		h->clen[i] = ix->h.seq[i].len;
		h->base[i + 1] = h->base[i] + h->clen[i], h->wbase[i + 1] = h->wbase[i] + ((uint64_t)h->clen[i] + h->win_eff - 1) / h->win_eff;
	}
	h->total = h->base[n_ref], h->n_win = h->wbase[n_ref];
	auto refuse = [&](int rc, const std::string &what) {
		gd_cov_free_arrays(h);
		const int code = gd_cov_fail(h, rc, who, what);
		delete h;
		return code;
	};
	if (n_ref == 0 || n_ref > 0x7fffffffull) return refuse(GDIET_E_PARAM, "an index without contigs");
	(void)hipSetDevice(ctx->device);
	const size_t bytes = 4 * ((size_t)h->total + 1);
	hipError_t e = hipMalloc((void **)&h->d_diff, bytes);
	if (e != hipSuccess) {
		h->d_diff = nullptr;
		(void)hipGetLastError();
		return refuse(GDIET_E_NOMEM, "the difference array of " + std::to_string(h->total) + " reference bases takes " + std::to_string(bytes) + " bytes (4 per base): " + hipGetErrorString(e));
	}
	const size_t words = 2 * (n_ref + 1) + (size_t)GDC_N_CONTIG * n_ref + GDC_N_SUMMARY + 1, tab_bytes = 8 * words + 4 * n_ref;
	if ((e = hipMalloc((void **)&h->d_tab, tab_bytes)) != hipSuccess) {
		h->d_tab = nullptr;
		(void)hipGetLastError();
		return refuse(GDIET_E_NOMEM, "the counters take " + std::to_string(tab_bytes) + " bytes: " + hipGetErrorString(e));
	}
	GdcDev &D = h->D;
	D.diff = h->d_diff, D.base = h->d_tab, D.contig = h->d_tab + (n_ref + 1), D.summary = D.contig + (size_t)GDC_N_CONTIG * n_ref, D.first_bad = D.summary + GDC_N_SUMMARY;
	D.clen = (const uint32_t *)(h->d_tab + words);
	D.n_ref = h->n_ref, D.excl_flags = excl_flags, D.min_mapq = min_mapq;
	GdLane &L = ctx->cov;
	std::lock_guard<std::mutex> lk(L.mu);
	std::string why;
	if (L.ready(ctx->device, 0, "coverage", why)) return refuse(GDIET_E_HIP, why);
	hipStream_t s = L.stream;
	if ((e = hipMemsetAsync(h->d_diff, 0, bytes, s)) != hipSuccess || (e = hipMemsetAsync(h->d_tab, 0, tab_bytes, s)) != hipSuccess ||
	    (e = hipMemcpyAsync(h->d_tab, h->base.data(), 8 * (n_ref + 1), hipMemcpyHostToDevice, s)) != hipSuccess ||
	    (e = hipMemcpyAsync((void *)h->d_wbase(), h->wbase.data(), 8 * (n_ref + 1), hipMemcpyHostToDevice, s)) != hipSuccess ||
	    (e = hipMemcpyAsync((void *)D.clen, h->clen.data(), 4 * n_ref, hipMemcpyHostToDevice, s)) != hipSuccess || (e = hipStreamSynchronize(s)) != hipSuccess) {
		(void)hipStreamSynchronize(s);
		return refuse(GDIET_E_HIP, std::string("coverage: clearing the arrays: ") + hipGetErrorString(e));
	}
	{
		std::lock_guard<std::mutex> rk(ctx->cov_reg_mu);
		ctx->cov_open.push_back(h);
	}
	*out = h;
	return GDIET_OK;
}

extern "C" int gdiet_hip_cov_add_bam(gdiet_coverage *h, const void *recs, size_t len)
{
	if (!h || (!recs && len)) return GDIET_E_PARAM;
	gd_err_clear();
	const char *who = "gdiet_hip_cov_add_bam";
	std::lock_guard<std::mutex> hk(h->mu);
	std::string why;
	if (gd_cov_usable(h, why)) return gd_cov_fail(h, GDIET_E_PARAM, who, why);
	std::vector<uint64_t> start;
	if (gd_record_starts(recs, len, start, why)) return gd_cov_fail(h, GDIET_E_PARAM, who, why);
	if (start.empty()) return GDIET_OK;
	gdiet_ctx *ctx = h->ctx;
	GdLane &L = ctx->cov;
	std::lock_guard<std::mutex> lk(L.mu);
	if (L.ready(ctx->device, 0, "coverage", why)) return gd_cov_fail(h, GDIET_E_HIP, who, why);
	hipStream_t s = L.stream;
	GdStreamMem mem(s);
	uint8_t *d_in;
	hipError_t e = hipSuccess;
	auto hip_fail = [&](hipError_t err, const char *what) {
		mem.fail();
		return gd_cov_fail(h, GDIET_E_HIP, who, std::string("coverage: ") + what + ": " + hipGetErrorString(err));
	};
	if ((e = mem.alloc(&d_in, len + 16)) != hipSuccess) return hip_fail(e, "records");
	if ((e = hipMemcpyAsync(d_in, recs, len, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e, "records copy");
	if (gd_cov_enqueue(h, s, mem, d_in, len, start.data(), start.size(), why)) { mem.fail(); return gd_cov_fail(h, GDIET_E_HIP, who, why); }
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(e, "scatter kernel");
	const int rc = gd_cov_verdict(h, why);
	return rc ? gd_cov_fail(h, rc, who, why) : GDIET_OK;
}

extern "C" int gdiet_hip_cov_add(gdiet_coverage *h, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs, const char *const *quals,
                                 const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs, const char *const *comments, int64_t opt_flag)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	const char *who = "gdiet_hip_cov_add";
	gdiet_ctx *ctx;
	{
		std::lock_guard<std::mutex> hk(h->mu);
		ctx = h->ctx;
	}
	if (!ctx) return gd_cov_fail(h, GDIET_E_PARAM, who, "coverage: the context has been destroyed");
	if (!gd_bam_args_ok(ctx, ix, n_reads, qnames, seqs, lens, n_regs, regs)) return GDIET_E_PARAM;
	std::lock_guard<std::mutex> lk(ctx->bam.mu);
	std::lock_guard<std::mutex> hk(h->mu);
	std::string why;
	if (gd_cov_usable(h, why)) return gd_cov_fail(h, GDIET_E_PARAM, who, why);
	GdbPart &P = gd_bam_pool(ctx).all;
	int rc = gd_bam_flatten(ctx, ix, n_reads, qnames, seqs, quals, comments, lens, n_regs, regs, opt_flag, P, why);
	if (rc) return why.empty() ? rc : gd_cov_fail(h, rc, who, why);
	if (P.bytes == 0) return GDIET_OK;
	std::vector<uint64_t> starts;
	rc = gd_bam_encode_device(ctx, P, nullptr, 0, why, [&](uint8_t *d_stream, size_t, hipStream_t s) { // (the stream is synchronised when this has returned)
		return gd_cov_enqueue_part(h, s, d_stream, P, starts, why);
	});
	if (rc) return gd_cov_fail(h, GDIET_E_HIP, who, why);
	rc = gd_cov_verdict(h, why);
	return rc ? gd_cov_fail(h, rc, who, why) : GDIET_OK;
}

// the inclusive sum in chunks, the window reduction, the counters: once; the caller holds h->mu.  0 or a GDIET_E_* code with why
static int gd_cov_finish_device(gdiet_coverage *h, uint64_t chunk, std::string &why)
{
	gdiet_ctx *ctx = h->ctx;
	GdLane &L = ctx->cov;
	std::lock_guard<std::mutex> lk(L.mu);
	if (L.ready(ctx->device, 0, "coverage", why)) return GDIET_E_HIP;
	hipStream_t s = L.stream;
	GdStreamMem mem(s);
	hipError_t e = hipSuccess;
	auto fail = [&](hipError_t err, const char *what) {
		mem.fail();
		why = std::string("coverage: ") + what + ": " + hipGetErrorString(err);
		return (int)GDIET_E_HIP;
	};
	const uint64_t slots = h->total + 1;
	chunk = std::min<uint64_t>(std::min<uint64_t>(chunk ? chunk : GDC_DEFAULT_CHUNK, GDC_MAX_CHUNK), slots);
	size_t tmp_bytes = 0;
	void *d_tmp;
	if ((e = hipcub::DeviceScan::InclusiveSum(nullptr, tmp_bytes, h->d_diff, h->d_diff, (int)chunk, s)) != hipSuccess) return fail(e, "scan size");
	if ((e = mem.alloc((uint8_t **)&d_tmp, std::max<size_t>(tmp_bytes, 16))) != hipSuccess) return fail(e, "scan scratch");
	for (uint64_t c0 = 0; c0 < slots; c0 += chunk) {
		const uint64_t m = std::min<uint64_t>(chunk, slots - c0);
		if (c0) {
			hipLaunchKernelGGL(cov_carry_kernel, dim3(1), dim3(64), 0, s, h->d_diff, c0);
			if ((e = hipGetLastError()) != hipSuccess) return fail(e, "carry launch");
		}
		size_t tb = tmp_bytes;
		if ((e = hipcub::DeviceScan::InclusiveSum(d_tmp, tb, h->d_diff + c0, h->d_diff + c0, (int)m, s)) != hipSuccess) return fail(e, "scan");
	}
	uint32_t *d_cov;
	uint64_t *d_sum;
	h->win_cov.assign((size_t)h->n_win, 0), h->win_sum.assign((size_t)h->n_win, 0);
	std::vector<uint64_t> tab((size_t)GDC_N_CONTIG * h->n_ref + GDC_N_SUMMARY);
	if (h->n_win) {
		if ((e = mem.alloc(&d_cov, 4 * (size_t)h->n_win + 16)) != hipSuccess || (e = mem.alloc(&d_sum, 8 * (size_t)h->n_win + 16)) != hipSuccess) return fail(e, "window tables");
		const uint64_t blocks = std::min<uint64_t>((h->n_win + 3) / 4, GDC_MAX_BLOCKS);
		hipLaunchKernelGGL(cov_window_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const uint32_t *)h->d_diff, h->D.base, h->d_wbase(), h->n_ref, h->win_eff, h->n_win, d_cov, d_sum);
		if ((e = hipGetLastError()) != hipSuccess) return fail(e, "window launch");
		if ((e = hipMemcpyAsync(h->win_cov.data(), d_cov, 4 * (size_t)h->n_win, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "window copy down");
		if ((e = hipMemcpyAsync(h->win_sum.data(), d_sum, 8 * (size_t)h->n_win, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "window copy down");
	}
	if ((e = hipMemcpyAsync(tab.data(), h->D.contig, 8 * tab.size(), hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "counters copy down");
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "scan and windows");
	h->contigs.resize(h->n_ref);
	for (uint32_t r = 0; r < h->n_ref; ++r) {
		memcpy(&h->contigs[r], tab.data() + (size_t)GDC_N_CONTIG * r, sizeof(gdiet_cov_contig_t));
		uint64_t cov = 0;
		for (uint64_t w = h->wbase[r]; w < h->wbase[r + 1]; ++w) cov += h->win_cov[(size_t)w];
		h->contigs[r].cov_bases = cov;
	}
	memcpy(&h->summary, tab.data() + (size_t)GDC_N_CONTIG * h->n_ref, sizeof(gdiet_cov_summary_t));
	h->finished = true;
	return 0;
}

extern "C" int gdiet_hip_cov_finish_chunked(gdiet_coverage *h, uint64_t chunk, gdiet_cov_contig_t *contigs_out, gdiet_cov_summary_t *summary_out)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	const char *who = "gdiet_hip_cov_finish";
	std::lock_guard<std::mutex> hk(h->mu);
	std::string why;
	if (!h->finished) {
		if (gd_cov_usable(h, why)) return gd_cov_fail(h, GDIET_E_PARAM, who, why);
		const int rc = gd_cov_finish_device(h, chunk, why);
		if (rc) { h->poisoned = true; return gd_cov_fail(h, rc, who, why); }
	}
	if (contigs_out) memcpy(contigs_out, h->contigs.data(), sizeof(gdiet_cov_contig_t) * h->n_ref);
	if (summary_out) *summary_out = h->summary;
	return GDIET_OK;
}
extern "C" int gdiet_hip_cov_finish(gdiet_coverage *h, gdiet_cov_contig_t *contigs_out, gdiet_cov_summary_t *summary_out)
{
	return gdiet_hip_cov_finish_chunked(h, 0, contigs_out, summary_out);
}

extern "C" int64_t gdiet_hip_cov_windows(gdiet_coverage *h, uint32_t rid, uint32_t *cov_bases_out, uint64_t *sum_depth_out, size_t cap)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	const char *who = "gdiet_hip_cov_windows";
	std::lock_guard<std::mutex> hk(h->mu);
	if (!h->finished) return gd_cov_fail(h, GDIET_E_PARAM, who, "coverage: not finished");
	if (!h->window) return gd_cov_fail(h, GDIET_E_PARAM, who, "coverage: opened without a window");
	if (rid >= h->n_ref) return gd_cov_fail(h, GDIET_E_PARAM, who, "coverage: rid " + std::to_string(rid) + " of " + std::to_string(h->n_ref) + " contigs");
	const uint64_t w0 = h->wbase[rid], n = h->wbase[rid + 1] - w0;
	if (!cov_bases_out && !sum_depth_out) return (int64_t)n; // the size first
	if (cap < n) return gd_cov_fail(h, GDIET_E_PARAM, who, "coverage: " + std::to_string(n) + " windows, room for " + std::to_string(cap));
	if (cov_bases_out && n) memcpy(cov_bases_out, h->win_cov.data() + w0, 4 * (size_t)n);
	if (sum_depth_out && n) memcpy(sum_depth_out, h->win_sum.data() + w0, 8 * (size_t)n);
	return (int64_t)n;
}

extern "C" int gdiet_hip_cov_depth(gdiet_coverage *h, uint32_t rid, uint32_t beg, uint32_t end, uint32_t *out)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	const char *who = "gdiet_hip_cov_depth";
	std::lock_guard<std::mutex> hk(h->mu);
	if (!h->finished) return gd_cov_fail(h, GDIET_E_PARAM, who, "coverage: not finished");
	if (!h->ctx || !h->d_diff) return gd_cov_fail(h, GDIET_E_PARAM, who, "coverage: the context has been destroyed");
	if (rid >= h->n_ref || beg > end || end > h->clen[rid]) return gd_cov_fail(h, GDIET_E_PARAM, who, "coverage: the interval lies outside the contig");
	if (beg == end) return GDIET_OK;
	if (!out) return GDIET_E_PARAM;
	GdLane &L = h->ctx->cov;
	std::lock_guard<std::mutex> lk(L.mu);
	std::string why;
	if (L.ready(h->ctx->device, 0, "coverage", why)) return gd_cov_fail(h, GDIET_E_HIP, who, why);
	hipError_t e = hipMemcpyAsync(out, h->d_diff + h->base[rid] + beg, 4 * (size_t)(end - beg), hipMemcpyDeviceToHost, L.stream);
	if (e == hipSuccess) e = hipStreamSynchronize(L.stream);
	return e == hipSuccess ? GDIET_OK : gd_cov_fail(h, GDIET_E_HIP, who, std::string("coverage: depth copy down: ") + hipGetErrorString(e));
}

extern "C" int gdiet_hip_cov_close(gdiet_coverage *h)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	{
		std::lock_guard<std::mutex> hk(h->mu);
		if (h->ctx) {
			(void)hipSetDevice(h->ctx->device);
			std::lock_guard<std::mutex> rk(h->ctx->cov_reg_mu);
			auto &v = h->ctx->cov_open;
			v.erase(std::remove(v.begin(), v.end(), (void *)h), v.end());
		}
		gd_cov_free_arrays(h);
	}
	delete h;
	return GDIET_OK;
}
