// Driver of the coverage accumulator (cov.hip.h) and its entry points gdiet_hip_cov_*.  Included by gdiet_hip.hip behind bam_driver.hip.h,
// which brings accum_driver.hip.h: the routes on which records arrive, the lock order and everything the accumulators share are there.
//
// Coverage's own: the difference array (4 bytes per reference base) and one small table -- the contigs' bases and lengths, the counters,
// the cell of the first bad record; the scan and the window reduction of finish; the readers.
#pragma once
#include <hipcub/hipcub.hpp>
#include "cov.hip.h"

enum { GDC_DEFAULT_WINDOW = 65536 };
static const uint64_t GDC_DEFAULT_CHUNK = 1ull << 28, GDC_MAX_CHUNK = 1ull << 30;

struct gdiet_coverage : GdAccum {
	gdiet_coverage() : GdAccum("coverage") {}
	uint32_t n_ref = 0, window = 0, win_eff = GDC_DEFAULT_WINDOW;
	uint64_t total = 0, n_win = 0;
	std::vector<uint32_t> clen;
	std::vector<uint64_t> base, wbase; // n_ref + 1 each
	int32_t *d_diff = nullptr;
	uint64_t *d_tab = nullptr; // base | contig counters | summary | first bad | wbase | lengths
	GdcDev D;
	std::vector<gdiet_cov_contig_t> contigs;
	gdiet_cov_summary_t summary;
	std::vector<uint32_t> win_cov;
	std::vector<uint64_t> win_sum;
	const uint64_t *d_wbase() const { return d_tab + (n_ref + 1) + (uint64_t)GDC_N_CONTIG * n_ref + GDC_N_SUMMARY + 1; }
	void launch(hipStream_t s, const uint8_t *d_recs, uint64_t bytes, const uint64_t *d_start, uint64_t n, unsigned blocks) override
	{
		hipLaunchKernelGGL(cov_scatter_kernel, dim3(blocks), dim3(256), 0, s, d_recs, bytes, d_start, n, D);
	}
	void free_arrays() override
	{
		if (d_diff) (void)hipFree(d_diff);
		if (d_tab) (void)hipFree(d_tab);
		d_diff = nullptr, d_tab = nullptr;
	}
};
static_assert(sizeof(gdiet_cov_contig_t) == 8 * GDC_N_CONTIG && sizeof(gdiet_cov_summary_t) == 8 * GDC_N_SUMMARY, "the counters are the structs of the header");

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
		gd_accum_free(h);
		const int code = gd_accum_fail(h, rc, who, what);
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
	h->d_first_bad = D.first_bad;
	gd_accum_register(ctx, h);
	*out = h;
	return GDIET_OK;
}

extern "C" int gdiet_hip_cov_add_bam(gdiet_coverage *h, const void *recs, size_t len) { return gd_accum_add_bam(h, "gdiet_hip_cov_add_bam", recs, len); }
extern "C" int gdiet_hip_cov_add(gdiet_coverage *h, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs, const char *const *quals,
                                 const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs, const char *const *comments, int64_t opt_flag)
{
	return gd_accum_add(h, "gdiet_hip_cov_add", ix, n_reads, qnames, seqs, quals, lens, n_regs, regs, comments, opt_flag);
}
extern "C" int gdiet_hip_cov_close(gdiet_coverage *h) { return gd_accum_close(h); }
extern "C" int gdiet_hip_bgzf_out_set_coverage(gdiet_bgzf_out *w, gdiet_coverage *cov)
{
	return w ? gd_accum_attach(w->ctx, w->acc, GD_ACC_COV, cov, "gdiet_hip_bgzf_out_set_coverage", "writer") : GDIET_E_PARAM;
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
		if (gd_accum_usable(h, why)) return gd_accum_fail(h, GDIET_E_PARAM, who, why);
		const int rc = gd_cov_finish_device(h, chunk, why);
		if (rc) { h->poisoned = true; return gd_accum_fail(h, rc, who, why); }
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
	if (!h->finished) return gd_accum_fail(h, GDIET_E_PARAM, who, "coverage: not finished");
	if (!h->window) return gd_accum_fail(h, GDIET_E_PARAM, who, "coverage: opened without a window");
	if (rid >= h->n_ref) return gd_accum_fail(h, GDIET_E_PARAM, who, "coverage: rid " + std::to_string(rid) + " of " + std::to_string(h->n_ref) + " contigs");
	const uint64_t w0 = h->wbase[rid], n = h->wbase[rid + 1] - w0;
	if (!cov_bases_out && !sum_depth_out) return (int64_t)n; // the size first
	if (cap < n) return gd_accum_fail(h, GDIET_E_PARAM, who, "coverage: " + std::to_string(n) + " windows, room for " + std::to_string(cap));
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
	if (!h->finished) return gd_accum_fail(h, GDIET_E_PARAM, who, "coverage: not finished");
	if (!h->ctx || !h->d_diff) return gd_accum_fail(h, GDIET_E_PARAM, who, "coverage: the context has been destroyed");
	if (rid >= h->n_ref || beg > end || end > h->clen[rid]) return gd_accum_fail(h, GDIET_E_PARAM, who, "coverage: the interval lies outside the contig");
	if (beg == end) return GDIET_OK;
	if (!out) return GDIET_E_PARAM;
	GdLane &L = h->ctx->cov;
	std::lock_guard<std::mutex> lk(L.mu);
	std::string why;
	if (L.ready(h->ctx->device, 0, "coverage", why)) return gd_accum_fail(h, GDIET_E_HIP, who, why);
	hipError_t e = hipMemcpyAsync(out, h->d_diff + h->base[rid] + beg, 4 * (size_t)(end - beg), hipMemcpyDeviceToHost, L.stream);
	if (e == hipSuccess) e = hipStreamSynchronize(L.stream);
	return e == hipSuccess ? GDIET_OK : gd_accum_fail(h, GDIET_E_HIP, who, std::string("coverage: depth copy down: ") + hipGetErrorString(e));
}
