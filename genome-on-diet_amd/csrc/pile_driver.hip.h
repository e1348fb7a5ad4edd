// Driver of the pileup accumulator (pile.hip.h) and its entry points gdiet_hip_pile_*.  Included by gdiet_hip.hip behind
// cov_driver.hip.h, whose shape it has.
//
// The accumulator owns the counters (plain hipMalloc: 32 bytes per position of the regions, for as long as the handle lives) and one
// small table: the regions, the contigs' lengths, the summary, the cell of the first bad record.  Records reach it on coverage's three
// routes (gdiet_hip_pile_add_bam on the lane gdiet_ctx::cov; gdiet_hip_pile_add and the attached writer / sorter on the encoder's lane),
// which end in pile_scatter_kernel on whatever stream holds the records.  Every route synchronises its stream before it returns, so
// finish and the calls (on the lane cov) need no event.  One producer at a time: gdiet_pileup::mu is held from the enqueue to the
// verdict.  Lock order: bam.mu, then the coverage accumulator's, then the pileup accumulator's, then cov.mu of the context.
#pragma once
#include <hipcub/hipcub.hpp>
#include "pile.hip.h"
#include "bam_flatten.h"

static const uint64_t GDP_DEFAULT_CHUNK = 1ull << 24, GDP_MAX_CHUNK = 1ull << 30;

struct gdiet_pileup {
	std::mutex mu;
	gdiet_ctx *ctx = nullptr; // NULL once the context has been destroyed: the arrays went with it
	const gdiet_index *ix = nullptr;
	uint32_t n_ref = 0;
	uint64_t total = 0, chunk = GDP_DEFAULT_CHUNK;
	std::vector<uint32_t> clen;
	std::vector<GdpRegion> regs;
	uint32_t *d_cnt = nullptr;
	uint64_t *d_tab = nullptr; // summary | first bad | regions | lengths
	GdpDev D;
	uint64_t h_first_bad = ~(uint64_t)0;
	bool poisoned = false, finished = false;
	gdiet_pile_summary_t summary;
};
static_assert(sizeof(gdiet_pile_summary_t) == 8 * GDP_N_SUMMARY && sizeof(gdiet_pile_site_t) == 4 * (5 + GDP_N_CNT) && sizeof(GdpRegion) == 24, "the structs of the header");

static int gd_pile_fail(gdiet_pileup *h, int rc, const char *who, const std::string &what) { return gd_err_fail(h ? h->ctx : nullptr, rc, std::string(who) + ": " + what); }

// 0, or -1 with why: the accumulator takes no more records
static int gd_pile_usable(gdiet_pileup *h, std::string &why)
{
	if (!h->ctx || !h->d_cnt) { why = "pileup: the context has been destroyed"; return -1; }
	if (h->poisoned) { why = "pileup: used after a bad record"; return -1; }
	if (h->finished) { why = "pileup: finished, the accumulator is read-only"; return -1; }
	return 0;
}

// as gd_cov_enqueue: the caller holds h->mu, keeps h_start alive until it has synchronised s, and then asks gd_pile_verdict
static int gd_pile_enqueue(gdiet_pileup *h, hipStream_t s, GdStreamMem &mem, const uint8_t *d_recs, uint64_t bytes, const uint64_t *h_start, uint64_t n, std::string &why)
{
	hipError_t e = hipSuccess;
	auto fail = [&](hipError_t err, const char *what) {
		why = std::string("pileup: ") + what + ": " + hipGetErrorString(err);
		return -1;
	};
	h->h_first_bad = ~(uint64_t)0;
	if (n == 0) return 0;
	uint64_t *d_start;
	if ((e = mem.alloc(&d_start, 8 * (size_t)n + 16)) != hipSuccess) return fail(e, "starts");
	if ((e = hipMemcpyAsync(d_start, h_start, 8 * (size_t)n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "starts copy");
	if ((e = hipMemsetAsync(h->D.first_bad, 0xff, 8, s)) != hipSuccess) return fail(e, "cell");
	const uint64_t blocks = std::min<uint64_t>((n + 3) / 4, GDC_MAX_BLOCKS);
	hipLaunchKernelGGL(pile_scatter_kernel, dim3((unsigned)blocks), dim3(256), 0, s, d_recs, bytes, (const uint64_t *)d_start, n, h->D);
	if ((e = hipGetLastError()) != hipSuccess) return fail(e, "scatter launch");
	if ((e = hipMemcpyAsync(&h->h_first_bad, h->D.first_bad, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "cell copy down");
	return 0;
}
static int gd_pile_verdict(gdiet_pileup *h, std::string &why)
{
	if (h->h_first_bad == ~(uint64_t)0) return 0;
	h->poisoned = true;
	why = "pileup: record " + std::to_string(h->h_first_bad >> 8) + " of the call: " + gdc_reason_text((uint32_t)(h->h_first_bad & 0xff));
	h->h_first_bad = ~(uint64_t)0;
	return GDIET_E_PARAM;
}

// ---- the attached routes (declared in bam_driver.hip.h) -------------------------------------------------------------------------------
static int gd_pile_hold(gdiet_pileup *h, std::string &why)
{
	h->mu.lock();
	if (gd_pile_usable(h, why)) { h->mu.unlock(); return -1; }
	return 0;
}
static void gd_pile_release(gdiet_pileup *h) { h->mu.unlock(); }
static int gd_pile_enqueue_part(gdiet_pileup *h, hipStream_t s, const uint8_t *d_recs, const GdbPart &P, std::vector<uint64_t> &starts, std::string &why)
{
	starts.resize(P.rec.size());
	for (size_t k = 0; k < P.rec.size(); ++k) starts[k] = P.rec[k].out;
	GdStreamMem mem(s); // (the table is freed behind the kernel, in stream order)
	return gd_pile_enqueue(h, s, mem, d_recs, P.bytes, starts.data(), starts.size(), why);
}
extern "C" int gdiet_hip_bgzf_out_set_pileup(gdiet_bgzf_out *w, gdiet_pileup *pile)
{
	if (!w) return GDIET_E_PARAM;
	gd_err_clear();
	if (pile && (!w->ctx || pile->ctx != w->ctx)) return gd_err_fail(w->ctx, GDIET_E_PARAM, "gdiet_hip_bgzf_out_set_pileup: the writer and the accumulator need one context");
	w->pile = pile;
	return GDIET_OK;
}

static void gd_pile_free_arrays(gdiet_pileup *h) // the caller holds h->mu
{
	if (h->d_cnt) (void)hipFree(h->d_cnt);
	if (h->d_tab) (void)hipFree(h->d_tab);
	h->d_cnt = nullptr, h->d_tab = nullptr;
}
// gdiet_hip_destroy: the arrays of the accumulators still open go with the context; their handles take nothing but close from then on
static void gd_pile_orphan_all(gdiet_ctx *ctx)
{
	std::vector<void *> open;
	{
		std::lock_guard<std::mutex> lk(ctx->cov_reg_mu);
		open.swap(ctx->pile_open);
	}
	for (void *p : open) {
		gdiet_pileup *h = (gdiet_pileup *)p;
		std::lock_guard<std::mutex> lk(h->mu);
		gd_pile_free_arrays(h);
		h->ctx = nullptr;
	}
}

extern "C" int gdiet_hip_pile_open(gdiet_ctx *ctx, const gdiet_index *ix, const gdiet_pile_region_t *regions, size_t n_regions, uint32_t excl_flags, uint32_t min_mapq,
                                   uint32_t min_baseq, gdiet_pileup **out)
{
	if (!ctx || !ix || !out || (!regions && n_regions)) return GDIET_E_PARAM;
	*out = nullptr;
	gd_err_clear();
	const char *who = "gdiet_hip_pile_open";
	gdiet_pileup *h = new gdiet_pileup();
	h->ctx = ctx, h->ix = ix;
	const size_t n_ref = ix->h.seq.size();
	h->n_ref = (uint32_t)n_ref;
	h->clen.resize(n_ref);
	for (size_t i = 0; i < n_ref; ++i) h->clen[i] = ix->h.seq[i].len;
	auto refuse = [&](int rc, const std::string &what) {
		gd_pile_free_arrays(h);
		const int code = gd_pile_fail(h, rc, who, what);
		delete h;
		return code;
	};
	if (n_ref == 0 || n_ref > 0x7fffffffull) return refuse(GDIET_E_PARAM, "an index without contigs");
	if (n_regions > 0x7fffffffull) return refuse(GDIET_E_PARAM, "2^31 regions or more");
	auto push = [&](uint32_t rid, uint32_t beg, uint32_t end) {
		GdpRegion R;
		R.off = h->total, R.rid = rid, R.beg = beg, R.end = end, R.pad = 0;
		h->regs.push_back(R), h->total += end - beg;
	};
	for (size_t i = 0; i < n_regions; ++i) {
		const gdiet_pile_region_t &g = regions[i];
		const std::string name = "region " + std::to_string(i) + " (" + std::to_string(g.rid) + ", " + std::to_string(g.beg) + ", " + std::to_string(g.end) + ")";
		if (g.beg >= g.end) return refuse(GDIET_E_PARAM, name + " is empty");
		if (g.rid >= n_ref || g.end > h->clen[g.rid]) return refuse(GDIET_E_PARAM, name + " lies past its contig");
		if (i && (regions[i - 1].rid > g.rid || (regions[i - 1].rid == g.rid && regions[i - 1].beg > g.beg))) return refuse(GDIET_E_PARAM, name + ": the list is not sorted by (rid, beg)");
		if (i && regions[i - 1].rid == g.rid && regions[i - 1].end > g.beg) return refuse(GDIET_E_PARAM, name + " overlaps the region before it");
		push(g.rid, g.beg, g.end);
	}
	if (n_regions == 0)
		for (size_t i = 0; i < n_ref; ++i)
			if (h->clen[i]) push((uint32_t)i, 0, h->clen[i]);
	if (h->regs.empty()) return refuse(GDIET_E_PARAM, "an index without bases");
	(void)hipSetDevice(ctx->device);
	if (gd_index_seq_table(ctx, ix)) return refuse(GDIET_E_HIP, "pileup: the contig table: " + ctx->err);
	const size_t bytes = 4 * (size_t)GDP_N_CNT * (size_t)h->total;
	hipError_t e = hipMalloc((void **)&h->d_cnt, bytes);
	if (e != hipSuccess) {
		h->d_cnt = nullptr;
		(void)hipGetLastError();
		return refuse(GDIET_E_NOMEM, "the counters of " + std::to_string(h->total) + " positions take " + std::to_string(bytes) + " bytes (32 per position): " + hipGetErrorString(e));
	}
	const size_t n_reg = h->regs.size(), words = GDP_N_SUMMARY + 1 + 3 * n_reg, tab_bytes = 8 * words + 4 * n_ref;
	if ((e = hipMalloc((void **)&h->d_tab, tab_bytes)) != hipSuccess) {
		h->d_tab = nullptr;
		(void)hipGetLastError();
		return refuse(GDIET_E_NOMEM, "the tables take " + std::to_string(tab_bytes) + " bytes: " + hipGetErrorString(e));
	}
	GdpDev &D = h->D;
	D.cnt = h->d_cnt, D.summary = h->d_tab, D.first_bad = D.summary + GDP_N_SUMMARY, D.regs = (const GdpRegion *)(D.first_bad + 1), D.clen = (const uint32_t *)(h->d_tab + words);
	D.n_ref = h->n_ref, D.n_reg = (uint32_t)n_reg, D.excl_flags = excl_flags, D.min_mapq = min_mapq, D.min_baseq = min_baseq;
	GdLane &L = ctx->cov;
	std::lock_guard<std::mutex> lk(L.mu);
	std::string why;
	if (L.ready(ctx->device, 0, "coverage", why)) return refuse(GDIET_E_HIP, why);
	hipStream_t s = L.stream;
	if ((e = hipMemsetAsync(h->d_cnt, 0, bytes, s)) != hipSuccess || (e = hipMemsetAsync(h->d_tab, 0, tab_bytes, s)) != hipSuccess ||
	    (e = hipMemcpyAsync((void *)D.regs, h->regs.data(), sizeof(GdpRegion) * n_reg, hipMemcpyHostToDevice, s)) != hipSuccess ||
	    (e = hipMemcpyAsync((void *)D.clen, h->clen.data(), 4 * n_ref, hipMemcpyHostToDevice, s)) != hipSuccess || (e = hipStreamSynchronize(s)) != hipSuccess) {
		(void)hipStreamSynchronize(s);
		return refuse(GDIET_E_HIP, std::string("pileup: clearing the arrays: ") + hipGetErrorString(e));
	}
	{
		std::lock_guard<std::mutex> rk(ctx->cov_reg_mu);
		ctx->pile_open.push_back(h);
	}
	*out = h;
	return GDIET_OK;
}

extern "C" int gdiet_hip_pile_add_bam(gdiet_pileup *h, const void *recs, size_t len)
{
	if (!h || (!recs && len)) return GDIET_E_PARAM;
	gd_err_clear();
	const char *who = "gdiet_hip_pile_add_bam";
	std::lock_guard<std::mutex> hk(h->mu);
	std::string why;
	if (gd_pile_usable(h, why)) return gd_pile_fail(h, GDIET_E_PARAM, who, why);
	std::vector<uint64_t> start;
	if (gd_record_starts(recs, len, start, why)) return gd_pile_fail(h, GDIET_E_PARAM, who, why); // (cov_driver.hip.h)
	if (start.empty()) return GDIET_OK;
	gdiet_ctx *ctx = h->ctx;
	GdLane &L = ctx->cov;
	std::lock_guard<std::mutex> lk(L.mu);
	if (L.ready(ctx->device, 0, "coverage", why)) return gd_pile_fail(h, GDIET_E_HIP, who, why);
	hipStream_t s = L.stream;
	GdStreamMem mem(s);
	uint8_t *d_in;
	hipError_t e = hipSuccess;
	auto hip_fail = [&](hipError_t err, const char *what) {
		mem.fail();
		return gd_pile_fail(h, GDIET_E_HIP, who, std::string("pileup: ") + what + ": " + hipGetErrorString(err));
	};
	if ((e = mem.alloc(&d_in, len + 16)) != hipSuccess) return hip_fail(e, "records");
	if ((e = hipMemcpyAsync(d_in, recs, len, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e, "records copy");
	if (gd_pile_enqueue(h, s, mem, d_in, len, start.data(), start.size(), why)) { mem.fail(); return gd_pile_fail(h, GDIET_E_HIP, who, why); }
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(e, "scatter kernel");
	const int rc = gd_pile_verdict(h, why);
	return rc ? gd_pile_fail(h, rc, who, why) : GDIET_OK;
}

extern "C" int gdiet_hip_pile_add(gdiet_pileup *h, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs, const char *const *quals,
                                  const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs, const char *const *comments, int64_t opt_flag)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	const char *who = "gdiet_hip_pile_add";
	gdiet_ctx *ctx;
	{
		std::lock_guard<std::mutex> hk(h->mu);
		ctx = h->ctx;
	}
	if (!ctx) return gd_pile_fail(h, GDIET_E_PARAM, who, "pileup: the context has been destroyed");
	if (!gd_bam_args_ok(ctx, ix, n_reads, qnames, seqs, lens, n_regs, regs)) return GDIET_E_PARAM;
	std::lock_guard<std::mutex> lk(ctx->bam.mu);
	std::lock_guard<std::mutex> hk(h->mu);
	std::string why;
	if (gd_pile_usable(h, why)) return gd_pile_fail(h, GDIET_E_PARAM, who, why);
	GdbPart &P = gd_bam_pool(ctx).all;
	int rc = gd_bam_flatten(ctx, ix, n_reads, qnames, seqs, quals, comments, lens, n_regs, regs, opt_flag, P, why);
	if (rc) return why.empty() ? rc : gd_pile_fail(h, rc, who, why);
	if (P.bytes == 0) return GDIET_OK;
	std::vector<uint64_t> starts;
	rc = gd_bam_encode_device(ctx, P, nullptr, 0, why, [&](uint8_t *d_stream, size_t, hipStream_t s) { // (the stream is synchronised when this has returned)
		return gd_pile_enqueue_part(h, s, d_stream, P, starts, why);
	});
	if (rc) return gd_pile_fail(h, GDIET_E_HIP, who, why);
	rc = gd_pile_verdict(h, why);
	return rc ? gd_pile_fail(h, rc, who, why) : GDIET_OK;
}

extern "C" int gdiet_hip_pile_finish_chunked(gdiet_pileup *h, uint64_t chunk, gdiet_pile_summary_t *summary_out)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	const char *who = "gdiet_hip_pile_finish";
	std::lock_guard<std::mutex> hk(h->mu);
	std::string why;
	if (!h->finished) {
		if (gd_pile_usable(h, why)) return gd_pile_fail(h, GDIET_E_PARAM, who, why);
		GdLane &L = h->ctx->cov;
		std::lock_guard<std::mutex> lk(L.mu);
		if (L.ready(h->ctx->device, 0, "coverage", why)) return gd_pile_fail(h, GDIET_E_HIP, who, why);
		hipError_t e = hipMemcpyAsync(&h->summary, h->D.summary, sizeof(h->summary), hipMemcpyDeviceToHost, L.stream);
		if (e == hipSuccess) e = hipStreamSynchronize(L.stream);
		if (e != hipSuccess) { h->poisoned = true; return gd_pile_fail(h, GDIET_E_HIP, who, std::string("pileup: summary copy down: ") + hipGetErrorString(e)); }
		h->chunk = std::min<uint64_t>(chunk ? chunk : GDP_DEFAULT_CHUNK, GDP_MAX_CHUNK);
		h->finished = true;
	}
	if (summary_out) *summary_out = h->summary;
	return GDIET_OK;
}
extern "C" int gdiet_hip_pile_finish(gdiet_pileup *h, gdiet_pile_summary_t *summary_out) { return gdiet_hip_pile_finish_chunked(h, 0, summary_out); }

// 0, or -1 with why: the results can be read
static int gd_pile_readable(gdiet_pileup *h, std::string &why)
{
	if (!h->finished) { why = "pileup: not finished"; return -1; }
	if (!h->ctx || !h->d_cnt) { why = "pileup: the context has been destroyed"; return -1; }
	return 0;
}

extern "C" int gdiet_hip_pile_counts(gdiet_pileup *h, uint32_t rid, uint32_t beg, uint32_t end, uint32_t *out)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	const char *who = "gdiet_hip_pile_counts";
	std::lock_guard<std::mutex> hk(h->mu);
	std::string why;
	if (gd_pile_readable(h, why)) return gd_pile_fail(h, GDIET_E_PARAM, who, why);
	const GdpRegion *R = nullptr;
	for (const GdpRegion &g : h->regs)
		if (g.rid == rid && g.beg <= beg && beg <= end && end <= g.end) { R = &g; break; }
	if (!R) return gd_pile_fail(h, GDIET_E_PARAM, who, "pileup: the interval does not lie inside one region");
	if (beg == end) return GDIET_OK;
	if (!out) return GDIET_E_PARAM;
	GdLane &L = h->ctx->cov;
	std::lock_guard<std::mutex> lk(L.mu);
	if (L.ready(h->ctx->device, 0, "coverage", why)) return gd_pile_fail(h, GDIET_E_HIP, who, why);
	hipError_t e = hipMemcpyAsync(out, h->d_cnt + (R->off + (beg - R->beg)) * GDP_N_CNT, 4 * (size_t)GDP_N_CNT * (end - beg), hipMemcpyDeviceToHost, L.stream);
	if (e == hipSuccess) e = hipStreamSynchronize(L.stream);
	return e == hipSuccess ? GDIET_OK : gd_pile_fail(h, GDIET_E_HIP, who, std::string("pileup: counters copy down: ") + hipGetErrorString(e));
}

static GdpCallIn gd_pile_call_in(const gdiet_pileup *h, uint64_t t0, uint64_t m, const GdpCallOpt &opt)
{
	GdpCallIn I;
	I.cnt = h->d_cnt, I.regs = h->D.regs, I.S = (const uint32_t *)h->ix->d_S, I.seq_off = h->ix->d_seq_off, I.t0 = t0, I.m = m, I.n_reg = h->D.n_reg, I.opt = opt;
	return I;
}

extern "C" int gdiet_hip_pile_consensus(gdiet_pileup *h, size_t region, uint32_t min_depth, uint8_t *out)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	const char *who = "gdiet_hip_pile_consensus";
	std::lock_guard<std::mutex> hk(h->mu);
	std::string why;
	if (gd_pile_readable(h, why)) return gd_pile_fail(h, GDIET_E_PARAM, who, why);
	if (region >= h->regs.size()) return gd_pile_fail(h, GDIET_E_PARAM, who, "pileup: region " + std::to_string(region) + " of " + std::to_string(h->regs.size()));
	if (!out) return GDIET_E_PARAM;
	const GdpRegion &R = h->regs[region];
	const uint64_t n = R.end - R.beg;
	GdLane &L = h->ctx->cov;
	std::lock_guard<std::mutex> lk(L.mu);
	if (L.ready(h->ctx->device, 0, "coverage", why)) return gd_pile_fail(h, GDIET_E_HIP, who, why);
	hipStream_t s = L.stream;
	GdStreamMem mem(s);
	hipError_t e = hipSuccess;
	auto hip_fail = [&](hipError_t err, const char *what) {
		mem.fail();
		return gd_pile_fail(h, GDIET_E_HIP, who, std::string("pileup: ") + what + ": " + hipGetErrorString(err));
	};
	uint8_t *d_cons;
	if ((e = mem.alloc(&d_cons, (size_t)n + 16)) != hipSuccess) return hip_fail(e, "consensus bytes");
	const GdpCallOpt opt = {min_depth, 0, 0, 1};
	hipLaunchKernelGGL(pile_call_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, gd_pile_call_in(h, R.off, n, opt), d_cons, (uint32_t *)nullptr, (uint8_t *)nullptr);
	if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "call launch");
	if ((e = hipMemcpyAsync(out, d_cons, (size_t)n, hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(e, "consensus copy down");
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(e, "call kernel");
	return GDIET_OK;
}

extern "C" int64_t gdiet_hip_pile_sites(gdiet_pileup *h, uint32_t min_depth, uint32_t min_alt, uint32_t num, uint32_t den, gdiet_pile_site_t *out, size_t cap)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	const char *who = "gdiet_hip_pile_sites";
	std::lock_guard<std::mutex> hk(h->mu);
	std::string why;
	if (gd_pile_readable(h, why)) return gd_pile_fail(h, GDIET_E_PARAM, who, why);
	if (den == 0) return gd_pile_fail(h, GDIET_E_PARAM, who, "pileup: a fraction with den == 0");
	GdLane &L = h->ctx->cov;
	std::lock_guard<std::mutex> lk(L.mu);
	if (L.ready(h->ctx->device, 0, "coverage", why)) return gd_pile_fail(h, GDIET_E_HIP, who, why);
	hipStream_t s = L.stream;
	GdStreamMem mem(s);
	hipError_t e = hipSuccess;
	auto hip_fail = [&](hipError_t err, const char *what) {
		mem.fail();
		return (int64_t)gd_pile_fail(h, GDIET_E_HIP, who, std::string("pileup: ") + what + ": " + hipGetErrorString(err));
	};
	// per chunk of positions: flags, their exclusive sum, the chunk's count comes down (the carry), the rows are written and come down
	const uint64_t chunk = std::min<uint64_t>(h->chunk, h->total);
	const GdpCallOpt opt = {min_depth, min_alt, num, den};
	uint32_t *d_flag, *d_offs;
	uint8_t *d_alt;
	void *d_tmp;
	size_t tmp_bytes = 0;
	if ((e = mem.alloc(&d_flag, 4 * (size_t)chunk + 16)) != hipSuccess || (e = mem.alloc(&d_offs, 4 * (size_t)chunk + 16)) != hipSuccess ||
	    (e = mem.alloc(&d_alt, (size_t)chunk + 16)) != hipSuccess)
		return hip_fail(e, "flags");
	if ((e = hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_flag, d_offs, (int)chunk, s)) != hipSuccess) return hip_fail(e, "scan size");
	if ((e = mem.alloc((uint8_t **)&d_tmp, std::max<size_t>(tmp_bytes, 16))) != hipSuccess) return hip_fail(e, "scan scratch");
	uint64_t n_sites = 0;
	for (uint64_t c0 = 0; c0 < h->total; c0 += chunk) {
		const uint64_t m = std::min<uint64_t>(chunk, h->total - c0);
		const GdpCallIn I = gd_pile_call_in(h, c0, m, opt);
		const unsigned blocks = (unsigned)((m + 255) / 256);
		hipLaunchKernelGGL(pile_call_kernel, dim3(blocks), dim3(256), 0, s, I, (uint8_t *)nullptr, d_flag, d_alt);
		if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "call launch");
		size_t tb = tmp_bytes;
		if ((e = hipcub::DeviceScan::ExclusiveSum(d_tmp, tb, d_flag, d_offs, (int)m, s)) != hipSuccess) return hip_fail(e, "scan");
		uint32_t last[2] = {0, 0};
		if ((e = hipMemcpyAsync(&last[0], d_offs + (m - 1), 4, hipMemcpyDeviceToHost, s)) != hipSuccess || (e = hipMemcpyAsync(&last[1], d_flag + (m - 1), 4, hipMemcpyDeviceToHost, s)) != hipSuccess ||
		    (e = hipStreamSynchronize(s)) != hipSuccess)
			return hip_fail(e, "count copy down");
		const uint64_t n_c = (uint64_t)last[0] + last[1];
		if (out && n_c && n_sites + n_c <= cap) {
			uint32_t *d_rows;
			if ((e = mem.alloc(&d_rows, sizeof(gdiet_pile_site_t) * (size_t)n_c + 16)) != hipSuccess) return hip_fail(e, "rows");
			hipLaunchKernelGGL(pile_site_kernel, dim3(blocks), dim3(256), 0, s, I, (const uint32_t *)d_flag, (const uint32_t *)d_offs, (const uint8_t *)d_alt, d_rows, (uint32_t)n_c);
			if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "site launch");
			if ((e = hipMemcpyAsync(out + n_sites, d_rows, sizeof(gdiet_pile_site_t) * (size_t)n_c, hipMemcpyDeviceToHost, s)) != hipSuccess || (e = hipStreamSynchronize(s)) != hipSuccess)
				return hip_fail(e, "rows copy down");
		}
		n_sites += n_c;
	}
	if (out && n_sites > cap) return gd_pile_fail(h, GDIET_E_PARAM, who, "pileup: " + std::to_string(n_sites) + " sites, room for " + std::to_string(cap));
	return (int64_t)n_sites;
}

extern "C" int gdiet_hip_pile_close(gdiet_pileup *h)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	{
		std::lock_guard<std::mutex> hk(h->mu);
		if (h->ctx) {
			(void)hipSetDevice(h->ctx->device);
			std::lock_guard<std::mutex> rk(h->ctx->cov_reg_mu);
			auto &v = h->ctx->pile_open;
			v.erase(std::remove(v.begin(), v.end(), (void *)h), v.end());
		}
		gd_pile_free_arrays(h);
	}
	delete h;
	return GDIET_OK;
}
