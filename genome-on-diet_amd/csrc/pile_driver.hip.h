// Driver of the pileup accumulator (pile.hip.h) and its entry points gdiet_hip_pile_*.  Included by gdiet_hip.hip behind
// cov_driver.hip.h; the routes on which records arrive, the lock order and everything the accumulators share are in accum_driver.hip.h.
//
// The pileup's own: the counters (32 bytes per position of the regions) and one small table -- the regions, the contigs' lengths, the
// summary, the cell of the first bad record; finish; the readers and the calls after it, on the lane gdiet_ctx::cov.
#pragma once
#include <hipcub/hipcub.hpp>
#include "pile.hip.h"

static const uint64_t GDP_DEFAULT_CHUNK = 1ull << 24, GDP_MAX_CHUNK = 1ull << 30;

struct gdiet_pileup : GdAccum {
	gdiet_pileup() : GdAccum("pileup") {}
	const gdiet_index *ix = nullptr;
	uint32_t n_ref = 0;
	uint64_t total = 0, chunk = GDP_DEFAULT_CHUNK;
	std::vector<uint32_t> clen;
	std::vector<GdpRegion> regs;
	uint32_t *d_cnt = nullptr;
	uint64_t *d_tab = nullptr; // summary | first bad | regions | lengths
	GdpDev D;
	gdiet_pile_summary_t summary;
	void launch(hipStream_t s, const uint8_t *d_recs, uint64_t bytes, const uint64_t *d_start, uint64_t n, unsigned blocks) override
	{
		hipLaunchKernelGGL(pile_scatter_kernel, dim3(blocks), dim3(256), 0, s, d_recs, bytes, d_start, n, D);
	}
	void free_arrays() override
	{
		if (d_cnt) (void)hipFree(d_cnt);
		if (d_tab) (void)hipFree(d_tab);
		d_cnt = nullptr, d_tab = nullptr;
	}
};
static_assert(sizeof(gdiet_pile_summary_t) == 8 * GDP_N_SUMMARY && sizeof(gdiet_pile_site_t) == 4 * (5 + GDP_N_CNT) && sizeof(GdpRegion) == 24, "the structs of the header");

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
		gd_accum_free(h);
		const int code = gd_accum_fail(h, rc, who, what);
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
	h->d_first_bad = D.first_bad;
	gd_accum_register(ctx, h);
	*out = h;
	return GDIET_OK;
}

extern "C" int gdiet_hip_pile_add_bam(gdiet_pileup *h, const void *recs, size_t len) { return gd_accum_add_bam(h, "gdiet_hip_pile_add_bam", recs, len); }
extern "C" int gdiet_hip_pile_add(gdiet_pileup *h, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs, const char *const *quals,
                                  const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs, const char *const *comments, int64_t opt_flag)
{
	return gd_accum_add(h, "gdiet_hip_pile_add", ix, n_reads, qnames, seqs, quals, lens, n_regs, regs, comments, opt_flag);
}
extern "C" int gdiet_hip_pile_close(gdiet_pileup *h) { return gd_accum_close(h); }
extern "C" int gdiet_hip_bgzf_out_set_pileup(gdiet_bgzf_out *w, gdiet_pileup *pile)
{
	return w ? gd_accum_attach(w->ctx, w->acc, GD_ACC_PILE, pile, "gdiet_hip_bgzf_out_set_pileup", "writer") : GDIET_E_PARAM;
}

extern "C" int gdiet_hip_pile_finish_chunked(gdiet_pileup *h, uint64_t chunk, gdiet_pile_summary_t *summary_out)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	const char *who = "gdiet_hip_pile_finish";
	std::lock_guard<std::mutex> hk(h->mu);
	std::string why;
	if (!h->finished) {
		if (gd_accum_usable(h, why)) return gd_accum_fail(h, GDIET_E_PARAM, who, why);
		GdLane &L = h->ctx->cov;
		std::lock_guard<std::mutex> lk(L.mu);
		if (L.ready(h->ctx->device, 0, "coverage", why)) return gd_accum_fail(h, GDIET_E_HIP, who, why);
		hipError_t e = hipMemcpyAsync(&h->summary, h->D.summary, sizeof(h->summary), hipMemcpyDeviceToHost, L.stream);
		if (e == hipSuccess) e = hipStreamSynchronize(L.stream);
		if (e != hipSuccess) { h->poisoned = true; return gd_accum_fail(h, GDIET_E_HIP, who, std::string("pileup: summary copy down: ") + hipGetErrorString(e)); }
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
	if (gd_pile_readable(h, why)) return gd_accum_fail(h, GDIET_E_PARAM, who, why);
	const GdpRegion *R = nullptr;
	for (const GdpRegion &g : h->regs)
		if (g.rid == rid && g.beg <= beg && beg <= end && end <= g.end) { R = &g; break; }
	if (!R) return gd_accum_fail(h, GDIET_E_PARAM, who, "pileup: the interval does not lie inside one region");
	if (beg == end) return GDIET_OK;
	if (!out) return GDIET_E_PARAM;
	GdLane &L = h->ctx->cov;
	std::lock_guard<std::mutex> lk(L.mu);
	if (L.ready(h->ctx->device, 0, "coverage", why)) return gd_accum_fail(h, GDIET_E_HIP, who, why);
	hipError_t e = hipMemcpyAsync(out, h->d_cnt + (R->off + (beg - R->beg)) * GDP_N_CNT, 4 * (size_t)GDP_N_CNT * (end - beg), hipMemcpyDeviceToHost, L.stream);
	if (e == hipSuccess) e = hipStreamSynchronize(L.stream);
	return e == hipSuccess ? GDIET_OK : gd_accum_fail(h, GDIET_E_HIP, who, std::string("pileup: counters copy down: ") + hipGetErrorString(e));
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
	if (gd_pile_readable(h, why)) return gd_accum_fail(h, GDIET_E_PARAM, who, why);
	if (region >= h->regs.size()) return gd_accum_fail(h, GDIET_E_PARAM, who, "pileup: region " + std::to_string(region) + " of " + std::to_string(h->regs.size()));
	if (!out) return GDIET_E_PARAM;
	const GdpRegion &R = h->regs[region];
	const uint64_t n = R.end - R.beg;
	GdLane &L = h->ctx->cov;
	std::lock_guard<std::mutex> lk(L.mu);
	if (L.ready(h->ctx->device, 0, "coverage", why)) return gd_accum_fail(h, GDIET_E_HIP, who, why);
	hipStream_t s = L.stream;
	GdStreamMem mem(s);
	hipError_t e = hipSuccess;
	auto hip_fail = [&](hipError_t err, const char *what) {
		mem.fail();
		return gd_accum_fail(h, GDIET_E_HIP, who, std::string("pileup: ") + what + ": " + hipGetErrorString(err));
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
	if (gd_pile_readable(h, why)) return gd_accum_fail(h, GDIET_E_PARAM, who, why);
	if (den == 0) return gd_accum_fail(h, GDIET_E_PARAM, who, "pileup: a fraction with den == 0");
	GdLane &L = h->ctx->cov;
	std::lock_guard<std::mutex> lk(L.mu);
	if (L.ready(h->ctx->device, 0, "coverage", why)) return gd_accum_fail(h, GDIET_E_HIP, who, why);
	hipStream_t s = L.stream;
	GdStreamMem mem(s);
	hipError_t e = hipSuccess;
	auto hip_fail = [&](hipError_t err, const char *what) {
		mem.fail();
		return (int64_t)gd_accum_fail(h, GDIET_E_HIP, who, std::string("pileup: ") + what + ": " + hipGetErrorString(err));
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
	if (out && n_sites > cap) return gd_accum_fail(h, GDIET_E_PARAM, who, "pileup: " + std::to_string(n_sites) + " sites, room for " + std::to_string(cap));
	return (int64_t)n_sites;
}
