// Driver of the statistics accumulator (stats.hip.h) and its entry points gdiet_hip_stats_*.  Included by gdiet_hip.hip behind
// pile_driver.hip.h; the routes on which records arrive, the lock order and everything the accumulators share are in accum_driver.hip.h.
//
// The accumulator's own: one array of uint64 cells (stats.h, THE CELLS: a few tens of kilobytes plus 8 bytes per read-length bin) with
// the cell of the first bad record and the contigs' lengths behind it; finish, which needs no kernel -- the cells come down on the lane
// gdiet_ctx::cov --, and the reader of a table after it.
#pragma once
#include "stats.hip.h"

struct gdiet_stats : GdAccum {
	gdiet_stats() : GdAccum("stats") {}
	const gdiet_index *ix = nullptr;
	std::vector<uint32_t> clen;
	uint64_t *d_cells = nullptr; // cells | first bad | lengths
	size_t lds_bytes = 0;
	GdtDev D;
	std::vector<uint64_t> cells; // after finish
	void launch(hipStream_t s, const uint8_t *d_recs, uint64_t bytes, const uint64_t *d_start, uint64_t n, unsigned blocks) override
	{
		hipLaunchKernelGGL(stats_scatter_kernel, dim3(std::min<unsigned>(blocks, GDT_MAX_BLOCKS)), dim3(256), lds_bytes, s, d_recs, bytes, d_start, n, D);
	}
	void free_arrays() override
	{
		if (d_cells) (void)hipFree(d_cells);
		d_cells = nullptr;
	}
};
static_assert(sizeof(gdiet_stats_summary_t) == 8 * GDT_N_SUMMARY, "the structs of the header");
static_assert(GDIET_STATS_GC == GDT_T_GC && GDIET_STATS_IDENTITY == GDT_T_IDENTITY && GDIET_STATS_READ_LEN == GDT_T_READ_LEN, "the tables of the header");

extern "C" int gdiet_hip_stats_open_bounded(gdiet_ctx *ctx, const gdiet_index *ix, uint32_t excl_flags, uint32_t min_mapq, uint32_t cycles, uint32_t max_len, uint32_t max_indel,
                                            uint64_t bound, gdiet_stats **out)
{
	if (!ctx || !ix || !out) return GDIET_E_PARAM;
	*out = nullptr;
	gd_err_clear();
	const char *who = "gdiet_hip_stats_open";
	gdiet_stats *h = new gdiet_stats();
	h->ctx = ctx, h->ix = ix;
	const size_t n_ref = ix->h.seq.size();
	h->clen.resize(n_ref);
	for (size_t i = 0; i < n_ref; ++i) h->clen[i] = ix->h.seq[i].len;
	auto refuse = [&](int rc, const std::string &what) {
		gd_accum_free(h);
		const int code = gd_accum_fail(h, rc, who, what);
		delete h;
		return code;
	};
	if (n_ref == 0 || n_ref > 0x7fffffffull) return refuse(GDIET_E_PARAM, "an index without contigs");
	if (cycles < 1 || cycles > GDT_MAX_CYCLES) return refuse(GDIET_E_PARAM, "cycles is " + std::to_string(cycles) + ": 1 to " + std::to_string((int)GDT_MAX_CYCLES));
	if (max_len < 1 || max_len > GDT_MAX_LEN) return refuse(GDIET_E_PARAM, "max_len is " + std::to_string(max_len) + ": 1 to " + std::to_string((int)GDT_MAX_LEN));
	if (max_indel < 1 || max_indel > GDT_MAX_INDEL) return refuse(GDIET_E_PARAM, "max_indel is " + std::to_string(max_indel) + ": 1 to " + std::to_string((int)GDT_MAX_INDEL));
	if (bound > GDT_DEFAULT_BOUND) return refuse(GDIET_E_PARAM, "bound is " + std::to_string(bound) + ": at most " + std::to_string(GDT_DEFAULT_BOUND));
	(void)hipSetDevice(ctx->device);
	if (gd_index_seq_table(ctx, ix)) return refuse(GDIET_E_HIP, "stats: the contig table: " + ctx->err);
	GdtDev &D = h->D;
	D.Y = gdt_layout(cycles, max_len, max_indel);
	h->lds_bytes = 4 * ((size_t)D.Y.n_lds + 8);
	hipError_t e = hipSuccess;
	if (h->lds_bytes > 64 * 1024 && (e = hipFuncSetAttribute((const void *)stats_scatter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes)) != hipSuccess) {
		(void)hipGetLastError();
		return refuse(GDIET_E_HIP, std::string("stats: local memory of ") + std::to_string(h->lds_bytes) + " bytes: " + hipGetErrorString(e));
	}
	const size_t bytes = 8 * ((size_t)D.Y.n_all + 1) + 4 * n_ref;
	if ((e = hipMalloc((void **)&h->d_cells, bytes)) != hipSuccess) {
		h->d_cells = nullptr;
		(void)hipGetLastError();
		return refuse(GDIET_E_NOMEM, "the tables take " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
	}
	D.cells = h->d_cells, D.first_bad = h->d_cells + D.Y.n_all, D.clen = (const uint32_t *)(D.first_bad + 1);
	D.S = (const uint32_t *)ix->d_S, D.seq_off = ix->d_seq_off, D.n_ref = (uint32_t)n_ref, D.bound = bound ? bound : GDT_DEFAULT_BOUND;
	D.opt.excl_flags = excl_flags, D.opt.min_mapq = min_mapq, D.opt.cycles = cycles, D.opt.max_len = max_len, D.opt.max_indel = max_indel;
	GdLane &L = ctx->cov;
	std::lock_guard<std::mutex> lk(L.mu);
	std::string why;
	if (L.ready(ctx->device, 0, "coverage", why)) return refuse(GDIET_E_HIP, why);
	hipStream_t s = L.stream;
	if ((e = hipMemsetAsync(h->d_cells, 0, bytes, s)) != hipSuccess || (e = hipMemcpyAsync((void *)D.clen, h->clen.data(), 4 * n_ref, hipMemcpyHostToDevice, s)) != hipSuccess ||
	    (e = hipStreamSynchronize(s)) != hipSuccess) {
		(void)hipStreamSynchronize(s);
		return refuse(GDIET_E_HIP, std::string("stats: clearing the tables: ") + hipGetErrorString(e));
	}
	h->d_first_bad = D.first_bad;
	gd_accum_register(ctx, h);
	*out = h;
	return GDIET_OK;
}
extern "C" int gdiet_hip_stats_open(gdiet_ctx *ctx, const gdiet_index *ix, uint32_t excl_flags, uint32_t min_mapq, uint32_t cycles, uint32_t max_len, uint32_t max_indel, gdiet_stats **out)
{
	return gdiet_hip_stats_open_bounded(ctx, ix, excl_flags, min_mapq, cycles, max_len, max_indel, 0, out);
}

extern "C" int gdiet_hip_stats_add_bam(gdiet_stats *h, const void *recs, size_t len) { return gd_accum_add_bam(h, "gdiet_hip_stats_add_bam", recs, len); }
extern "C" int gdiet_hip_stats_add(gdiet_stats *h, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs, const char *const *quals, const int32_t *lens,
                                   const int32_t *n_regs, gdiet_reg_t *const *regs, const char *const *comments, int64_t opt_flag)
{
	return gd_accum_add(h, "gdiet_hip_stats_add", ix, n_reads, qnames, seqs, quals, lens, n_regs, regs, comments, opt_flag);
}
extern "C" int gdiet_hip_stats_close(gdiet_stats *h) { return gd_accum_close(h); }
extern "C" int gdiet_hip_bgzf_out_set_stats(gdiet_bgzf_out *w, gdiet_stats *stats)
{
	return w ? gd_accum_attach(w->ctx, w->acc, GD_ACC_STATS, stats, "gdiet_hip_bgzf_out_set_stats", "writer") : GDIET_E_PARAM;
}

extern "C" int gdiet_hip_stats_finish(gdiet_stats *h, gdiet_stats_summary_t *summary_out)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	const char *who = "gdiet_hip_stats_finish";
	std::lock_guard<std::mutex> hk(h->mu);
	std::string why;
	if (!h->finished) {
		if (gd_accum_usable(h, why)) return gd_accum_fail(h, GDIET_E_PARAM, who, why);
		GdLane &L = h->ctx->cov;
		std::lock_guard<std::mutex> lk(L.mu);
		if (L.ready(h->ctx->device, 0, "coverage", why)) return gd_accum_fail(h, GDIET_E_HIP, who, why);
		h->cells.resize(h->D.Y.n_all);
		hipError_t e = hipMemcpyAsync(h->cells.data(), h->d_cells, 8 * (size_t)h->D.Y.n_all, hipMemcpyDeviceToHost, L.stream);
		if (e == hipSuccess) e = hipStreamSynchronize(L.stream);
		if (e != hipSuccess) { h->poisoned = true; return gd_accum_fail(h, GDIET_E_HIP, who, std::string("stats: tables copy down: ") + hipGetErrorString(e)); }
		h->finished = true;
	}
	if (summary_out) memcpy(summary_out, h->cells.data() + h->D.Y.off[GDT_T_SUMMARY], sizeof *summary_out);
	return GDIET_OK;
}

extern "C" int64_t gdiet_hip_stats_table(gdiet_stats *h, int which, uint64_t *out, size_t cap)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	const char *who = "gdiet_hip_stats_table";
	std::lock_guard<std::mutex> hk(h->mu);
	if (!h->finished) return gd_accum_fail(h, GDIET_E_PARAM, who, "stats: not finished");
	if (!h->ctx || !h->d_cells) return gd_accum_fail(h, GDIET_E_PARAM, who, "stats: the context has been destroyed");
	if (which < 0 || which >= GDT_T_SUMMARY) return gd_accum_fail(h, GDIET_E_PARAM, who, "stats: table " + std::to_string(which) + " of " + std::to_string((int)GDT_T_SUMMARY));
	const size_t n = h->D.Y.len[which];
	if (!out) return (int64_t)n;
	if (cap < n) return gd_accum_fail(h, GDIET_E_PARAM, who, "stats: the table holds " + std::to_string(n) + " counters, room for " + std::to_string(cap));
	memcpy(out, h->cells.data() + h->D.Y.off[which], 8 * n);
	return (int64_t)n;
}
