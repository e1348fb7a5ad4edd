// Driver of the difference-string kernel (map_diffstr.hip.h); included by map_pipeline.hip.h (needs gdiet_ctx, gdiet_index,
// gdiet_read_batch, gd_parallel_for, gd_index_seq_table).  mm_gen_cs_or_MD (LR/format.c:270-281) for every record of a mini-batch.
// The call works on a lane and device buffers of its own (gdiet_ctx::ds, ds_*): it touches nothing a map call or an open ticket uses, so
// it is safe from another caller thread while batches are in flight -- the position gdiet_hip_sam_batch is called from.  The text of a
// failing pass is kept apart from gdiet_ctx::err, with the thread whose call failed (err_mark.h): the pass is designed to refuse bad
// records on a writer thread while a mapping thread may be writing err.
#pragma once
#include "map_diffstr.hip.h"

// (like gd_grow, on the difference strings' own stream; the caller holds ds.mu)
static int gd_ds_grow(gdiet_ctx *ctx, DevBuf &b, size_t bytes, std::string &why)
{
	if (bytes <= b.cap) return GDIET_OK;
	hipError_t e0 = hipStreamSynchronize(ctx->ds.stream);
	if (e0 == hipSuccess) e0 = b.release();
	if (e0 != hipSuccess) { why = std::string("difference strings: buffer: ") + hipGetErrorString(e0); return GDIET_E_HIP; }
	b.kind = DevBuf::DEVICE;
	const size_t want = bytes + (bytes >> 3) + 4096;
	const hipError_t e = hipMalloc(&b.p, want);
	if (e != hipSuccess) {
		(void)hipGetLastError();
		why = "hipMalloc of " + std::to_string(want) + " bytes failed: " + hipGetErrorString(e);
		b.p = nullptr;
		return GDIET_E_NOMEM;
	}
	b.cap = want;
	return GDIET_OK;
}

// -1: neither tag asked for; else GDD_MD / GDD_CS / GDD_CS_LONG (the two flags together mean MD: LR/format.c:261)
static int gd_ds_mode(int64_t opt_flag)
{
	if (opt_flag & GD_F_OUT_MD) return GDD_MD;
	if (opt_flag & GD_F_OUT_CS) return (opt_flag & GD_F_OUT_CS_LONG) ? GDD_CS_LONG : GDD_CS;
	return -1;
}

// *text / *off are malloc'd: off[k] .. off[k + 1] is the string of record k, records read-major in the order of regs[i]
static int gd_diffstr_run(gdiet_ctx *ctx, const gdiet_index *ix, const gdiet_read_batch *batch, int n_reads, const char *const *seqs, const int32_t *lens,
                          const int32_t *n_regs, gdiet_reg_t *const *regs, int64_t opt_flag, char **text, int64_t **off)
{
	*text = nullptr, *off = nullptr;
	gd_err_clear();
	std::lock_guard<std::mutex> lk(ctx->ds.mu); // (from the first check on: the buffers belong to one call at a time)
	const int mode = gd_ds_mode(opt_flag);
	int64_t n_rec = 0, n_cig = 0;
	for (int i = 0; i < n_reads; ++i)
		for (int j = 0; j < n_regs[i]; ++j) ++n_rec, n_cig += regs[i][j].n_cigar;
	int64_t *h_off = (int64_t *)calloc((size_t)n_rec + 1, sizeof(int64_t));
	auto fail = [&](int rc, const std::string &what) { free(h_off); return gd_err_fail(ctx, rc, what); };
	if (!h_off) return fail(GDIET_E_NOMEM, "out of host memory");
	if (mode < 0 || n_rec == 0) {
		char *t = (char *)calloc(1, 1);
		if (!t) return fail(GDIET_E_NOMEM, "out of host memory");
		*text = t, *off = h_off;
		return GDIET_OK;
	}
	if (batch && batch->n != n_reads) return fail(GDIET_E_PARAM, "the resident batch holds another number of reads");
	if (!batch && (!seqs || !lens)) return fail(GDIET_E_PARAM, "neither a resident batch nor sequences");
	// the record table and its host check: nothing is launched for a batch with a record the kernel must not see
	const GdRefView R = ix->h.ref();
	std::vector<GddRec> rec((size_t)n_rec);
	std::vector<uint32_t> cig((size_t)n_cig + 1);
	{
		int64_t k = 0, c = 0;
		for (int i = 0; i < n_reads; ++i)
			for (int j = 0; j < n_regs[i]; ++j, ++k) {
				const gdiet_reg_t &g = regs[i][j];
				GddRec &r = rec[(size_t)k];
				r.read = i, r.qs = g.qs, r.qe = g.qe, r.rs = g.rs, r.re = g.re, r.rid = g.rid, r.rev = g.rev ? 1 : 0, r.n_cigar = g.n_cigar, r.cig_off = c;
				if (g.n_cigar == 0) { r.qe = r.qs, r.re = r.rs; if (r.rid < 0 || (uint32_t)r.rid >= R.n_seq) r.rid = 0; continue; } // no alignment (r->p == 0): no string
				if (!g.cigar) return fail(GDIET_E_PARAM, "read " + std::to_string(i) + " record " + std::to_string(j) + ": no CIGAR array");
				memcpy(cig.data() + c, g.cigar, sizeof(uint32_t) * g.n_cigar);
				c += g.n_cigar;
				const int64_t rl = batch ? batch->roff[i + 1] - batch->roff[i] : (lens[i] > 0 ? lens[i] : 0);
				int bad = (r.rid < 0 || (uint32_t)r.rid >= R.n_seq) ? 1 : gdd_check_record(r, g.cigar, rl, R.seq[r.rid].len, mode != GDD_MD);
				if (bad) {
					static const char *const why[] = {"", "rid out of range", "qs / qe outside the read", "rs / re outside the contig", "a CIGAR operation other than M I D N = X",
					                                  "an N operation shorter than 2", "the CIGAR's lengths do not sum to qe - qs and re - rs"};
					return fail(GDIET_E_PARAM, "difference string of read " + std::to_string(i) + " record " + std::to_string(j) + ": " + why[bad]);
				}
			}
	}
	(void)hipSetDevice(ctx->device);
	int rc = gd_index_seq_table(ctx, ix);
	if (rc) return fail(rc, "difference strings: the contig table could not be uploaded");
	auto hip_fail = [&](hipError_t e, const char *what) { return fail(GDIET_E_HIP, std::string(what) + ": " + hipGetErrorString(e)); };
	hipError_t e;
	std::string why; // of ready() and gd_ds_grow
	if (ctx->ds.ready(ctx->device, 0, "difference strings", why)) return fail(GDIET_E_HIP, why);
	hipStream_t s = ctx->ds.stream;
	const uint8_t *d_reads;
	const int64_t *d_roff;
	if (batch) d_reads = (const uint8_t *)batch->d_reads, d_roff = (const int64_t *)batch->d_roff;
	else { // encode and upload the reads (what a caller with a resident batch saves)
		std::vector<int64_t> roff((size_t)n_reads + 1, 0);
		for (int i = 0; i < n_reads; ++i) roff[i + 1] = roff[i] + (lens[i] > 0 ? lens[i] : 0);
		const size_t bytes = (size_t)roff[n_reads] + 8;
		if (ctx->ds_enc.size() < bytes) ctx->ds_enc.resize(bytes + (bytes >> 3));
		uint8_t *enc = ctx->ds_enc.data();
		gd_parallel_for(ctx, ctx->host_threads, n_reads, [&](int i) {
			if (lens[i] > 0 && n_regs[i] > 0) gd_nt4_encode(seqs[i], enc + roff[i], (size_t)lens[i]); // (reads without records are never read)
		});
		if ((rc = gd_ds_grow(ctx, ctx->ds_reads, bytes, why)) || (rc = gd_ds_grow(ctx, ctx->ds_roff, sizeof(int64_t) * ((size_t)n_reads + 1), why))) return fail(rc, why);
		if ((e = hipMemcpyAsync(ctx->ds_reads.p, enc, bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e, "difference strings: reads");
		if ((e = hipMemcpyAsync(ctx->ds_roff.p, roff.data(), sizeof(int64_t) * ((size_t)n_reads + 1), hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e, "difference strings: reads");
		if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(e, "difference strings: reads"); // (roff is a local)
		d_reads = (const uint8_t *)ctx->ds_reads.p, d_roff = (const int64_t *)ctx->ds_roff.p;
	}
	if ((rc = gd_ds_grow(ctx, ctx->ds_rec, sizeof(GddRec) * (size_t)n_rec, why)) || (rc = gd_ds_grow(ctx, ctx->ds_cig, sizeof(uint32_t) * cig.size(), why)) ||
	    (rc = gd_ds_grow(ctx, ctx->ds_len, sizeof(int64_t) * ((size_t)n_rec + 1), why)) || (rc = gd_ds_grow(ctx, ctx->ds_off, sizeof(int64_t) * ((size_t)n_rec + 1), why)))
		return fail(rc, why);
	if ((e = hipMemcpyAsync(ctx->ds_rec.p, rec.data(), sizeof(GddRec) * (size_t)n_rec, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e, "difference strings: records");
	if ((e = hipMemcpyAsync(ctx->ds_cig.p, cig.data(), sizeof(uint32_t) * cig.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e, "difference strings: records");
	if ((e = hipMemsetAsync((int64_t *)ctx->ds_len.p + n_rec, 0, sizeof(int64_t), s)) != hipSuccess) return hip_fail(e, "difference strings: lengths");
	GddIn in;
	in.rec = (const GddRec *)ctx->ds_rec.p, in.cig = (const uint32_t *)ctx->ds_cig.p, in.reads = d_reads, in.roff = d_roff, in.S = (const uint32_t *)ix->d_S;
	in.seq_off = ix->d_seq_off, in.seq_len = ix->d_seq_len, in.qstrand = (opt_flag & GD_F_QSTRAND) ? 1 : 0;
	int64_t *d_len = (int64_t *)ctx->ds_len.p, *d_off = (int64_t *)ctx->ds_off.p;
	// count pass, exclusive scan over n + 1 entries (the last output is the total), and the offsets back: the host sizes the text by them
	map_diffstr_launch<false>(mode, s, n_rec, in, d_len, nullptr, nullptr);
	size_t sb = 0;
	if ((e = hipcub::DeviceScan::ExclusiveSum(nullptr, sb, d_len, d_off, (int)(n_rec + 1), s)) != hipSuccess) return hip_fail(e, "difference strings: scan");
	if ((rc = gd_ds_grow(ctx, ctx->ds_scan, sb + 64, why))) return fail(rc, why);
	sb = ctx->ds_scan.cap;
	if ((e = hipcub::DeviceScan::ExclusiveSum(ctx->ds_scan.p, sb, d_len, d_off, (int)(n_rec + 1), s)) != hipSuccess) return hip_fail(e, "difference strings: scan");
	if ((e = hipMemcpyAsync(h_off, d_off, sizeof(int64_t) * ((size_t)n_rec + 1), hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(e, "difference strings: offsets");
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(e, "difference strings: count pass");
	const int64_t total = h_off[n_rec];
	char *t = (char *)malloc((size_t)total + 1);
	if (!t) return fail(GDIET_E_NOMEM, "out of host memory");
	t[total] = 0;
	if (total > 0) {
		if ((rc = gd_ds_grow(ctx, ctx->ds_text, (size_t)total, why))) { free(t); return fail(rc, why); }
		map_diffstr_launch<true>(mode, s, n_rec, in, nullptr, d_off, (char *)ctx->ds_text.p);
		if ((e = hipMemcpyAsync(t, ctx->ds_text.p, (size_t)total, hipMemcpyDeviceToHost, s)) != hipSuccess) { free(t); return hip_fail(e, "difference strings: text"); }
		if ((e = hipStreamSynchronize(s)) != hipSuccess) { free(t); return hip_fail(e, "difference strings: write pass"); }
	}
	*text = t, *off = h_off;
	return GDIET_OK;
}

extern "C" int gdiet_hip_diffstr_batch(gdiet_ctx *ctx, const gdiet_index *ix, const gdiet_read_batch *batch, int n_reads, const char *const *seqs,
                                       const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs, int64_t opt_flag, char **text, int64_t **off)
{
	if (!ctx || !ix || n_reads < 0 || !text || !off || (n_reads && (!n_regs || !regs))) return GDIET_E_PARAM;
	return gd_diffstr_run(ctx, ix, batch, n_reads, seqs, lens, n_regs, regs, opt_flag, text, off);
}

// the strings of a batch as the formatters read them: record j of read i
struct GdDsText {
	char *text = nullptr;
	int64_t *off = nullptr;
	std::vector<int64_t> first; // index of read i's first record; n_reads + 1 entries
	GdDsText() = default;
	GdDsText(const GdDsText &) = delete;
	GdDsText &operator=(const GdDsText &) = delete;
	~GdDsText() { free(text), free(off); }
	const char *str(int i, int j) const { return text ? text + off[first[(size_t)i] + j] : nullptr; }
	size_t len(int i, int j) const { return text ? (size_t)(off[first[(size_t)i] + j + 1] - off[first[(size_t)i] + j]) : 0; }
	size_t bytes_of_read(int i) const { return text ? (size_t)(off[first[(size_t)i + 1]] - off[first[(size_t)i]]) : 0; }
};

static int gd_ds_for_batch(gdiet_ctx *ctx, const gdiet_index *ix, int n_reads, const char *const *seqs, const int32_t *lens, const int32_t *n_regs,
                           gdiet_reg_t *const *regs, int64_t opt_flag, GdDsText &ds)
{
	ds.first.assign((size_t)n_reads + 1, 0);
	for (int i = 0; i < n_reads; ++i) ds.first[(size_t)i + 1] = ds.first[(size_t)i] + (n_regs[i] > 0 ? n_regs[i] : 0);
	return gd_diffstr_run(ctx, ix, nullptr, n_reads, seqs, lens, n_regs, regs, opt_flag, &ds.text, &ds.off);
}
