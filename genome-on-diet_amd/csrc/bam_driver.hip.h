// Driver of the BAM record encoder (bam_encode.hip.h) and the three entry points that write BAM: gdiet_hip_bam_header,
// gdiet_hip_bam_batch_into and gdiet_hip_bgzf_out_write_bam.  Included by gdiet_hip.hip behind the BGZF writer (needs gdiet_ctx,
// gdiet_index, gdiet_bgzf_out, gd_parallel_for, gd_ds_for_batch, gd_bz_deflate_resident).
//
// A batch is flattened on the context's host threads (bam_flatten.h: chunks of reads side by side, every chunk with pools of its own,
// merged by a prefix sum of their sizes), the table and the pools go up, ONE kernel writes every record at its final offset of a resident
// stream, and then either the stream comes down (gdiet_hip_bam_batch_into) or the BGZF deflate kernel reads it where it is
// (gdiet_hip_bgzf_out_write_bam on a writer with a context) and only compressed members and the next tail come down.  A lane of the
// context's own (gdiet_ctx::bam), like the deflate driver: a writer thread encodes batch i while batch i + 1 maps.
// Failures leave their text with the calling thread (gd_err_fail), as the BGZF writing side does.
#pragma once
#include "bam_encode.hip.h"
#include "bam_flatten.h"

// the chunks' pools and the merged table of a batch: the context's (gdiet_ctx::bam_pool), so that they keep their pages from mini-batch to
// mini-batch -- a mini-batch is some 130 MB of table and text, and a fresh allocation of that size is paid for page by page every time
struct GdbPool { std::vector<GdbPart> parts; GdbPart all; };
static GdbPool &gd_bam_pool(gdiet_ctx *ctx) // the caller holds bam.mu
{
	if (!ctx->bam_pool) ctx->bam_pool = std::make_shared<GdbPool>();
	return *static_cast<GdbPool *>(ctx->bam_pool.get());
}

// the records of a batch as one table (all: the pool's, whose vectors are resized, not cleared, so only growth touches new pages); 0, or a GDIET_E_* code with the reason in why ("" when a difference-string pass failed: its text is kept by that pass)
static int gd_bam_flatten(gdiet_ctx *ctx, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs, const char *const *quals,
                          const char *const *comments, const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs, int64_t opt_flag, GdbPart &all, std::string &why)
{
	const char *rg = ctx->rg_id.empty() ? nullptr : ctx->rg_id.c_str();
	GdDsText ds; // --cs / --MD: one pass over the batch on the device, as in gd_sam_batch_impl
	if (gd_ds_mode(opt_flag) >= 0) {
		const int rc = gd_ds_for_batch(ctx, ix, n_reads, seqs, lens, n_regs, regs, opt_flag & ~GD_F_QSTRAND, ds);
		if (rc) { why.clear(); return rc; }
	}
	const int CH = gd_fmt_chunk(ctx, n_reads), n_ch = (n_reads + CH - 1) / CH;
	std::vector<GdbPart> &part = gd_bam_pool(ctx).parts; // (the caller holds bam.mu)
	if (part.size() < (size_t)n_ch) part.resize((size_t)n_ch);
	for (int c = 0; c < n_ch; ++c) part[c].clear();
	std::vector<std::string> err((size_t)n_ch);
	const GdRefView R = ix->h.ref();
	gd_parallel_for(ctx, ctx->host_threads, n_ch, [&](int c) {
		static thread_local std::vector<GdReg> v;
		const int i1 = std::min(n_reads, (c + 1) * CH);
		for (int i = c * CH; i < i1 && err[c].empty(); ++i) {
			const int nr = n_regs[i] > 0 ? n_regs[i] : 0;
			v.resize((size_t)nr);
			for (int j = 0; j < nr; ++j) gd_reg_from_c(regs[i][j], v[j]);
			err[c] = gdb_flatten_read(part[c], R, qnames[i], seqs[i], quals ? quals[i] : nullptr, lens[i], v, opt_flag, rg, comments ? comments[i] : nullptr,
			                          [&](int j, size_t *l) { *l = ds.len(i, j); return ds.str(i, j); });
		}
	});
	for (int c = 0; c < n_ch; ++c)
		if (!err[c].empty()) { why = err[c]; return GDIET_E_PARAM; }
	// the chunks behind one another: bases by a prefix sum, then every chunk copies and rebases its own rows
	std::vector<uint64_t> t0((size_t)n_ch + 1, 0), b0(t0), c0(t0), o0(t0), r0(t0);
	for (int c = 0; c < n_ch; ++c) {
		t0[c + 1] = t0[c] + part[c].text.size(), b0[c + 1] = b0[c] + part[c].blob.size(), c0[c + 1] = c0[c] + part[c].cig.size();
		o0[c + 1] = o0[c] + part[c].bytes, r0[c + 1] = r0[c] + part[c].rec.size();
	}
	all.text.resize(t0[n_ch]), all.blob.resize(b0[n_ch]), all.cig.resize(c0[n_ch]), all.rec.resize(r0[n_ch]), all.bytes = o0[n_ch];
	gd_parallel_for(ctx, ctx->host_threads, n_ch, [&](int c) {
		const GdbPart &p = part[c];
		if (!p.text.empty()) memcpy(all.text.data() + t0[c], p.text.data(), p.text.size());
		if (!p.blob.empty()) memcpy(all.blob.data() + b0[c], p.blob.data(), p.blob.size());
		if (!p.cig.empty()) memcpy(all.cig.data() + c0[c], p.cig.data(), sizeof(uint32_t) * p.cig.size());
		for (size_t k = 0; k < p.rec.size(); ++k) {
			GdbRec g = p.rec[k];
			g.out += o0[c], g.name += t0[c], g.seq += t0[c], g.qual += t0[c], g.cig += c0[c];
			for (int b = 0; b < 3; ++b) g.blob[b] += b0[c];
			all.rec[r0[c] + k] = g;
		}
	});
	return 0;
}

// The records of P written on the device behind front[0, front_len) (the BGZF writer's waiting tail; may be empty) in one resident buffer
// of front_len + P.bytes bytes, which `use(d_stream, bytes, stream)` then reads: it returns a hipError_t-free 0 or -1 with why set.  The
// stream has been synchronised when use() runs.  Returns 0 or -1 (the device failed; why says where).
template <class Use>
static int gd_bam_encode_device(gdiet_ctx *ctx, const GdbPart &P, const unsigned char *front, size_t front_len, std::string &why, Use use)
{
	GdLane &L = ctx->bam; // (the caller holds bam.mu, from the flattening on: the table it made is the context's)
	if (L.ready(ctx->device, 4, "device BAM encoder", why)) return -1;
	hipStream_t s = L.stream;
	hipError_t e = hipSuccess;
	GdStreamMem mem(s);
	uint8_t *d_stream, *d_text, *d_blob;
	uint32_t *d_cig;
	GdbRec *d_rec;
	auto fail = [&](hipError_t err, const char *what) {
		mem.fail();
		why = std::string("device BAM encoder: ") + what + ": " + hipGetErrorString(err);
		return -1;
	};
	const size_t n = P.rec.size(), total = front_len + (size_t)P.bytes;
	if ((n + 3) / 4 > 0x7fffffffull) { why = "device BAM encoder: too many records for one launch"; return -1; }
	if ((e = mem.alloc(&d_stream, total + 16)) != hipSuccess) return fail(e, "stream buffer");
	if ((e = mem.alloc(&d_text, P.text.size() + 16)) != hipSuccess) return fail(e, "read text");
	if ((e = mem.alloc(&d_blob, P.blob.size() + 16)) != hipSuccess) return fail(e, "tag blobs");
	if ((e = mem.alloc(&d_cig, sizeof(uint32_t) * P.cig.size() + 16)) != hipSuccess) return fail(e, "CIGAR pool");
	if ((e = mem.alloc(&d_rec, sizeof(GdbRec) * n + 16)) != hipSuccess) return fail(e, "record table");
	(void)hipEventRecord(L.ev[0], s);
	if (front_len && (e = hipMemcpyAsync(d_stream, front, front_len, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "tail copy");
	if (!P.text.empty() && (e = hipMemcpyAsync(d_text, P.text.data(), P.text.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "read text copy");
	if (!P.blob.empty() && (e = hipMemcpyAsync(d_blob, P.blob.data(), P.blob.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "tag blobs copy");
	if (!P.cig.empty() && (e = hipMemcpyAsync(d_cig, P.cig.data(), sizeof(uint32_t) * P.cig.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "CIGAR pool copy");
	if (n && (e = hipMemcpyAsync(d_rec, P.rec.data(), sizeof(GdbRec) * n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "record table copy");
	(void)hipEventRecord(L.ev[1], s);
	if (n) {
		hipLaunchKernelGGL(bam_encode_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, (const GdbRec *)d_rec, (uint64_t)n, (const uint8_t *)d_text, (const uint32_t *)d_cig,
		                   (const uint8_t *)d_blob, d_stream + front_len, (uint64_t)P.bytes);
		if ((e = hipGetLastError()) != hipSuccess) return fail(e, "launch");
	}
	(void)hipEventRecord(L.ev[2], s);
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "kernel");
	const int rc = use(d_stream, total, s);
	(void)hipEventRecord(L.ev[3], s);
	if (rc) { mem.fail(); return -1; } // (why is use()'s)
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "copy down");
	for (int i = 0; i < 3; ++i) { // (for measurements: gdiet_hip_debug_bam_seconds)
		float ms = 0;
		if (hipEventElapsedTime(&ms, L.ev[i], L.ev[i + 1]) == hipSuccess) L.ms[i] += ms;
	}
	return 0;
}

static int gd_bam_args_ok(gdiet_ctx *ctx, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs, const int32_t *lens, const int32_t *n_regs,
                          gdiet_reg_t *const *regs)
{
	return ctx && ix && n_reads >= 0 && (n_reads == 0 || (qnames && seqs && lens && n_regs && regs));
}

#include "accum_driver.hip.h" // the accumulators over the records encoded above: their add routes use the encoder, gdiet_hip_bgzf_out_write_bam below feeds the attached ones

// magic, the text gdiet_hip_sam_header returns (no NUL), the reference dictionary
extern "C" size_t gdiet_hip_bam_header(gdiet_ctx *ctx, const gdiet_index *ix, const char *version, int argc, const char *const *argv, char **out)
{
	if (!ctx || !ix || !out || argc < 0 || (argc > 1 && !argv)) return 0;
	*out = nullptr;
	const GdRefView R = ix->h.ref();
	const std::string s = gdb_header(R, gd_sam_header(R, ctx->rg_line, version, argc, argv));
	char *buf = (char *)malloc(s.size() + 1);
	if (!buf) return 0;
	memcpy(buf, s.data(), s.size()), buf[s.size()] = 0;
	*out = buf;
	return s.size();
}

// the same with an @HD line in front of the text
extern "C" size_t gdiet_hip_bam_header_so(gdiet_ctx *ctx, const gdiet_index *ix, const char *version, int argc, const char *const *argv, const char *sort_order, char **out)
{
	if (!ctx || !ix || !out || !sort_order || !*sort_order || argc < 0 || (argc > 1 && !argv)) return 0;
	*out = nullptr;
	for (const char *p = sort_order; *p; ++p)
		if (!((*p >= 'a' && *p <= 'z') || (*p >= 'A' && *p <= 'Z'))) return 0;
	const GdRefView R = ix->h.ref();
	const std::string s = gdb_header(R, std::string("@HD\tVN:1.6\tSO:") + sort_order + "\n" + gd_sam_header(R, ctx->rg_line, version, argc, argv));
	char *buf = (char *)malloc(s.size() + 1);
	if (!buf) return 0;
	memcpy(buf, s.data(), s.size()), buf[s.size()] = 0;
	*out = buf;
	return s.size();
}

extern "C" int64_t gdiet_hip_bam_batch_into(gdiet_ctx *ctx, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs, const char *const *quals,
                                            const char *const *comments, const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs, int64_t opt_flag, char **buf,
                                            size_t *cap)
{
	if (!gd_bam_args_ok(ctx, ix, n_reads, qnames, seqs, lens, n_regs, regs) || !buf || !cap) return GDIET_E_PARAM;
	gd_err_clear();
	std::lock_guard<std::mutex> lk(ctx->bam.mu);
	GdbPart &P = gd_bam_pool(ctx).all;
	std::string why;
	int rc = gd_bam_flatten(ctx, ix, n_reads, qnames, seqs, quals, comments, lens, n_regs, regs, opt_flag, P, why);
	if (rc) return why.empty() ? rc : gd_err_fail(ctx, rc, "gdiet_hip_bam_batch_into: " + why);
	const size_t tot = (size_t)P.bytes;
	if (tot == 0) return 0;
	if (!*buf || *cap < tot + 1) {
		const size_t want = tot + 1 + (tot >> 3);
		char *nb = (char *)realloc(*buf, want);
		if (!nb) return gd_err_fail(ctx, GDIET_E_NOMEM, "gdiet_hip_bam_batch_into: out of host memory");
		*buf = nb, *cap = want;
	}
	char *dst = *buf;
	rc = gd_bam_encode_device(ctx, P, nullptr, 0, why, [&](uint8_t *d_stream, size_t bytes, hipStream_t s) {
		const hipError_t e = hipMemcpyAsync(dst, d_stream, bytes, hipMemcpyDeviceToHost, s);
		if (e != hipSuccess) { why = std::string("device BAM encoder: copy down: ") + hipGetErrorString(e); return -1; }
		return 0;
	});
	if (rc) return gd_err_fail(ctx, GDIET_E_HIP, "gdiet_hip_bam_batch_into: " + why);
	dst[tot] = 0;
	return (int64_t)tot;
}

extern "C" int gdiet_hip_bgzf_out_write_bam(gdiet_bgzf_out *h, gdiet_ctx *ctx, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs,
                                            const char *const *quals, const char *const *comments, const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs,
                                            int64_t opt_flag)
{
	if (!h || !gd_bam_args_ok(ctx, ix, n_reads, qnames, seqs, lens, n_regs, regs) || (h->ctx && h->ctx != ctx)) return GDIET_E_PARAM;
	gd_err_clear();
	if (!h->ctx) { // a host writer: the records come down and go through write()
		char *buf = nullptr;
		size_t cap = 0;
		const int64_t n = gdiet_hip_bam_batch_into(ctx, ix, n_reads, qnames, seqs, quals, comments, lens, n_regs, regs, opt_flag, &buf, &cap);
		int rc = n < 0 ? (int)n : GDIET_OK;
		if (n > 0) rc = gd_bzo_done(h, h->w.write((const unsigned char *)buf, (size_t)n));
		free(buf);
		return rc;
	}
	if (h->w.failed || h->w.fd < 0) return gd_bzo_done(h, -1);
	std::lock_guard<std::mutex> lk(ctx->bam.mu);
	GdbPart &P = gd_bam_pool(ctx).all;
	std::string why;
	GdAccumHold held; // (nothing without an attached accumulator)
	if (held.take(h->acc, why)) return gd_err_fail(ctx, GDIET_E_PARAM, "gdiet_hip_bgzf_out_write_bam: " + why);
	int rc = gd_bam_flatten(ctx, ix, n_reads, qnames, seqs, quals, comments, lens, n_regs, regs, opt_flag, P, why);
	if (rc) return why.empty() ? rc : gd_err_fail(ctx, rc, "gdiet_hip_bgzf_out_write_bam: " + why);
	if (P.bytes == 0) return GDIET_OK;
	// the waiting tail in front, the records behind it; every whole member is compressed from there, the rest comes down as the next tail
	GdBgzfOut &w = h->w;
	std::vector<unsigned char> next_tail;
	int wrc = 0;
	rc = gd_bam_encode_device(ctx, P, w.tail.data(), w.tail.size(), why, [&](uint8_t *d_stream, size_t bytes, hipStream_t s) {
		if (gd_accum_enqueue_all(held, s, d_stream + w.tail.size(), P, why)) return -1; // from the records where they are, before they are compressed
		const size_t whole = bytes / GD_BGZF_MEMBER_IN * GD_BGZF_MEMBER_IN;
		next_tail.resize(bytes - whole);
		if (!next_tail.empty()) {
			const hipError_t e = hipMemcpyAsync(next_tail.data(), d_stream + whole, next_tail.size(), hipMemcpyDeviceToHost, s);
			if (e != hipSuccess) { why = std::string("device BAM encoder: tail copy down: ") + hipGetErrorString(e); return -1; }
		}
		wrc = w.members_resident(d_stream, whole); // (on the deflate driver's own stream, which it synchronises)
		return 0;
	});
	if (rc) { w.dev_error = true, (void)w.fail(why); return gd_bzo_done(h, -1); }
	if (wrc) return gd_bzo_done(h, wrc);
	w.tail.swap(next_tail);
	rc = gd_accum_verdict_all(held, why);
	return rc ? gd_err_fail(ctx, rc, "gdiet_hip_bgzf_out_write_bam: " + why) : GDIET_OK;
}

// measurement only (tools/map_file.py; not declared in include/gdiet_hip.h): the device's side of encoding BAM records since the context
// was created, in seconds: copy up, the encode kernel, and what followed it on the encoder's stream (copy down)
extern "C" int gdiet_hip_debug_bam_seconds(gdiet_ctx *ctx, double *out3)
{
	if (!ctx || !out3) return GDIET_E_PARAM;
	std::lock_guard<std::mutex> lk(ctx->bam.mu);
	for (int i = 0; i < 3; ++i) out3[i] = 1e-3 * ctx->bam.ms[i];
	return GDIET_OK;
}
