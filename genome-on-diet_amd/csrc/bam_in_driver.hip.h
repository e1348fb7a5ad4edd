// Driver of the BAM unpack kernel (bam_in.hip.h); included by gdiet_hip.hip behind fastx_dev_driver.hip.h (needs gdiet_ctx, GdFxBlock,
// err_mark.h).  Two callers:
//   GdFxExecutor::bam_unpack    the attached reader: the block and the walk's rows up, the kernel, the text down in one copy into the
//                               chunk's arena; the device's copy of the text and a GdxRec table over it stay alive with the chunk
//                               (GdFxBlock), so gd_fx_build_batch encodes the resident batch from them like from a parsed FASTQ block.
//   gdiet_hip_bam_in_unpack     the kernel-level boundary: whole uncompressed records in, text and offsets out.
// Everything runs on the lane gdiet_ctx::fx with stream-ordered allocations (GdStreamMem), like the FASTQ passes; the stream is
// synchronised before the host touches the text.
#pragma once
#include "bam_in.hip.h"

// text[0, text_len) of rows[0, n_rows) over b[0, n).  keep != NULL: *keep takes the device's text and record table.  0, or -1 with why.
static int gd_bam_in_unpack_device(gdiet_ctx *ctx, const unsigned char *b, size_t n, const GdiRow *rows, size_t n_rows, uint64_t text_len, char *text, std::shared_ptr<void> *keep,
                                   std::string &why)
{
	if (n_rows == 0) return 0;
	std::vector<GdxRec> rec;
	if (keep) {
		rec.resize(n_rows);
		for (size_t k = 0; k < n_rows; ++k) {
			const GdiRow &r = rows[k];
			rec[k] = GdxRec{GDX_NONE, 0, GDX_NONE, 0, (uint32_t)r.dst, r.l_seq, (r.flags & GDI_NOQUAL) ? GDX_NONE : (uint32_t)(r.dst + r.l_seq + 1)};
		}
	}
	GdLane &L = ctx->fx;
	std::lock_guard<std::mutex> lk(L.mu);
	// the kernel takes every range from this table: none may leave its buffer
	if (!gdi_rows_inside(rows, n_rows, n, text_len) || text_len >= ((uint64_t)1 << 32)) {
		why = "BAM unpack: a table row outside its buffers";
		return gd_err_fail(ctx, -1, why);
	}
	if (L.ready(ctx->device, 0, "BAM unpack", why)) return gd_err_fail(ctx, -1, why);
	hipStream_t s = L.stream;
	hipError_t e = hipSuccess;
	GdStreamMem mem(s);
	uint8_t *d_blk, *d_text;
	GdiRow *d_rows;
	GdxRec *d_rec = nullptr;
	auto fail = [&](hipError_t err, const char *what) {
		mem.fail();
		why = std::string("BAM unpack: ") + what + ": " + hipGetErrorString(err);
		return gd_err_fail(ctx, -1, why);
	};
	if ((e = mem.alloc(&d_blk, n + 16)) != hipSuccess) return fail(e, "block");
	if ((e = mem.alloc(&d_text, (size_t)text_len + 16)) != hipSuccess) return fail(e, "text");
	if ((e = mem.alloc(&d_rows, sizeof(GdiRow) * n_rows)) != hipSuccess) return fail(e, "rows");
	if (keep && (e = mem.alloc(&d_rec, sizeof(GdxRec) * n_rows)) != hipSuccess) return fail(e, "records");
	if ((e = hipMemcpyAsync(d_blk, b, n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "block copy");
	if ((e = hipMemcpyAsync(d_rows, rows, sizeof(GdiRow) * n_rows, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "rows copy");
	if (keep && (e = hipMemcpyAsync(d_rec, rec.data(), sizeof(GdxRec) * n_rows, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "records copy");
	hipLaunchKernelGGL(bam_unpack_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s, (const GdiRow *)d_rows, (uint64_t)n_rows, (const uint8_t *)d_blk, (uint64_t)n, d_text,
	                   text_len);
	if ((e = hipGetLastError()) != hipSuccess) return fail(e, "launch");
	if ((e = hipMemcpyAsync(text, d_text, (size_t)text_len, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "text copy");
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "kernel");
	if (keep) {
		GdFxBlock *B = new GdFxBlock{ctx, d_text, d_rec};
		mem.release(d_text), mem.release(d_rec); // the chunk's from here on
		*keep = std::shared_ptr<void>((void *)B, gd_fx_block_free);
	}
	return 0;
}

extern "C" int gdiet_hip_bam_in_unpack(gdiet_ctx *ctx, const uint8_t *recs, size_t len, int with_qual, char *text, size_t text_cap, size_t *text_len, int64_t *off, int32_t *lens,
                                       int32_t *n_reads)
{
	if (!ctx || (!recs && len) || !text_len || !n_reads) return GDIET_E_PARAM;
	*text_len = 0, *n_reads = 0;
	gd_err_clear(); // (an earlier refusal on this thread is not this call's text)
	auto fail = [&](int rc, const std::string &what) { return gd_err_fail(ctx, rc, "gdiet_hip_bam_in_unpack: " + what); };
	if (len >= ((size_t)1 << 31)) return fail(GDIET_E_PARAM, "2 GiB of records or more");
	GdiWalk W;
	gdi_walk(recs, 0, len, with_qual != 0, false, 0, 0, W);
	if (W.bad) return fail(GDIET_E_PARAM, W.msg);
	if (W.pos != len) return fail(GDIET_E_PARAM, "offset " + std::to_string(W.pos) + ": the range ends inside a record");
	const size_t n = W.rows.size();
	if (n > 0x7fffffffu || W.text_len >= ((uint64_t)1 << 32)) return fail(GDIET_E_PARAM, "the records unpack to 4 GiB of text or more");
	*text_len = (size_t)W.text_len, *n_reads = (int32_t)n;
	if (!text && !off && !lens) return GDIET_OK; // sizes first
	if (!text || !off || !lens) return fail(GDIET_E_PARAM, "text, off and lens go together");
	if (W.text_len > text_cap) return fail(GDIET_E_PARAM, "the records unpack to " + std::to_string(W.text_len) + " bytes, text holds " + std::to_string(text_cap));
	std::string why;
	if (gd_bam_in_unpack_device(ctx, recs, len, W.rows.data(), n, W.text_len, text, nullptr, why) < 0) return GDIET_E_HIP; // (gd_err_fail has the text)
	for (size_t k = 0; k < n; ++k) {
		const GdiRow &R = W.rows[k];
		off[4 * k] = W.host[k].name_off, off[4 * k + 1] = W.host[k].aux_len ? (int64_t)W.host[k].aux_off : -1;
		off[4 * k + 2] = (int64_t)R.dst, off[4 * k + 3] = (R.flags & GDI_NOQUAL) ? -1 : (int64_t)(R.dst + R.l_seq + 1);
		lens[k] = (int32_t)R.l_seq;
	}
	return GDIET_OK;
}
