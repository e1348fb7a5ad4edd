// Driver of the device mode of the reader (fastx_dev.hip.h); included by gdiet_hip.hip behind fastx_reader.h and map_pipeline.hip.h
// (needs gdiet_ctx, gdiet_read_batch, gd_parallel_for, GdFastx).  Two pieces:
//   GdFxExecutor::parse   a block of the file -> the record table of its strict prefix (count, scan, write, record pass);
//   (bam_in_driver.hip.h  a BAM block's records -> their text, on the device and in the chunk's arena: GdFxExecutor::bam_unpack)
//   gd_fx_build_batch     the reads read_batch selected -> a gdiet_read_batch, what gdiet_hip_batch_upload would have built of their
//                         strings: reads of device-parsed chunks are encoded by the encode kernel from the blocks that are already on
//                         the device, reads of host-parsed chunks by gd_nt4_encode and a copy, as before.
// Everything runs on gdiet_ctx::fx_stream under gdiet_ctx::fx_mu; device memory is stream-ordered (a plain hipMalloc / hipFree would
// synchronise every batch in flight), except the scan's scratch buffer, which grows a few times at most.  The stream is synchronised
// before a table or a batch is handed out: the host reads the table next, and the lanes' streams read the batch.
#pragma once
#include <hipcub/hipcub.hpp>
#include "fastx_dev.hip.h"
#include "bgzf_inflate.hip.h"
#include "bgzf_deflate.hip.h"
#include "bgzf_out.h"
#include <fcntl.h>

static const char *gd_fx_err_of(const gdiet_ctx *ctx) { return ctx && gd_fx_failed_on == ctx ? ctx->fx_err.c_str() : nullptr; }
static int gd_fx_fail(gdiet_ctx *ctx, int rc, const std::string &what) // (the caller holds fx_mu)
{
	gd_ds_clear_mark();
	ctx->fx_err = what, gd_fx_failed_on = ctx; // (gd_fx_failed_on: map_diffstr_driver.hip.h)
	return rc;
}

// the device's copy of a block and of its record table; lives as GdFastxChunk::dev
struct GdFxBlock {
	gdiet_ctx *ctx;
	uint8_t *d_blk = nullptr;
	GdxRec *d_rec = nullptr;
};
static void gd_fx_block_free(void *p)
{
	GdFxBlock *B = (GdFxBlock *)p;
	{
		std::lock_guard<std::mutex> lk(B->ctx->fx_mu);
		(void)hipSetDevice(B->ctx->device);
		if (B->d_blk) (void)hipFreeAsync(B->d_blk, B->ctx->fx_stream);
		if (B->d_rec) (void)hipFreeAsync(B->d_rec, B->ctx->fx_stream);
	}
	delete B;
}

// BGZF members on the device (bgzf_inflate.hip.h): the raw members and their table up, one wavefront per member, the inflated range down
// into the block the reader asked for.  A stream and a lock of its own (gdiet_ctx::bz_stream, bz_mu): it runs on the reader's I/O thread
// while parse() holds fx_mu on the reader thread, and sharing fx_mu would put the two in sequence.  Stream-ordered allocations; the stream
// is synchronised before the host touches the bytes (it checks every member's length and CRC next).  Returns 0, -1 (the device failed)
// or -2 (a member's stream is not valid deflate), with the reason in why.
static int gd_bz_inflate_device(gdiet_ctx *ctx, const unsigned char *raw, size_t raw_len, const GdBgzfMember *m, size_t n, unsigned char *dst, size_t dst_len, uint32_t *out_len,
                                std::string &why)
{
	if (n == 0) return 0;
	for (size_t i = 0; i < n; ++i) // the kernel takes every range from this table: none may leave its buffer
		if (m[i].in_off > raw_len || m[i].in_len > raw_len - m[i].in_off || m[i].isize > GD_BGZF_MAX_ISIZE || m[i].out_off > dst_len || m[i].isize > dst_len - m[i].out_off) {
			why = "BGZF member " + std::to_string(i) + ": outside its buffers";
			return -2;
		}
	std::lock_guard<std::mutex> lk(ctx->bz_mu);
	(void)hipSetDevice(ctx->device);
	hipError_t e = hipSuccess;
	if (!ctx->bz_stream && (e = hipStreamCreateWithFlags(&ctx->bz_stream, hipStreamNonBlocking)) != hipSuccess) {
		why = std::string("device inflate: stream: ") + hipGetErrorString(e);
		return -1;
	}
	hipStream_t s = ctx->bz_stream;
	for (hipEvent_t &ev : ctx->bz_ev)
		if (!ev && (e = hipEventCreate(&ev)) != hipSuccess) { ev = nullptr; why = std::string("device inflate: event: ") + hipGetErrorString(e); return -1; }
	uint8_t *d_raw = nullptr, *d_out = nullptr;
	GdBgzfMember *d_tab = nullptr;
	GdzResult *d_res = nullptr;
	auto fail = [&](hipError_t err, const char *what) {
		(void)hipStreamSynchronize(s);
		if (d_raw) (void)hipFreeAsync(d_raw, s);
		if (d_out) (void)hipFreeAsync(d_out, s);
		if (d_tab) (void)hipFreeAsync(d_tab, s);
		if (d_res) (void)hipFreeAsync(d_res, s);
		why = std::string("device inflate: ") + what + ": " + hipGetErrorString(err);
		return -1;
	};
	std::vector<GdzResult> res(n);
	if ((e = hipMallocAsync((void **)&d_raw, raw_len + 16, s)) != hipSuccess) return fail(e, "members");
	if ((e = hipMallocAsync((void **)&d_out, dst_len + 16, s)) != hipSuccess) return fail(e, "output");
	if ((e = hipMallocAsync((void **)&d_tab, sizeof(GdBgzfMember) * n, s)) != hipSuccess) return fail(e, "table");
	if ((e = hipMallocAsync((void **)&d_res, sizeof(GdzResult) * n, s)) != hipSuccess) return fail(e, "results");
	(void)hipEventRecord(ctx->bz_ev[0], s);
	if ((e = hipMemcpyAsync(d_raw, raw, raw_len, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "members copy");
	if ((e = hipMemcpyAsync(d_tab, m, sizeof(GdBgzfMember) * n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "table copy");
	if ((e = hipMemsetAsync(d_res, 0xff, sizeof(GdzResult) * n, s)) != hipSuccess) return fail(e, "results");
	(void)hipEventRecord(ctx->bz_ev[1], s);
	hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((unsigned)n), dim3(64), 0, s, (const uint8_t *)d_raw, (const GdBgzfMember *)d_tab, (uint32_t)n, d_out, d_res);
	if ((e = hipGetLastError()) != hipSuccess) return fail(e, "launch");
	(void)hipEventRecord(ctx->bz_ev[2], s);
	if (dst_len && (e = hipMemcpyAsync(dst, d_out, dst_len, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "output copy");
	if ((e = hipMemcpyAsync(res.data(), d_res, sizeof(GdzResult) * n, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "results copy");
	(void)hipEventRecord(ctx->bz_ev[3], s);
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "kernel");
	for (int i = 0; i < 3; ++i) { // (for measurements: gdiet_hip_debug_bgzf_seconds)
		float ms = 0;
		if (hipEventElapsedTime(&ms, ctx->bz_ev[i], ctx->bz_ev[i + 1]) == hipSuccess) ctx->bz_ms[i] += ms;
	}
	(void)hipFreeAsync(d_raw, s), (void)hipFreeAsync(d_out, s), (void)hipFreeAsync(d_tab, s), (void)hipFreeAsync(d_res, s);
	for (size_t i = 0; i < n; ++i) {
		out_len[i] = res[i].out_len;
		if (res[i].rc != GDZ_OK) {
			why = "BGZF member " + std::to_string(i) + ": " + gdz_strerror(res[i].rc);
			return -2;
		}
	}
	return 0;
}

// BGZF members written on the device (bgzf_deflate.hip.h): in[0, in_len) up, one wavefront per member of 65280 input bytes into a slot
// of 65536 bytes, the members' lengths down, their prefix sum (on the host) up, the pack kernel, and one copy brings the file bytes
// out[0, *out_len) back.  A stream and a lock of its own (gdiet_ctx::bzd_stream, bzd_mu): a writer thread compresses the text of batch i
// while batch i + 1 maps and the reader inflates.  Stream-ordered allocations.  The stream is synchronised twice: once for the 8 bytes
// per member that the host's prefix sum needs (it also sizes the copy down), once before the host touches the bytes.  out_cap must be
// at least 65536 bytes per member.  Returns 0 or -1 (the device failed) with the reason in why.
// The middle of it: members from an input that is already resident, d_in[0, in_len) in device memory (the BAM route encodes its records
// there: bam_driver.hip.h).  The caller holds bzd_mu, has made the stream and the events (gd_bzd_ready) and recorded bzd_ev[0] and [1]
// around whatever brought the input up; d_in stays the caller's.  On failure the stream has been synchronised.
static int gd_bzd_ready(gdiet_ctx *ctx, std::string &why)
{
	(void)hipSetDevice(ctx->device);
	hipError_t e = hipSuccess;
	if (!ctx->bzd_stream && (e = hipStreamCreateWithFlags(&ctx->bzd_stream, hipStreamNonBlocking)) != hipSuccess) {
		why = std::string("device deflate: stream: ") + hipGetErrorString(e);
		return -1;
	}
	for (hipEvent_t &ev : ctx->bzd_ev)
		if (!ev && (e = hipEventCreate(&ev)) != hipSuccess) { ev = nullptr; why = std::string("device deflate: event: ") + hipGetErrorString(e); return -1; }
	return 0;
}
static int gd_bz_deflate_resident(gdiet_ctx *ctx, const uint8_t *d_in, size_t in_len, unsigned char *out, size_t out_cap, size_t *out_len, std::string &why)
{
	const size_t n = (in_len + GDD_MAX_IN - 1) / GDD_MAX_IN;
	hipStream_t s = ctx->bzd_stream;
	hipError_t e = hipSuccess;
	uint8_t *d_slots = nullptr, *d_out = nullptr;
	GddResult *d_res = nullptr;
	uint64_t *d_off = nullptr; // off[n], then len[n] as 32-bit words
	auto fail = [&](hipError_t err, const char *what) {
		(void)hipStreamSynchronize(s);
		if (d_slots) (void)hipFreeAsync(d_slots, s);
		if (d_out) (void)hipFreeAsync(d_out, s);
		if (d_res) (void)hipFreeAsync(d_res, s);
		if (d_off) (void)hipFreeAsync(d_off, s);
		why = std::string("device deflate: ") + what + ": " + hipGetErrorString(err);
		return -1;
	};
	std::vector<GddResult> res(n);
	if ((e = hipMallocAsync((void **)&d_slots, n * GDD_SLOT, s)) != hipSuccess) return fail(e, "slots");
	if ((e = hipMallocAsync((void **)&d_res, sizeof(GddResult) * n, s)) != hipSuccess) return fail(e, "results");
	if ((e = hipMemsetAsync(d_res, 0xff, sizeof(GddResult) * n, s)) != hipSuccess) return fail(e, "results");
	(void)hipEventRecord(ctx->bzd_ev[1], s);
	hipLaunchKernelGGL(bgzf_deflate_kernel, dim3((unsigned)n), dim3(64), 0, s, d_in, (uint64_t)in_len, (uint32_t)n, d_slots, d_res);
	if ((e = hipGetLastError()) != hipSuccess) return fail(e, "launch");
	(void)hipEventRecord(ctx->bzd_ev[2], s);
	if ((e = hipMemcpyAsync(res.data(), d_res, sizeof(GddResult) * n, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "results copy");
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "kernel");
	std::vector<uint64_t> tab(n + (n + 1) / 2);
	uint32_t *len = (uint32_t *)(tab.data() + n);
	size_t total = 0;
	for (size_t i = 0; i < n; ++i) { // the pack kernel takes every range from this table: none may leave its buffer
		if (res[i].rc != GDD_OK || res[i].member_len < 28 || res[i].member_len > GDD_SLOT) return fail(hipErrorInvalidValue, "a member's result");
		tab[i] = total, len[i] = res[i].member_len, total += res[i].member_len;
	}
	if (total > out_cap) return fail(hipErrorInvalidValue, "members larger than the output");
	if ((e = hipMallocAsync((void **)&d_off, sizeof(uint64_t) * tab.size(), s)) != hipSuccess) return fail(e, "offsets");
	if ((e = hipMallocAsync((void **)&d_out, total + 16, s)) != hipSuccess) return fail(e, "output");
	if ((e = hipMemcpyAsync(d_off, tab.data(), sizeof(uint64_t) * tab.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "offsets copy");
	(void)hipEventRecord(ctx->bzd_ev[3], s);
	hipLaunchKernelGGL(bgzf_pack_kernel, dim3((unsigned)n), dim3(256), 0, s, (const uint8_t *)d_slots, (const uint64_t *)d_off, (const uint32_t *)(d_off + n), (uint32_t)n, d_out);
	if ((e = hipGetLastError()) != hipSuccess) return fail(e, "pack launch");
	(void)hipEventRecord(ctx->bzd_ev[4], s);
	if ((e = hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "output copy");
	(void)hipEventRecord(ctx->bzd_ev[5], s);
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "pack kernel");
	{ // (for measurements: gdiet_hip_debug_bgzf_deflate_seconds)
		float ms = 0;
		if (hipEventElapsedTime(&ms, ctx->bzd_ev[0], ctx->bzd_ev[1]) == hipSuccess) ctx->bzd_ms[0] += ms;
		if (hipEventElapsedTime(&ms, ctx->bzd_ev[1], ctx->bzd_ev[2]) == hipSuccess) ctx->bzd_ms[1] += ms;
		if (hipEventElapsedTime(&ms, ctx->bzd_ev[3], ctx->bzd_ev[4]) == hipSuccess) ctx->bzd_ms[1] += ms;
		if (hipEventElapsedTime(&ms, ctx->bzd_ev[4], ctx->bzd_ev[5]) == hipSuccess) ctx->bzd_ms[2] += ms;
	}
	(void)hipFreeAsync(d_slots, s), (void)hipFreeAsync(d_out, s), (void)hipFreeAsync(d_res, s), (void)hipFreeAsync(d_off, s);
	*out_len = total;
	return 0;
}

static int gd_bz_deflate_device(gdiet_ctx *ctx, const unsigned char *in, size_t in_len, unsigned char *out, size_t out_cap, size_t *out_len, std::string &why)
{
	*out_len = 0;
	const size_t n = (in_len + GDD_MAX_IN - 1) / GDD_MAX_IN;
	if (n == 0) return 0;
	if (n > ((size_t)1 << 30) || out_cap / GDD_SLOT < n) { why = "device deflate: the output holds fewer than 65536 bytes per member"; return -1; }
	std::lock_guard<std::mutex> lk(ctx->bzd_mu);
	if (gd_bzd_ready(ctx, why)) return -1;
	hipStream_t s = ctx->bzd_stream;
	hipError_t e = hipSuccess;
	uint8_t *d_in = nullptr;
	auto fail = [&](hipError_t err, const char *what) {
		(void)hipStreamSynchronize(s);
		if (d_in) (void)hipFreeAsync(d_in, s);
		why = std::string("device deflate: ") + what + ": " + hipGetErrorString(err);
		return -1;
	};
	if ((e = hipMallocAsync((void **)&d_in, in_len + 16, s)) != hipSuccess) return fail(e, "input");
	(void)hipEventRecord(ctx->bzd_ev[0], s);
	if ((e = hipMemcpyAsync(d_in, in, in_len, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "input copy");
	const int rc = gd_bz_deflate_resident(ctx, d_in, in_len, out, out_cap, out_len, why);
	(void)hipFreeAsync(d_in, s);
	return rc;
}

// BAM records unpacked on the device (bam_in_driver.hip.h, included behind this file)
static int gd_bam_in_unpack_device(gdiet_ctx *ctx, const unsigned char *b, size_t n, const GdiRow *rows, size_t n_rows, uint64_t text_len, char *text, std::shared_ptr<void> *keep,
                                   std::string &why);

struct GdFxExecutor : GdFastxDevice {
	gdiet_ctx *ctx;
	explicit GdFxExecutor(gdiet_ctx *c) : ctx(c) {}
	int bam_unpack(const unsigned char *b, size_t n, const GdiRow *rows, size_t n_rows, uint64_t text_len, char *text, std::shared_ptr<void> &dev, std::string &why) override
	{
		return gd_bam_in_unpack_device(ctx, b, n, rows, n_rows, text_len, text, &dev, why);
	}
	int inflate(const unsigned char *raw, size_t raw_len, const GdBgzfMember *m, size_t n, unsigned char *dst, size_t dst_len, uint32_t *out_len, std::string &why) override
	{
		return gd_bz_inflate_device(ctx, raw, raw_len, m, n, dst, dst_len, out_len, why);
	}
	long parse(const unsigned char *b, size_t n, std::vector<GdxRec> &rec, std::shared_ptr<void> &dev) override
	{
		rec.clear(), dev.reset();
		if (n == 0 || n >= ((size_t)1 << 31)) return 0;
		std::lock_guard<std::mutex> lk(ctx->fx_mu);
		(void)hipSetDevice(ctx->device);
		hipError_t e = hipSuccess;
		if (!ctx->fx_stream && (e = hipStreamCreateWithFlags(&ctx->fx_stream, hipStreamNonBlocking)) != hipSuccess)
			return gd_fx_fail(ctx, -1, std::string("device reader: stream: ") + hipGetErrorString(e));
		hipStream_t s = ctx->fx_stream;
		const uint32_t n32 = (uint32_t)n, n_tiles = (n32 + GDX_TILE - 1) / GDX_TILE;
		uint8_t *d_blk = nullptr;
		uint32_t *d_cnt = nullptr, *d_nl = nullptr; // d_cnt: counts[n_tiles + 1] | their scan[n_tiles + 1] | GdxMeta
		GdxRec *d_rec = nullptr;
		auto drop = [&]() { // (stream-ordered: whatever was enqueued finishes first)
			if (d_blk) (void)hipFreeAsync(d_blk, s);
			if (d_cnt) (void)hipFreeAsync(d_cnt, s);
			if (d_nl) (void)hipFreeAsync(d_nl, s);
			if (d_rec) (void)hipFreeAsync(d_rec, s);
			d_blk = nullptr, d_cnt = nullptr, d_nl = nullptr, d_rec = nullptr;
		};
		auto fail = [&](hipError_t err, const char *what) {
			(void)hipStreamSynchronize(s);
			drop();
			return (long)gd_fx_fail(ctx, -1, std::string("device reader: ") + what + ": " + hipGetErrorString(err));
		};
		const size_t cnt_words = 2 * ((size_t)n_tiles + 1) + 2;
		if ((e = hipMallocAsync((void **)&d_blk, (size_t)n_tiles * GDX_TILE, s)) != hipSuccess) return fail(e, "block");
		if ((e = hipMallocAsync((void **)&d_cnt, sizeof(uint32_t) * cnt_words, s)) != hipSuccess) return fail(e, "counts");
		uint32_t *d_off = d_cnt + n_tiles + 1;
		GdxMeta *d_meta = (GdxMeta *)(d_off + n_tiles + 1);
		if ((e = hipMemcpyAsync(d_blk, b, n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "block copy");
		if ((e = hipMemsetAsync(d_cnt + n_tiles, 0, sizeof(uint32_t), s)) != hipSuccess) return fail(e, "counts");
		if ((e = hipMemsetAsync(d_meta, 0xff, sizeof(GdxMeta), s)) != hipSuccess) return fail(e, "counts");
		hipLaunchKernelGGL(fastx_count_kernel, dim3(n_tiles), dim3(64), 0, s, (const uint8_t *)d_blk, n32, d_cnt, d_meta);
		size_t sb = 0;
		if ((e = hipcub::DeviceScan::ExclusiveSum(nullptr, sb, d_cnt, d_off, (int)(n_tiles + 1), s)) != hipSuccess) return fail(e, "scan");
		if (sb + 64 > ctx->fx_scan.cap) { // (rare: the first blocks; older scans on this stream have completed once it is synchronised)
			if ((e = hipStreamSynchronize(s)) != hipSuccess || (e = ctx->fx_scan.release()) != hipSuccess) return fail(e, "scan buffer");
			const size_t want = 2 * sb + 4096;
			if ((e = hipMalloc(&ctx->fx_scan.p, want)) != hipSuccess) { (void)hipGetLastError(); ctx->fx_scan.p = nullptr; return fail(e, "scan buffer"); }
			ctx->fx_scan.kind = DevBuf::DEVICE, ctx->fx_scan.cap = want;
		}
		sb = ctx->fx_scan.cap;
		if ((e = hipcub::DeviceScan::ExclusiveSum(ctx->fx_scan.p, sb, d_cnt, d_off, (int)(n_tiles + 1), s)) != hipSuccess) return fail(e, "scan");
		uint32_t n_lines = 0;
		if ((e = hipMemcpyAsync(&n_lines, d_off + n_tiles, sizeof(uint32_t), hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "line count");
		if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "count pass");
		const uint32_t n_cand = n_lines / 4; // groups of four complete lines
		if (n_cand == 0) { drop(); return 0; }
		// the offset table is sized by the scanned count itself; the write pass checks every store against this capacity again
		const uint32_t cap = n_lines;
		if (n_lines > n32) return fail(hipErrorInvalidValue, "more newlines than bytes");
		if ((e = hipMallocAsync((void **)&d_nl, sizeof(uint32_t) * (size_t)cap, s)) != hipSuccess) return fail(e, "offsets");
		if ((e = hipMallocAsync((void **)&d_rec, sizeof(GdxRec) * (size_t)n_cand, s)) != hipSuccess) return fail(e, "records");
		hipLaunchKernelGGL(fastx_write_kernel, dim3(n_tiles), dim3(64), 0, s, (const uint8_t *)d_blk, n32, (const uint32_t *)d_off, d_nl, cap);
		hipLaunchKernelGGL(fastx_record_kernel, dim3((n_cand + 255) / 256), dim3(256), 0, s, (const uint8_t *)d_blk, (const uint32_t *)d_nl, n_cand, d_rec, d_meta);
		GdxMeta meta = {GDX_NONE, GDX_NONE};
		rec.resize(n_cand);
		if ((e = hipMemcpyAsync(rec.data(), d_rec, sizeof(GdxRec) * (size_t)n_cand, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "record table");
		if ((e = hipMemcpyAsync(&meta, d_meta, sizeof(GdxMeta), hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "record table");
		if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "record pass");
		if ((e = hipGetLastError()) != hipSuccess) return fail(e, "kernels");
		const uint32_t n_acc = meta.first_bad < n_cand ? meta.first_bad : n_cand;
		(void)hipFreeAsync(d_cnt, s), (void)hipFreeAsync(d_nl, s);
		d_cnt = nullptr, d_nl = nullptr;
		rec.resize(n_acc);
		if (n_acc == 0) { drop(); return 0; }
		// every offset the host is going to use lies inside the block (the table came over a bus; the NULs are written by it)
		for (const GdxRec &R : rec)
			if ((uint64_t)R.qual_off + R.seq_len >= n || R.seq_off == 0 || (uint64_t)R.seq_off + R.seq_len >= n || (uint64_t)R.name_off + R.name_len >= n ||
			    (R.comment_off != GDX_NONE && (uint64_t)R.comment_off + R.comment_len >= n))
				return fail(hipErrorInvalidValue, "a record outside its block");
		GdFxBlock *B = new GdFxBlock{ctx, d_blk, d_rec};
		dev = std::shared_ptr<void>((void *)B, gd_fx_block_free);
		return (long)n_acc;
	}
};

struct gdiet_fastx { GdFastx *r; gdiet_ctx *ctx = nullptr; };

// The batch of the reads the last read_batch handed out.  Called without fx_mu held.
static int gd_fx_build_batch(gdiet_ctx *ctx, GdFastx &R, gdiet_read_batch **out)
{
	const int n = (int)R.v_len.size();
	gdiet_read_batch *b = new gdiet_read_batch();
	b->n = n;
	b->roff.assign((size_t)n + 1, 0);
	for (int i = 0; i < n; ++i) b->roff[i + 1] = b->roff[i] + (R.v_len[i] > 0 ? R.v_len[i] : 0);
	const size_t total = (size_t)b->roff[n], enc_len = total + 8;
	{
		std::lock_guard<std::mutex> lk(ctx->enc_mu);
		if (!ctx->enc_pool.empty()) b->enc.swap(ctx->enc_pool.back()), ctx->enc_pool.pop_back();
	}
	if (b->enc.size() < enc_len) b->enc.resize(enc_len + (enc_len >> 3));
	// runs of consecutive records of one device chunk, and the reads the host parsed
	std::vector<GdxSeg> seg;
	std::vector<std::pair<int, int>> host_runs; // [first, last)
	int n_dev = 0;
	for (int i = 0; i < n;) {
		const GdFastxChunk &C = *R.lent[(size_t)R.v_chunk[i]];
		int j = i + 1;
		while (j < n && R.v_chunk[j] == R.v_chunk[i] && R.v_rec[j] == R.v_rec[j - 1] + 1) ++j;
		if (C.on_device && C.dev) {
			const GdFxBlock *B = (const GdFxBlock *)C.dev.get();
			seg.push_back(GdxSeg{B->d_blk, B->d_rec, R.v_rec[i], i, n_dev, 0});
			n_dev += j - i;
		} else if (!host_runs.empty() && host_runs.back().second == i) host_runs.back().second = j;
		else host_runs.push_back(std::make_pair(i, j));
		i = j;
	}
	uint8_t *enc = b->enc.data();
	if (!host_runs.empty())
		gd_parallel_for(ctx, ctx->host_threads, (int)host_runs.size(), [&](int k) {
			for (int i = host_runs[(size_t)k].first; i < host_runs[(size_t)k].second; ++i)
				if (R.v_len[i] > 0) gd_nt4_encode(R.v_seq[i], enc + b->roff[i], (size_t)R.v_len[i]);
		});
	std::vector<uint8_t> uflag;
	{
		std::lock_guard<std::mutex> lk(ctx->fx_mu);
		(void)hipSetDevice(ctx->device);
		hipError_t e = hipSuccess;
		GdxSeg *d_seg = nullptr;
		uint8_t *d_uflag = nullptr;
		auto fail = [&](hipError_t err, const char *what) {
			if (ctx->fx_stream) (void)hipStreamSynchronize(ctx->fx_stream);
			if (d_seg) (void)hipFreeAsync(d_seg, ctx->fx_stream);
			if (d_uflag) (void)hipFreeAsync(d_uflag, ctx->fx_stream);
			if (b->d_reads) (void)hipFreeAsync(b->d_reads, ctx->fx_stream);
			if (b->d_roff) (void)hipFreeAsync(b->d_roff, ctx->fx_stream);
			delete b;
			return gd_fx_fail(ctx, GDIET_E_HIP, std::string("resident batch of the reader: ") + what + ": " + hipGetErrorString(err));
		};
		if (!ctx->fx_stream && (e = hipStreamCreateWithFlags(&ctx->fx_stream, hipStreamNonBlocking)) != hipSuccess) return fail(e, "stream");
		hipStream_t s = ctx->fx_stream;
		if ((e = hipMallocAsync(&b->d_reads, enc_len + 64, s)) != hipSuccess) return fail(e, "reads"); // (slack: the seed kernel reads aligned 8-byte words)
		if ((e = hipMallocAsync(&b->d_roff, sizeof(int64_t) * ((size_t)n + 1), s)) != hipSuccess) return fail(e, "offsets");
		if ((e = hipMemcpyAsync(b->d_roff, b->roff.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "offsets");
		if ((e = hipMemsetAsync((uint8_t *)b->d_reads + total, 0, 8 + 64, s)) != hipSuccess) return fail(e, "reads");
		memset(enc + total, 0, 8);
		for (const auto &h : host_runs) {
			const size_t o = (size_t)b->roff[h.first], len = (size_t)b->roff[h.second] - o;
			if (len && (e = hipMemcpyAsync((uint8_t *)b->d_reads + o, enc + o, len, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "host-parsed reads");
		}
		if (n_dev > 0) {
			uflag.assign((size_t)n, 0);
			if ((e = hipMallocAsync((void **)&d_seg, sizeof(GdxSeg) * seg.size(), s)) != hipSuccess) return fail(e, "runs");
			if ((e = hipMallocAsync((void **)&d_uflag, (size_t)n, s)) != hipSuccess) return fail(e, "flags");
			if ((e = hipMemcpyAsync(d_seg, seg.data(), sizeof(GdxSeg) * seg.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "runs");
			if ((e = hipMemsetAsync(d_uflag, 0, (size_t)n, s)) != hipSuccess) return fail(e, "flags");
			hipLaunchKernelGGL(fastx_encode_kernel, dim3((unsigned)n_dev), dim3(64), 0, s, (int32_t)n_dev, (int32_t)seg.size(), (const GdxSeg *)d_seg, (const int64_t *)b->d_roff,
			                   (uint8_t *)b->d_reads, d_uflag);
			// the host copy gd_stage_records reads: one copy of all of it (the host-parsed stretches come back as they went)
			if (total && (e = hipMemcpyAsync(enc, b->d_reads, total, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "host copy");
			if ((e = hipMemcpyAsync(uflag.data(), d_uflag, (size_t)n, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "flags");
		}
		if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "encode pass"); // the lanes' streams read the batch next
		if ((e = hipGetLastError()) != hipSuccess) return fail(e, "encode kernel");
		if (d_seg) (void)hipFreeAsync(d_seg, s);
		if (d_uflag) (void)hipFreeAsync(d_uflag, s);
	}
	// the host strings of the reads the encode kernel flagged: U -> T (kseq2bseq, LR/bseq.c:71-73)
	for (int i = 0; i < n && !uflag.empty(); ++i)
		if (uflag[(size_t)i]) {
			char *q = const_cast<char *>(R.v_seq[i]);
			for (int32_t k = 0; k < R.v_len[i]; ++k) if (gdx_is_u((unsigned char)q[k])) --q[k];
		}
	*out = b;
	return GDIET_OK;
}

// after a batch has been handed out (and built): a device chunk whose records are all handed out needs its device copy no more
static void gd_fx_release_done(GdFastx &R)
{
	for (auto &c : R.lent)
		if (c->on_device && c->dev && c->next >= c->len.size()) c->dev.reset();
}
