// Driver of the device mode of the reader (fastx_dev.hip.h); included by gdiet_hip.hip behind fastx_reader.h and map_pipeline.hip.h
// (needs gdiet_ctx, gdiet_read_batch, gd_parallel_for, GdFastx).  Two pieces:
//   GdFxExecutor::parse   a block of the file -> the record table of its strict prefix (count, scan, write, record pass);
//   (bam_in_driver.hip.h  a BAM block's records -> their text, on the device and in the chunk's arena: GdFxExecutor::bam_unpack)
//   gd_fx_build_batch     the reads read_batch selected -> a gdiet_read_batch, what gdiet_hip_batch_upload would have built of their
//                         strings: reads of device-parsed chunks are encoded by the encode kernel from the blocks that are already on
//                         the device, reads of host-parsed chunks by gd_nt4_encode and a copy, as before.
// Everything runs on the lane gdiet_ctx::fx (its stream, under its mutex); device memory is stream-ordered (GdStreamMem), except the
// scan's scratch buffer, which grows a few times at most.  The stream is synchronised before a table or a batch is handed out: the
// host reads the table next, and the lanes' streams read the batch.  Failures leave their text with the calling thread (gd_err_fail).
#pragma once
#include <hipcub/hipcub.hpp>
#include "fastx_dev.hip.h"
#include "bgzf_driver.hip.h" // the BGZF drivers and entry points: GdFxExecutor::inflate is one of their callers

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
		std::lock_guard<std::mutex> lk(B->ctx->fx.mu);
		(void)hipSetDevice(B->ctx->device);
		if (B->d_blk) (void)hipFreeAsync(B->d_blk, B->ctx->fx.stream);
		if (B->d_rec) (void)hipFreeAsync(B->d_rec, B->ctx->fx.stream);
	}
	delete B;
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
		GdLane &L = ctx->fx;
		std::lock_guard<std::mutex> lk(L.mu);
		std::string why;
		if (L.ready(ctx->device, 0, "device reader", why)) return gd_err_fail(ctx, -1, why);
		hipStream_t s = L.stream;
		hipError_t e = hipSuccess;
		const uint32_t n32 = (uint32_t)n, n_tiles = (n32 + GDX_TILE - 1) / GDX_TILE;
		GdStreamMem mem(s); // (a return without a table frees the block behind whatever was enqueued)
		uint8_t *d_blk;
		uint32_t *d_cnt, *d_nl; // d_cnt: counts[n_tiles + 1] | their scan[n_tiles + 1] | GdxMeta
		GdxRec *d_rec;
		auto fail = [&](hipError_t err, const char *what) {
			mem.fail();
			return (long)gd_err_fail(ctx, -1, std::string("device reader: ") + what + ": " + hipGetErrorString(err));
		};
		const size_t cnt_words = 2 * ((size_t)n_tiles + 1) + 2;
		if ((e = mem.alloc(&d_blk, (size_t)n_tiles * GDX_TILE)) != hipSuccess) return fail(e, "block");
		if ((e = mem.alloc(&d_cnt, sizeof(uint32_t) * cnt_words)) != hipSuccess) return fail(e, "counts");
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
		if (n_cand == 0) return 0;
		// the offset table is sized by the scanned count itself; the write pass checks every store against this capacity again
		const uint32_t cap = n_lines;
		if (n_lines > n32) return fail(hipErrorInvalidValue, "more newlines than bytes");
		if ((e = mem.alloc(&d_nl, sizeof(uint32_t) * (size_t)cap)) != hipSuccess) return fail(e, "offsets");
		if ((e = mem.alloc(&d_rec, sizeof(GdxRec) * (size_t)n_cand)) != hipSuccess) return fail(e, "records");
		hipLaunchKernelGGL(fastx_write_kernel, dim3(n_tiles), dim3(64), 0, s, (const uint8_t *)d_blk, n32, (const uint32_t *)d_off, d_nl, cap);
		hipLaunchKernelGGL(fastx_record_kernel, dim3((n_cand + 255) / 256), dim3(256), 0, s, (const uint8_t *)d_blk, (const uint32_t *)d_nl, n_cand, d_rec, d_meta);
		GdxMeta meta = {GDX_NONE, GDX_NONE};
		rec.resize(n_cand);
		if ((e = hipMemcpyAsync(rec.data(), d_rec, sizeof(GdxRec) * (size_t)n_cand, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "record table");
		if ((e = hipMemcpyAsync(&meta, d_meta, sizeof(GdxMeta), hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "record table");
		if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "record pass");
		if ((e = hipGetLastError()) != hipSuccess) return fail(e, "kernels");
		const uint32_t n_acc = meta.first_bad < n_cand ? meta.first_bad : n_cand;
		mem.free_now(d_cnt), mem.free_now(d_nl);
		rec.resize(n_acc);
		if (n_acc == 0) return 0;
		// every offset the host is going to use lies inside the block (the table came over a bus; the NULs are written by it)
		for (const GdxRec &R : rec)
			if ((uint64_t)R.qual_off + R.seq_len >= n || R.seq_off == 0 || (uint64_t)R.seq_off + R.seq_len >= n || (uint64_t)R.name_off + R.name_len >= n ||
			    (R.comment_off != GDX_NONE && (uint64_t)R.comment_off + R.comment_len >= n))
				return fail(hipErrorInvalidValue, "a record outside its block");
		GdFxBlock *B = new GdFxBlock{ctx, d_blk, d_rec};
		mem.release(d_blk), mem.release(d_rec); // the chunk's from here on
		dev = std::shared_ptr<void>((void *)B, gd_fx_block_free);
		return (long)n_acc;
	}
};

struct gdiet_fastx { GdFastx *r; gdiet_ctx *ctx = nullptr; };

// The batch of the reads the last read_batch handed out.  Called without fx.mu held.
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
		GdLane &L = ctx->fx;
		std::lock_guard<std::mutex> lk(L.mu);
		std::string why;
		if (L.ready(ctx->device, 0, "resident batch of the reader", why)) { delete b; return gd_err_fail(ctx, GDIET_E_HIP, why); }
		hipStream_t s = L.stream;
		hipError_t e = hipSuccess;
		GdStreamMem mem(s);
		GdxSeg *d_seg;
		uint8_t *d_uflag;
		auto fail = [&](hipError_t err, const char *what) {
			mem.fail();
			delete b;
			return gd_err_fail(ctx, GDIET_E_HIP, std::string("resident batch of the reader: ") + what + ": " + hipGetErrorString(err));
		};
		if ((e = mem.alloc(&b->d_reads, enc_len + 64)) != hipSuccess) return fail(e, "reads"); // (slack: the seed kernel reads aligned 8-byte words)
		if ((e = mem.alloc(&b->d_roff, sizeof(int64_t) * ((size_t)n + 1))) != hipSuccess) return fail(e, "offsets");
		if ((e = hipMemcpyAsync(b->d_roff, b->roff.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "offsets");
		if ((e = hipMemsetAsync((uint8_t *)b->d_reads + total, 0, 8 + 64, s)) != hipSuccess) return fail(e, "reads");
		memset(enc + total, 0, 8);
		for (const auto &h : host_runs) {
			const size_t o = (size_t)b->roff[h.first], len = (size_t)b->roff[h.second] - o;
			if (len && (e = hipMemcpyAsync((uint8_t *)b->d_reads + o, enc + o, len, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "host-parsed reads");
		}
		if (n_dev > 0) {
			uflag.assign((size_t)n, 0);
			if ((e = mem.alloc(&d_seg, sizeof(GdxSeg) * seg.size())) != hipSuccess) return fail(e, "runs");
			if ((e = mem.alloc(&d_uflag, (size_t)n)) != hipSuccess) return fail(e, "flags");
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
		mem.release(b->d_reads), mem.release(b->d_roff); // the batch's from here on (gdiet_hip_batch_destroy)
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
