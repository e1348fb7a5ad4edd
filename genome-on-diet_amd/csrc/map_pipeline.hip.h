// B1: batch driver of the per-read mapping path.  Included at the end of gdiet_hip.hip (needs gdiet_ctx, GD_HIP, gd_grow).
//   host threads : encode reads, candidate linking + DP boxes (gd_lr_link_and_boxes), post-processing (gd_lr_finish)
//   device       : map_seed_kernel -> map_vote_kernel -> map_gather_kernel -> ksw batch (exact-match, DP, backtrack)
// gd_map_range is a sequence of stages (gd_stage_setup, _seed, _vote, _boxes_device / _boxes_host, gd_upload_boxes, gd_stage_dp, _pack,
// _records) over one GdMapCall; their host arithmetic -- capacity classes, scratch layout, box tables, failed reads -- is map_plan.h,
// which has no HIP in it and is tested on the CPU (tests/test_map_plan.py).
#pragma once
#include <atomic>
#include <memory>
#include <cstddef>
#include <chrono>
#include <thread>
#include <mutex>
#include "map_host.h"
#include "map_plan.h"
#include "map_index.h"
#include "map_kernels.hip.h"

struct gdiet_index {
	GdIndex h;
	void *d_tkey = nullptr, *d_tval = nullptr, *d_pos = nullptr, *d_S = nullptr;
	GdIdxView dview;
	// device-built index (map_index_dev.hip.h): the table exists on the device only until someone asks for the host copies
	bool host_tables = true;
	uint32_t *d_cnt_sorted = nullptr; // occurrence counts of the keys, ascending (mm_idx_cal_max_occ)
	uint64_t n_pos = 0;
	// contig table on the device (lengths, offsets into S), made on first use by the device-side box stage of the ShortReads variant
	uint32_t *d_seq_len = nullptr;
	uint64_t *d_seq_off = nullptr;
	std::mutex seq_mu;
	// gdiet_hip_index_info: the sequence table as C arrays, made on first use (under seq_mu); gdiet_hip_index_open_stats: the counters of
	// the gdiet_hip_index_open that made this index (ref_fasta_driver.hip.h), zero for any other
	std::vector<const char *> info_names;
	std::vector<uint32_t> info_lens;
	int64_t open_counts[6] = {0, 0, 0, 0, 0, 0};
	double open_seconds[5] = {0, 0, 0, 0, 0};
	uint64_t open_peak = 0;
};

struct gdiet_read_batch {
	int n = 0;
	std::vector<int64_t> roff;          // n+1
	std::vector<uint8_t> enc;           // nt4, forward strand, all reads packed (host copy for post-processing)
	void *d_reads = nullptr, *d_roff = nullptr;
};

#include "map_index_dev.hip.h"

#include "host_pool.h"
#include "nt4_encode.h"

static void gd_pool_free(void *pool) { delete (GdPool *)pool; }

static GdPool *gd_pool(gdiet_ctx *ctx)
{
	gdiet_ctx *owner = ctx->parent ? ctx->parent : ctx; // an async lane works in its parent's pool
	static std::mutex create_mu; // (taken on every call: a handful per batch; a plain pointer must not be double-checked without it)
	std::lock_guard<std::mutex> lk(create_mu);
	if (!owner->pool) owner->pool = new GdPool();
	return (GdPool *)owner->pool;
}

template <class F> static void gd_parallel_for(gdiet_ctx *ctx, int n_threads, int n, F f) { gd_pool(ctx)->run(n_threads, n, f); }


static int gd_index_upload(gdiet_ctx *ctx, gdiet_index *ix)
{
	GdIndex &h = ix->h;
	auto up = [&](void **d, const void *src, size_t bytes) -> int {
		if (bytes == 0) bytes = 8;
		GD_HIP(hipMalloc(d, bytes));
		if (src) GD_HIP(hipMemcpy(*d, src, bytes, hipMemcpyHostToDevice));
		return GDIET_OK;
	};
	int rc;
	if ((rc = up(&ix->d_tkey, h.tkey.data(), h.tkey.size() * 8))) return rc;
	if ((rc = up(&ix->d_tval, h.tval.data(), h.tval.size() * 8))) return rc;
	if ((rc = up(&ix->d_pos, h.pos.empty() ? nullptr : h.pos.data(), h.pos.size() * 8))) return rc;
	if ((rc = up(&ix->d_S, h.S.empty() ? nullptr : h.S.data(), h.S.size() * 4 + 8))) return rc;
	ix->dview.k = h.k, ix->dview.w = h.w, ix->dview.tbits = h.tbits;
	ix->dview.tkey = (const uint64_t *)ix->d_tkey, ix->dview.tval = (const uint64_t *)ix->d_tval, ix->dview.pos = (const uint64_t *)ix->d_pos;
	return GDIET_OK;
}

extern "C" int gdiet_hip_index_build(gdiet_ctx *ctx, gdiet_index **out, int n_seq, const char *const *names, const char *const *seqs,
                                     const uint32_t *lens, int k, int w, const char *pattern, int pattern_len, int n_threads)
{
	if (!ctx || !out || n_seq <= 0 || !seqs || !lens) return GDIET_E_PARAM;
	(void)hipSetDevice(ctx->device);
	GdPattern P;
	if (!gd_pattern_init(P, pattern, pattern_len)) { ctx->err = "bad pattern"; return GDIET_E_PARAM; }
	if (w <= 0 || w > GDM_MAX_W || k <= 0 || k > 28) { ctx->err = "k must be in [1,28] and w in [1,64]"; return GDIET_E_PARAM; }
	gdiet_index *ix = new gdiet_index();
	std::vector<std::string> nm(n_seq);
	std::vector<GdSeqSpan> sq(n_seq);
	for (int i = 0; i < n_seq; ++i) nm[i] = names && names[i] ? names[i] : "", sq[i].p = seqs[i], sq[i].n = lens[i];
	const int nt = n_threads > 0 ? n_threads : gd_effective_cpus();
	if (ctx->index_on_device) { // sketch, sort and table build on the GPU (map_index_dev.hip.h); GDIET_INDEX_BUILD=host selects the host builder
		if (!gd_index_build_device(ix, nm, sq, k, w, P, nt, ctx->stream, ctx->err)) { gdiet_hip_index_destroy(ctx, ix); return GDIET_E_HIP; }
		*out = ix;
		return GDIET_OK;
	}
	gd_index_build(ix->h, nm, sq, k, w, P, nt, true);
	int rc = gd_index_upload(ctx, ix);
	if (rc) { delete ix; return rc; }
	*out = ix;
	return GDIET_OK;
}

extern "C" int gdiet_hip_index_import(gdiet_ctx *ctx, gdiet_index **out, int k, int w, const char *pattern, int pattern_len, int n_seq,
                                      const char *const *names, const uint32_t *lens, const uint64_t *offsets, const uint32_t *S,
                                      uint64_t n_keys, const uint64_t *keys, const uint32_t *cnt, const uint64_t *pos)
{
	if (!ctx || !out || n_seq <= 0 || !lens || !offsets || !S || !keys || !cnt || !pos) return GDIET_E_PARAM;
	(void)hipSetDevice(ctx->device);
	GdPattern P;
	if (!gd_pattern_init(P, pattern, pattern_len)) { ctx->err = "bad pattern"; return GDIET_E_PARAM; }
	if (w <= 0 || w > GDM_MAX_W || k <= 0 || k > 28) { ctx->err = "k must be in [1,28] and w in [1,64]"; return GDIET_E_PARAM; }
	gdiet_index *ix = new gdiet_index();
	gd_index_from_flat(ix->h, k, w, P, n_seq, names, lens, offsets, S, n_keys, keys, cnt, pos);
	int rc = gd_index_upload(ctx, ix);
	if (rc) { delete ix; return rc; }
	*out = ix;
	return GDIET_OK;
}

// flat view of the index, the inverse of gdiet_hip_index_import (keys in table order; each position list ascending)
extern "C" int gdiet_hip_index_export(const gdiet_index *ix, uint64_t *n_keys, uint64_t *n_pos, uint64_t *n_S_words, uint64_t *keys,
                                      uint32_t *cnt, uint64_t *pos, uint32_t *S, uint64_t *offsets)
{
	if (!ix) return GDIET_E_PARAM;
	{ std::string e; if (!gd_index_fetch_host(const_cast<gdiet_index *>(ix), e)) return GDIET_E_HIP; }
	const GdIndex &h = ix->h;
	if (n_keys) *n_keys = h.n_keys;
	if (n_pos) *n_pos = h.pos.size();
	if (n_S_words) *n_S_words = h.S.size();
	if (keys && cnt) {
		uint64_t j = 0;
		for (size_t s = 0; s < h.tkey.size(); ++s)
			if (h.tkey[s] != UINT64_MAX) keys[j] = h.tkey[s], cnt[j] = (uint32_t)h.tval[s], ++j;
		if (j != h.n_keys) return GDIET_E_PARAM;
	}
	if (pos && keys && cnt) { // lists concatenated in the order of keys[]
		uint64_t o = 0;
		for (size_t s = 0; s < h.tkey.size(); ++s)
			if (h.tkey[s] != UINT64_MAX) {
				const uint64_t st = h.tval[s] >> 32, n = (uint32_t)h.tval[s];
				for (uint64_t t = 0; t < n; ++t) pos[o++] = h.pos[st + t];
			}
	}
	if (S) memcpy(S, h.S.data(), 4 * h.S.size());
	if (offsets) for (size_t i = 0; i < h.seq.size(); ++i) offsets[i] = h.seq[i].offset;
	return GDIET_OK;
}

// ---- .mmi files: parser / writer in map_index.h (gd_index_read_mmi / gd_index_write_mmi) ---------------------------------------
extern "C" int gdiet_hip_index_load_mmi(gdiet_ctx *ctx, gdiet_index **out, const char *path, const char *pattern, int pattern_len)
{
	if (!ctx || !out || !path) return GDIET_E_PARAM;
	(void)hipSetDevice(ctx->device);
	GdPattern P;
	if (!gd_pattern_init(P, pattern, pattern_len)) { ctx->err = "bad pattern"; return GDIET_E_PARAM; }
	gdiet_index *ix = new gdiet_index();
	if (!gd_index_read_mmi(ix->h, path, P, ctx->err)) { delete ix; return GDIET_E_PARAM; }
	if (ix->h.w <= 0 || ix->h.w > GDM_MAX_W || ix->h.k <= 0 || ix->h.k > 28) { // the sketch kernels' windows are sized for these (gdiet_hip_index_build)
		ctx->err = std::string(path) + ": k must be in [1,28] and w in [1,64]";
		delete ix;
		return GDIET_E_PARAM;
	}
	int rc = gd_index_upload(ctx, ix);
	if (rc) { delete ix; return rc; }
	*out = ix;
	return GDIET_OK;
}

extern "C" int gdiet_hip_index_dump_mmi(gdiet_ctx *ctx, const gdiet_index *ix, const char *path, int bucket_bits)
{
	if (!ctx || !ix || !path || bucket_bits < 1 || bucket_bits > 28) return GDIET_E_PARAM;
	if (!gd_index_fetch_host(const_cast<gdiet_index *>(ix), ctx->err)) return GDIET_E_HIP;
	return gd_index_write_mmi(ix->h, path, bucket_bits, ctx->err) ? GDIET_OK : GDIET_E_PARAM;
}

extern "C" void gdiet_hip_index_destroy(gdiet_ctx *ctx, gdiet_index *ix)
{
	if (!ix) return;
	if (ctx) (void)hipSetDevice(ctx->device);
	void *p[] = {ix->d_tkey, ix->d_tval, ix->d_pos, ix->d_S, ix->d_cnt_sorted, ix->d_seq_len, ix->d_seq_off};
	for (void *q : p) if (q) (void)hipFree(q);
	delete ix;
}

extern "C" int32_t gdiet_hip_index_cal_max_occ(const gdiet_index *ix, float frac)
{
	if (!ix) return 0;
	if (ix->host_tables) return gd_index_cal_max_occ(ix->h, frac);
	// device-built: the counts are on the device, sorted; mm_idx_cal_max_occ (LR/index.c:190-210) is their (1-f) quantile + 1
	if (frac <= 0.) return INT32_MAX;
	const size_t n = ix->h.n_keys;
	if (n == 0) return 1;
	size_t kk = (size_t)(uint32_t)((1. - frac) * n);
	if (kk >= n) kk = n - 1;
	uint32_t v = 0;
	if (hipMemcpy(&v, ix->d_cnt_sorted + kk, 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
	return (int32_t)(v + 1);
}
extern "C" uint64_t gdiet_hip_index_n_keys(const gdiet_index *ix) { return ix ? ix->h.n_keys : 0; }

extern "C" int gdiet_hip_set_host_threads(gdiet_ctx *ctx, int n)
{
	if (!ctx || n < 1) return GDIET_E_PARAM;
	ctx->host_threads = n;
	return GDIET_OK;
}

// batches whose seed stage overflowed its first scratch layout and ran again with the hard bound (process-wide: lanes are contexts of their own)
static std::atomic<int64_t> gd_scratch_retries{0};
extern "C" int64_t gdiet_hip_map_scratch_retries(void) { return gd_scratch_retries.load(); }

extern "C" int gdiet_hip_map_stage_seconds(const gdiet_ctx *ctx, double out[6])
{
	if (!ctx || !out) return GDIET_E_PARAM;
	for (int i = 0; i < 6; ++i) out[i] = ctx->stage_s[i];
	return GDIET_OK;
}

extern "C" int gdiet_hip_batch_upload(gdiet_ctx *ctx, gdiet_read_batch **out, int n, const char *const *seqs, const int32_t *lens)
{
	gd_err_clear();
	if (!ctx || !out || n < 0 || (n && (!seqs || !lens))) return GDIET_E_PARAM;
	(void)hipSetDevice(ctx->device);
	const bool trace = gd_trace_stages();
	double t_[5] = {gd_now(), 0, 0, 0, 0};
	gdiet_read_batch *b = new gdiet_read_batch();
	b->n = n;
	b->roff.assign(n + 1, 0);
	for (int i = 0; i < n; ++i) b->roff[i + 1] = b->roff[i] + (lens[i] > 0 ? lens[i] : 0);
	// the host copy of the encoded reads lives in a buffer taken from the context's pool (returned by gdiet_hip_batch_destroy): first
	// touch of fresh memory -- 77 MB per HiFi mini-batch -- cost ten times the encoding itself
	const size_t enc_len = (size_t)b->roff[n] + 8;
	{
		std::lock_guard<std::mutex> lk(ctx->enc_mu);
		if (!ctx->enc_pool.empty()) b->enc.swap(ctx->enc_pool.back()), ctx->enc_pool.pop_back();
	}
	if (b->enc.size() < enc_len) b->enc.resize(enc_len + (enc_len >> 3));
	t_[1] = gd_now();
	gd_parallel_for(ctx, ctx->host_threads, n, [&](int i) {
		if (lens[i] > 0) gd_nt4_encode(seqs[i], b->enc.data() + b->roff[i], (size_t)lens[i]);
	});
	t_[2] = gd_now();
	// stream-ordered allocation: a plain hipMalloc / hipFree per mini-batch synchronises the whole device, i.e. every batch in flight
	GdStreamMem mem(ctx->stream);
	hipError_t e = mem.alloc(&b->d_reads, enc_len + 64); // (slack: the seed kernel reads aligned 8-byte words)
	if (e == hipSuccess) e = mem.alloc(&b->d_roff, sizeof(int64_t) * (n + 1));
	if (e == hipSuccess) e = hipMemcpyAsync(b->d_reads, b->enc.data(), enc_len, hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(b->d_roff, b->roff.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, ctx->stream);
	t_[3] = gd_now();
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	t_[4] = gd_now();
	if (trace) fprintf(stderr, "[gdiet upload, ms] n=%d alloc %.2f encode %.2f enqueue %.2f sync %.2f\n", n, 1e3 * (t_[1] - t_[0]), 1e3 * (t_[2] - t_[1]), 1e3 * (t_[3] - t_[2]), 1e3 * (t_[4] - t_[3]));
	if (e != hipSuccess) { mem.fail(); ctx->err = std::string("batch upload: ") + hipGetErrorString(e); delete b; return GDIET_E_HIP; } // (a copy may still read b->enc)
	mem.release(b->d_reads), mem.release(b->d_roff); // the batch's from here on (gdiet_hip_batch_destroy)
	*out = b;
	return GDIET_OK;
}

extern "C" void gdiet_hip_batch_destroy(gdiet_ctx *ctx, gdiet_read_batch *b)
{
	if (!b) return;
	if (ctx) (void)hipSetDevice(ctx->device);
	if (ctx) {
		{
			std::lock_guard<std::mutex> lk(ctx->enc_mu);
			if (ctx->enc_pool.size() < 6) ctx->enc_pool.push_back(std::move(b->enc));
		}
		if (b->d_reads) (void)hipFreeAsync(b->d_reads, ctx->stream);
		if (b->d_roff) (void)hipFreeAsync(b->d_roff, ctx->stream);
	} else {
		if (b->d_reads) (void)hipFree(b->d_reads);
		if (b->d_roff) (void)hipFree(b->d_roff);
	}
	delete b;
}

// Records leave the library in slabs of many reads each: a short-read batch has a quarter of a million reads, and an allocation
// per read made the caller's gdiet_hip_free_regs the slowest stage of the pipeline.  Every host worker fills slabs of its own (a
// read's records are written, and its temporaries released, by the thread that computed them), so no lock is involved.  Every
// read's record array is preceded by a 16-byte GdRegHead; `head` marks the ones that start an allocation.
struct GdRegHead { uint32_t magic, head; uint64_t pad; };
static const uint32_t GD_REG_MAGIC = 0x67645247u;
static const size_t GD_REG_SLAB = 1 << 20;

struct GdRegCursor { uint64_t call = 0; char *p = nullptr; size_t left = 0; };
static GdRegCursor &gd_reg_cursor() // (this thread's: fetched once per chunk of reads -- a thread_local of a shared library costs a call per access)
{
	static thread_local GdRegCursor C;
	return C;
}
static void *gd_reg_slab_take(GdRegCursor &C, uint64_t call_id, size_t bytes, bool &head)
{
	head = false;
	if (C.call != call_id || C.left < bytes) { // what is left of the previous slab stays with its records
		const size_t sz = std::max(bytes, GD_REG_SLAB);
		char *m = (char *)malloc(sz);
		if (!m) return nullptr;
		C.call = call_id, C.p = m, C.left = sz, head = true;
	}
	void *at = C.p;
	C.p += bytes, C.left -= bytes;
	return at;
}

static size_t gd_regs_bytes(const std::vector<GdReg> &v)
{
	if (v.empty()) return 0;
	size_t words = 0;
	for (const GdReg &g : v) words += g.cigar.size() + 1;
	return sizeof(GdRegHead) + v.size() * sizeof(gdiet_reg_t) + ((words * 4 + 7) & ~(size_t)7);
}

static void gd_regs_fill(const std::vector<GdReg> &v, void *at, bool head, int32_t *n_regs, gdiet_reg_t **regs)
{
	*n_regs = (int32_t)v.size();
	*regs = nullptr;
	if (v.empty()) return;
	GdRegHead *h = (GdRegHead *)at;
	h->magic = GD_REG_MAGIC, h->head = head ? 1 : 0, h->pad = 0;
	gdiet_reg_t *r = (gdiet_reg_t *)(h + 1);
	uint32_t *cg = (uint32_t *)(r + v.size());
	for (size_t i = 0; i < v.size(); ++i) {
		const GdReg &g = v[i];
		memset(&r[i], 0, sizeof(r[i]));
		r[i].id = g.id, r[i].cnt = g.cnt, r[i].rid = g.rid, r[i].score = g.score, r[i].qs = g.qs, r[i].qe = g.qe, r[i].rs = g.rs, r[i].re = g.re;
		r[i].parent = g.parent, r[i].subsc = g.subsc, r[i].mlen = g.mlen, r[i].blen = g.blen, r[i].mapq = g.mapq, r[i].rev = g.rev, r[i].sam_pri = g.sam_pri;
		r[i].dp_score = g.dp_score, r[i].dp_max = g.dp_max, r[i].n_ambi = g.n_ambi, r[i].n_cigar = (uint32_t)g.cigar.size();
		r[i].cigar = cg;
		if (!g.cigar.empty()) memcpy(cg, g.cigar.data(), g.cigar.size() * 4);
		cg[g.cigar.size()] = 0;
		cg += g.cigar.size() + 1;
	}
	*regs = r;
}

// the inverse: a record of the C interface as the formatters' GdReg
static void gd_reg_from_c(const gdiet_reg_t &r, GdReg &g)
{
	g.id = r.id, g.cnt = r.cnt, g.rid = r.rid, g.score = r.score, g.qs = r.qs, g.qe = r.qe, g.rs = r.rs, g.re = r.re, g.parent = r.parent, g.subsc = r.subsc;
	g.mlen = r.mlen, g.blen = r.blen, g.mapq = r.mapq, g.rev = r.rev, g.sam_pri = r.sam_pri, g.dp_score = r.dp_score, g.dp_max = r.dp_max, g.n_ambi = r.n_ambi;
	g.has_p = true, g.cigar.assign(r.cigar, r.cigar + r.n_cigar);
}

extern "C" void gdiet_hip_free_regs(int n, int32_t *n_regs, gdiet_reg_t **regs)
{
	if (!n_regs || !regs) return;
	std::vector<void *> blocks; // freed after the scan: the other reads' heads live inside them
	for (int i = 0; i < n; ++i) {
		if (regs[i]) {
			GdRegHead *h = (GdRegHead *)regs[i] - 1;
			if (h->magic == GD_REG_MAGIC && h->head) blocks.push_back(h);
		}
		regs[i] = nullptr, n_regs[i] = 0;
	}
	for (void *b : blocks) free(b);
}

static void gd_opt_from_c(const gdiet_mapopt_t *o, const gdiet_index *ix, GdMapOpt &O)
{
	O.flag = o->flag, O.k = ix->h.k, O.w = ix->h.w, O.a = o->a, O.b = o->b, O.q = o->q, O.e = o->e, O.q2 = o->q2, O.e2 = o->e2;
	O.bw = o->bw, O.min_dp_max = o->min_dp_max, O.best_n = o->best_n, O.q_occ_frac = o->q_occ_frac, O.mid_occ = o->mid_occ;
	O.max_max_occ = o->max_max_occ, O.occ_dist = o->occ_dist, O.max_frag_len = o->max_frag_len, O.vt_dis = o->vt_dis, O.vt_nb_loc = o->vt_nb_loc;
	O.vt_cov = o->vt_cov, O.vt_f = o->vt_f, O.vt_df1 = o->vt_df1, O.vt_df2 = o->vt_df2, O.max_max_gap = o->max_max_gap, O.max_min_gap = o->max_min_gap;
	O.max_seeds = o->max_seeds, O.pat = ix->h.pat;
	O.min_cnt = o->min_cnt, O.rec_threshold_frac = o->rec_threshold_frac, O.bw_frac = o->bw_frac, O.bw_min = o->bw_min, O.bw_max = o->bw_max;
	O.af_max_loc = o->AF_max_loc;
}

static void gd_drop_async_lanes(gdiet_ctx *ctx)
{
	for (int i = 0; i < GD_MAX_INFLIGHT; ++i)
		if (ctx->async_lane[i] && !ctx->async_busy[i]) gdiet_hip_destroy(ctx->async_lane[i]), ctx->async_lane[i] = nullptr;
}

static int gd_check_opt(gdiet_ctx *ctx, const GdMapOpt &O)
{
	if (O.flag & GD_F_SR) {
		if (O.af_max_loc < 1 || O.af_max_loc > GDM_MAX_VT) { ctx->err = "AF_max_loc must be in [1," + std::to_string(GDM_MAX_VT) + "]"; return GDIET_E_PARAM; }
	} else if (O.vt_nb_loc + 2 > GDM_MAX_VT) { ctx->err = "vt_nb_loc too large"; return GDIET_E_PARAM; }
	if (O.mid_occ <= 0) { ctx->err = "mid_occ must be set (mm_mapopt_update)"; return GDIET_E_PARAM; }
	return GDIET_OK;
}

// The scoring of a mapping call: what the reference's mm_check_opt refuses (LR/options.c:208-223) is refused here too, and so is a value the
// DP's int8_t parameters cannot hold (gd_stage_dp narrows them).  The DP-level entry points keep their own checks (gd_consts): they
// take the larger gap model first as well.
static int gd_check_scoring(gdiet_ctx *ctx, const GdMapOpt &O)
{
	for (int v : {O.a, O.b, O.q, O.e, O.q2, O.e2})
		if (v < -128 || v > 127) { ctx->err = "scoring: a, b, q, e, q2 and e2 must each fit an int8_t"; return GDIET_E_PARAM; }
	if (O.q <= 0 || O.e <= 0) { ctx->err = "scoring: q and e (-O, -E) must be positive"; return GDIET_E_PARAM; }
	if ((O.q != O.q2 || O.e != O.e2) && !(O.e > O.e2 && O.q + O.e < O.q2 + O.e2)) {
		ctx->err = "scoring: dual gap penalties violating e > e2 and q + e < q2 + e2";
		return GDIET_E_PARAM;
	}
	if ((O.q + O.e) + (O.q2 + O.e2) > 127) { ctx->err = "scoring: (q+e)+(q2+e2) > 127"; return GDIET_E_PARAM; }
	return GDIET_OK;
}

// a contiguous slice of a resident read batch
struct GdBatchView {
	int n;
	const int64_t *roff;   // n+1 absolute offsets into enc / d_reads
	const uint8_t *enc;    // host copy (whole batch)
	const uint8_t *d_reads;
	const int64_t *d_roff; // device copy of roff (already offset to the slice)
};

// B4 (gdiet_hip_seed_batch): what the seeding stage leaves, copied out right behind the seed kernel instead of going on
struct GdSeedExport {
	std::vector<MapSeedOut> out;   // per read: shift, tmp_extracted_len, n_mv, n_seeds, n_a
	std::vector<GdSeed> seeds;     // the kept seeds of all reads, back to back
};

// GDIET_FAULT_BOX=<read index> (fault injection for the tests): the boxes of that read of every batch count as degenerate; -1: none
static int gd_fault_box()
{
	static const char *fault_env = getenv("GDIET_FAULT_BOX");
	return fault_env ? atoi(fault_env) : -1;
}

// The state of one gd_map_range call: what its stages hand to each other.  Lives on that function's stack.
struct GdMapCall {
	gdiet_ctx *ctx; // the lane: the parent context or one of its children
	const gdiet_index *ix;
	const GdMapOpt &O;
	const GdBatchView &B;
	int32_t *n_regs;
	gdiet_reg_t **regs;
	GdStageTrace mark; // wall time of the host-side sub-steps of this call
	double t0 = 0;     // start of the step that ctx->stage_s[] is charged for next (gd_lap)
	MapDevOpt D;
	bool is_sr = false, sr_dev = false; // ShortReads variant; its box stage on the device
	std::vector<MapReadScratch> sc;     // scratch layout
	GdSeedClasses cls;                  // capacity classes of the seed kernel
	MapSeedOut *so = nullptr;           // host copy of the seed records (ctx->h_seedout)
	std::vector<int64_t> hoff;          // hit offsets, n + 1
	GdBoxTables T;
	// pointers into m_aux: d_coff | d_ex | d_score | d_ncig in one buffer, the last three 256-byte aligned as their host copies
	size_t nbp = 64;
	int64_t *d_coff = nullptr;
	int32_t *d_ex = nullptr, *d_score = nullptr, *d_ncig = nullptr;
	// results of the DP and pack stages on the host
	int32_t *h_score = nullptr, *h_ncig = nullptr;
	const GdPostOut *h_post = nullptr;
	uint32_t *h_cig = nullptr;
	std::vector<int64_t> poff{0};
};

static void gd_lap(GdMapCall &c, int stage) { c.ctx->stage_s[stage] += gd_now() - c.t0, c.t0 = gd_now(); }

static int gd_scratch_grow(GdMapCall &c, bool full)
{
	gdiet_ctx *ctx = c.ctx;
	const int n = c.B.n;
	const uint64_t tot = gd_scratch_layout(n, c.B.roff, c.O.w, c.O.pat, c.O.max_seeds, full, c.sc.data());
	int rc;
	if ((rc = gd_grow(ctx, ctx->m_sc, sizeof(MapReadScratch) * n))) return rc;
	if ((rc = gd_grow(ctx, ctx->m_mv, sizeof(GdMini) * tot))) return rc;
	if ((rc = gd_grow(ctx, ctx->m_u64, sizeof(uint64_t) * 2 * tot))) return rc;
	if ((rc = gd_grow(ctx, ctx->m_seed, sizeof(GdSeed) * tot))) return rc;
	GD_HIP(hipMemcpyAsync(ctx->m_sc.p, c.sc.data(), sizeof(MapReadScratch) * n, hipMemcpyHostToDevice, ctx->stream));
	return GDIET_OK;
}

// scratch layout, MapDevOpt from GdMapOpt, capacity classes of the seed kernel
static int gd_stage_setup(GdMapCall &c)
{
	gdiet_ctx *ctx = c.ctx;
	const GdMapOpt &O = c.O;
	const int n = c.B.n;
	int rc;
	c.sc.resize(n);
	if ((rc = gd_scratch_grow(c, false))) return rc;
	if ((rc = gd_grow(ctx, ctx->m_seedout, sizeof(MapSeedOut) * n))) return rc;
	if ((rc = gd_grow(ctx, ctx->m_voteout, sizeof(MapVoteOut) * n))) return rc;
	if ((rc = gd_grow(ctx, ctx->m_hitoff, sizeof(int64_t) * (n + 1)))) return rc;
	MapDevOpt &D = c.D;
	D.k = O.k, D.w = O.w, D.max_seeds = O.max_seeds, D.q_occ_frac = O.q_occ_frac, D.mid_occ = O.mid_occ, D.max_max_occ = O.max_max_occ, D.occ_dist = O.occ_dist;
	D.max_nb_seeds = (O.flag & GD_F_FRAG_MODE) ? (O.max_frag_len == 0 ? 800u : (uint32_t)O.max_frag_len) : UINT32_MAX;
	D.flag = O.flag, D.pat = O.pat;
	D.vote.vt_dis = O.vt_dis, D.vote.vt_nb_loc = O.vt_nb_loc, D.vote.bw = O.bw, D.vote.vt_cov = O.vt_cov, D.vote.vt_f = O.vt_f;
	D.vote.vt_df1 = O.vt_df1, D.vote.vt_df2 = O.vt_df2, D.vote.k = O.k;
	c.is_sr = (O.flag & GD_F_SR) != 0;
	D.is_sr = c.is_sr;
	// The seeding / voting wavefronts of a batch run beside the DP wavefronts of the batch before it (five per SIMD, VALU-bound, older): at
	// the default priority they get the issue slots those leave, hold their scarce slots for a long time, and the batch is ready only when
	// that DP kernel ends -- with two batches in flight the next DP kernel then starts ~5 ms late (834 Mbases/s).  At s_setprio(2) they are
	// through in ~60 ms, the DP kernels follow each other back to back with TWO batches in flight (875-881 Mbases/s) and a batch spends two
	// step times in the pipeline instead of three (p50 174 instead of 261 ms).
	D.prio = 2;
	gd_seed_classes(O.pat, O.w, n, c.B.roff, c.cls); // (map_plan.h)
	D.sort_cap = c.cls.sort_cap;
	D.sr.min_cnt = O.min_cnt, D.sr.rec_threshold_frac = O.rec_threshold_frac, D.sr.bw_frac = O.bw_frac, D.sr.bw_min = O.bw_min, D.sr.bw_max = O.bw_max;
	D.sr.af_max_loc = O.af_max_loc, D.sr.max_nb_seeds = D.max_nb_seeds, D.sr.frag_mode = (O.flag & GD_F_FRAG_MODE) != 0;
	// ShortReads: the box stage on the device (map_sr_box_kernel / map_sr_fill_kernel).  GDIET_SR_BOXES=host keeps the host stages.
	c.sr_dev = c.is_sr && ctx->sr_boxes_on_device && (int64_t)n * std::min<int64_t>(O.af_max_loc, GDM_MAX_VT) < ((int64_t)1 << 28);
	return GDIET_OK;
}

// S1-S5: the seed kernel in one of its three launch forms; a scratch overflow makes the batch retry once with the hard bound
static int gd_stage_seed(GdMapCall &c)
{
	gdiet_ctx *ctx = c.ctx;
	const gdiet_index *ix = c.ix;
	const GdMapOpt &O = c.O;
	const GdBatchView &B = c.B;
	MapDevOpt &D = c.D;
	const int n = B.n;
	hipStream_t s = ctx->stream;
	int rc;
	if ((rc = gd_host_grow(ctx, ctx->h_seedout, sizeof(MapSeedOut) * (size_t)n))) return rc;
	MapSeedOut *so = c.so = (MapSeedOut *)ctx->h_seedout.p;
	const size_t seed_lds = gd_seed_wave_lds_bytes(D.sort_cap);
	D.seed_lds = (uint32_t)seed_lds;
	if (seed_lds > 64 * 1024) GD_HIP(hipFuncSetAttribute((const void *)map_seed_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)seed_lds));
	for (int attempt = 0; attempt < 2; ++attempt) {
		// one read per thread (the plain sequential form) for short reads -- a 150 bp read has ~75 sparsified bases, far too few to
		// split over 64 lanes (measured 18x faster at 150 bp) -- and on request (GDIET_SEED_KERNEL=thread) for A/B checks
		if (ctx->seed_thread_kernel == 1 || (ctx->seed_thread_kernel == 0 && (B.roff[n] - B.roff[0]) / n < 1024))
			hipLaunchKernelGGL(map_seed_kernel, dim3((n + 63) / 64), dim3(64), (size_t)O.w * 64 * sizeof(GdMini), s, n, B.d_reads, B.d_roff, ix->dview, D, (const MapReadScratch *)ctx->m_sc.p,
			                   (GdMini *)ctx->m_mv.p, (uint64_t *)ctx->m_u64.p, (GdSeed *)ctx->m_seed.p, (MapSeedOut *)ctx->m_seedout.p);
		else if (!c.cls.classes.empty()) { // one read per wavefront, one launch per LDS capacity class
			if ((rc = gd_grow(ctx, ctx->m_seedids, sizeof(int32_t) * (size_t)n))) return rc;
			GD_HIP(hipMemcpyAsync(ctx->m_seedids.p, c.cls.ids.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
			int at = 0;
			for (const auto &cls : c.cls.classes) {
				MapDevOpt Dc = D;
				Dc.sort_cap = cls.first;
				const size_t lds_c = gd_seed_wave_lds_bytes(cls.first);
				Dc.seed_lds = (uint32_t)lds_c;
				hipLaunchKernelGGL(map_seed_wave_kernel, dim3(cls.second), dim3(64), lds_c, s, cls.second, B.d_reads, B.d_roff, ix->dview, Dc, (const MapReadScratch *)ctx->m_sc.p,
				                   (GdMini *)ctx->m_mv.p, (uint64_t *)ctx->m_u64.p, (GdSeed *)ctx->m_seed.p, (MapSeedOut *)ctx->m_seedout.p, (const int32_t *)ctx->m_seedids.p + at);
				at += cls.second;
			}
		} else // one read per wavefront: the tile sketch (64 positions per step) + parallel index probes
			hipLaunchKernelGGL(map_seed_wave_kernel, dim3(n), dim3(64), seed_lds, s, n, B.d_reads, B.d_roff, ix->dview, D, (const MapReadScratch *)ctx->m_sc.p,
			                   (GdMini *)ctx->m_mv.p, (uint64_t *)ctx->m_u64.p, (GdSeed *)ctx->m_seed.p, (MapSeedOut *)ctx->m_seedout.p, (const int32_t *)nullptr);
		GD_HIP(hipGetLastError()); // a refused launch (LDS size, grid) must not pass for stale seed records
		GD_HIP(hipMemcpyAsync(so, ctx->m_seedout.p, sizeof(MapSeedOut) * n, hipMemcpyDeviceToHost, s));
		GD_HIP(gd_stream_wait(ctx, s));
		bool overflow = false;
		for (int i = 0; i < n; ++i) overflow |= so[i].n_seeds < 0;
		if (!overflow) break;
		if (attempt == 1) { ctx->err = "minimizer scratch overflow even with the hard bound"; return GDIET_E_NOMEM; }
		++gd_scratch_retries;
		if ((rc = gd_scratch_grow(c, true))) return rc;
	}
	return GDIET_OK;
}

// B4: the seeds themselves are the result
static int gd_seed_export(GdMapCall &c, GdSeedExport &sx)
{
	gdiet_ctx *ctx = c.ctx;
	const int n = c.B.n;
	const MapSeedOut *so = c.so;
	hipStream_t s = ctx->stream;
	sx.out.assign(so, so + n);
	int64_t tot_seeds = 0;
	for (int i = 0; i < n; ++i) tot_seeds += so[i].n_seeds > 0 ? so[i].n_seeds : 0;
	sx.seeds.resize((size_t)tot_seeds);
	int64_t at = 0;
	for (int i = 0; i < n; ++i)
		if (so[i].n_seeds > 0) {
			GD_HIP(hipMemcpyAsync(sx.seeds.data() + at, (const GdSeed *)ctx->m_seed.p + c.sc[i].seed_off, sizeof(GdSeed) * (size_t)so[i].n_seeds, hipMemcpyDeviceToHost, s));
			at += so[i].n_seeds;
		}
	GD_HIP(gd_stream_wait(ctx, s));
	return GDIET_OK;
}

// S6, S7, V1, V3, G1a: hit offsets, then the vote kernel in one of its two launch forms
static int gd_stage_vote(GdMapCall &c)
{
	gdiet_ctx *ctx = c.ctx;
	const gdiet_index *ix = c.ix;
	const GdBatchView &B = c.B;
	const int n = B.n;
	hipStream_t s = ctx->stream;
	std::vector<int64_t> &hoff = c.hoff;
	int rc;
	hoff.assign(n + 1, 0);
	for (int i = 0; i < n; ++i) {
		hoff[i + 1] = hoff[i] + (c.so[i].n_seeds > 0 ? c.so[i].n_a : 0);
	}
	if ((rc = gd_grow(ctx, ctx->m_hits, sizeof(GdLoc) * 3 * (size_t)(hoff[n] + 1)))) return rc;
	GD_HIP(hipMemcpyAsync(ctx->m_hitoff.p, hoff.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, s));
	// long reads: one read per wavefront (parallel expansion + LDS sort); short reads (a handful of hits each): one read per thread
	const int spread = (B.roff[n] - B.roff[0]) / n >= 1024;
	if (spread == 1 && ctx->vote_wave) {
		// LDS sort buffer of the batch: the largest hit count of a read bounds either strand (see the kernel)
		int64_t max_hits = 0;
		for (int i = 0; i < n; ++i) max_hits = std::max(max_hits, hoff[i + 1] - hoff[i]);
		unsigned vote_cap = 256;
		while (vote_cap < MAP_VOTE_CAP && (int64_t)vote_cap < max_hits) vote_cap <<= 1;
		// the kernel also holds static LDS (its candidate list): with the full sort buffer the total passes 64 KB, which a launch is
		// only granted after the attribute has been raised
		if (sizeof(GdLoc) * (size_t)vote_cap + sizeof(GdVt) * GDM_MAX_VT + 64 > 64 * 1024)
			GD_HIP(hipFuncSetAttribute((const void *)map_vote_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(GdLoc) * (size_t)vote_cap)));
		hipLaunchKernelGGL(map_vote_wave_kernel, dim3(n), dim3(64), sizeof(GdLoc) * (size_t)vote_cap, s, n, B.d_roff, ix->dview, c.D, (const MapReadScratch *)ctx->m_sc.p,
		                   (const GdSeed *)ctx->m_seed.p, (const MapSeedOut *)ctx->m_seedout.p, (const int64_t *)ctx->m_hitoff.p, (GdLoc *)ctx->m_hits.p,
		                   (MapVoteOut *)ctx->m_voteout.p, vote_cap);
	} else
		hipLaunchKernelGGL(map_vote_kernel, dim3(spread ? n : (n + 63) / 64), dim3(64), 0, s, n, B.d_roff, ix->dview, c.D, (const MapReadScratch *)ctx->m_sc.p,
		                   (const GdSeed *)ctx->m_seed.p, (const MapSeedOut *)ctx->m_seedout.p, (const int64_t *)ctx->m_hitoff.p, (GdLoc *)ctx->m_hits.p,
		                   (MapVoteOut *)ctx->m_voteout.p, spread);
	GD_HIP(hipGetLastError());
	return GDIET_OK;
}

static int gd_aux_layout(GdMapCall &c) // d_coff | d_ex | d_score | d_ncig in one buffer, the last three 256-byte aligned as their host copies
{
	gdiet_ctx *ctx = c.ctx;
	const int nb = c.T.nb;
	c.nbp = ((size_t)std::max(nb, 1) + 63) & ~(size_t)63;
	int rc;
	if ((rc = gd_grow(ctx, ctx->m_aux, sizeof(int64_t) * (nb + 1) + sizeof(int32_t) * 3 * c.nbp + 1024))) return rc;
	c.d_coff = (int64_t *)ctx->m_aux.p;
	c.d_ex = (int32_t *)(((uintptr_t)(c.d_coff + nb + 1) + 255) & ~(uintptr_t)255), c.d_score = c.d_ex + c.nbp, c.d_ncig = c.d_score + c.nbp;
	return GDIET_OK;
}

// the reads a box stage gave up on (a degenerate DP box): counted, and the last one named in the context's warning
static void gd_note_failed(gdiet_ctx *ctx, int64_t n_failed, int last_bad)
{
	ctx->failed_last = n_failed, ctx->failed_total += n_failed;
	if (n_failed) ctx->warn = gd_failed_reads_warning(n_failed, last_bad);
}

// the contig table of the index on the device (once), for the device-side box stage
static int gd_index_seq_table(gdiet_ctx *ctx, const gdiet_index *ix)
{
	const GdRefView R = ix->h.ref();
	gdiet_index *ixm = const_cast<gdiet_index *>(ix);
	std::lock_guard<std::mutex> lk(ixm->seq_mu);
	if (ixm->d_seq_len) return GDIET_OK;
	std::vector<uint32_t> sl(R.n_seq);
	std::vector<uint64_t> so(R.n_seq);
	for (uint32_t q = 0; q < R.n_seq; ++q) sl[q] = R.seq[q].len, so[q] = R.seq[q].offset;
	uint32_t *dl = nullptr;
	uint64_t *d_o = nullptr;
	GD_HIP(hipMalloc(&dl, sizeof(uint32_t) * std::max<size_t>(R.n_seq, 1)));
	GD_HIP(hipMalloc(&d_o, sizeof(uint64_t) * std::max<size_t>(R.n_seq, 1)));
	GD_HIP(hipMemcpy(dl, sl.data(), sizeof(uint32_t) * R.n_seq, hipMemcpyHostToDevice));
	GD_HIP(hipMemcpy(d_o, so.data(), sizeof(uint64_t) * R.n_seq, hipMemcpyHostToDevice));
	ixm->d_seq_off = d_o, ixm->d_seq_len = dl;
	return GDIET_OK;
}

// G2 on the device (ShortReads; map_sr_box_kernel / map_sr_fill_kernel): the candidates never visit the host; what comes back are the
// dense per-box tables the DP planner and the record stage read.  Leaves the windows gathered.
static int gd_stage_boxes_device(GdMapCall &c)
{
	gdiet_ctx *ctx = c.ctx;
	const gdiet_index *ix = c.ix;
	const GdMapOpt &O = c.O;
	GdBoxTables &T = c.T;
	const int n = c.B.n;
	const int64_t *d_roff = c.B.d_roff;
	hipStream_t s = ctx->stream;
	const uint32_t n_seq = ix->h.ref().n_seq;
	const int slots = (int)std::min<int64_t>(O.af_max_loc, GDM_MAX_VT);
	int rc;
	T.reset(n);
	if ((rc = gd_index_seq_table(ctx, ix))) return rc;
	// per-read tables: sumlen[n + 1] | len_first[n + 1] (int64), cnt[n + 1] | box_first[n + 1] (int32), totals.  (The last entry of cnt and
	// of sumlen is never written: the scans below read it, but no output of an exclusive scan depends on its last input.)
	const size_t tab_bytes = sizeof(int64_t) * (2 * (size_t)n + 2) + sizeof(int32_t) * (2 * (size_t)n + 2) + sizeof(MapSrTotals) + 64;
	if ((rc = gd_grow(ctx, ctx->m_srtab, tab_bytes))) return rc;
	if ((rc = gd_grow(ctx, ctx->m_srbox, sizeof(GdCandBox) * (size_t)n * slots))) return rc;
	int64_t *d_sumlen = (int64_t *)ctx->m_srtab.p, *d_lenfirst = d_sumlen + n + 1;
	int32_t *d_cnt = (int32_t *)(d_lenfirst + n + 1), *d_boxfirst = d_cnt + n + 1;
	MapSrTotals *d_tot = (MapSrTotals *)(d_boxfirst + n + 1);
	const MapSrTotals zero = {0, -1};
	GD_HIP(hipMemcpyAsync(d_tot, &zero, sizeof zero, hipMemcpyHostToDevice, s));
	hipLaunchKernelGGL(map_sr_box_kernel, dim3((n + 63) / 64), dim3(64), 0, s, n, d_roff, (const MapVoteOut *)ctx->m_voteout.p, (const uint32_t *)ix->d_seq_len, n_seq,
	                   O.k, O.a, slots, gd_fault_box(), (GdCandBox *)ctx->m_srbox.p, d_cnt, d_sumlen, d_tot);
	// exclusive scans over n + 1 entries, input and output apart: the scans' last outputs are the totals
	size_t b1 = 0, b2 = 0;
	GD_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b1, d_cnt, d_boxfirst, n + 1, s));
	GD_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b2, d_sumlen, d_lenfirst, n + 1, s));
	if ((rc = gd_grow(ctx, ctx->m_srscan, std::max(b1, b2) + 64))) return rc;
	size_t bb = ctx->m_srscan.cap;
	GD_HIP(hipcub::DeviceScan::ExclusiveSum(ctx->m_srscan.p, bb, d_cnt, d_boxfirst, n + 1, s));
	bb = ctx->m_srscan.cap;
	GD_HIP(hipcub::DeviceScan::ExclusiveSum(ctx->m_srscan.p, bb, d_sumlen, d_lenfirst, n + 1, s));
	// the two totals and the failure count: 24 bytes, the only thing the host waits for before it can size the batch's buffers
	struct { int32_t nb; int32_t pad; int64_t bases; MapSrTotals t; } h_tot;
	GD_HIP(hipMemcpyAsync(&h_tot.nb, d_boxfirst + n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
	GD_HIP(hipMemcpyAsync(&h_tot.bases, d_lenfirst + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
	GD_HIP(hipMemcpyAsync(&h_tot.t, d_tot, sizeof(MapSrTotals), hipMemcpyDeviceToHost, s));
	GD_HIP(gd_stream_wait(ctx, s));
	gd_lap(c, 1);
	c.mark("vote");
	const int nb = T.nb = h_tot.nb;
	gd_note_failed(ctx, h_tot.t.n_failed, h_tot.t.last_failed);
	if ((rc = gd_aux_layout(c))) return rc;
	if (nb > 0) {
		if ((rc = gd_grow(ctx, ctx->m_boxes, sizeof(MapBox) * (size_t)nb))) return rc;
		if ((rc = gd_grow(ctx, ctx->m_srcand, sizeof(GdCandBox) * (size_t)nb + sizeof(int64_t) * ((size_t)nb + 1) + sizeof(int32_t) * (size_t)nb + 256))) return rc;
		GdCandBox *d_cand = (GdCandBox *)ctx->m_srcand.p;
		int64_t *d_qoff = (int64_t *)(((uintptr_t)(d_cand + nb) + 63) & ~(uintptr_t)63);
		int32_t *d_bw = (int32_t *)(d_qoff + nb + 1);
		MapSrFillOut FO = {(MapBox *)ctx->m_boxes.p, d_cand, d_qoff, c.d_coff, d_bw, c.d_ex};
		hipLaunchKernelGGL(map_sr_fill_kernel, dim3((n + 1 + 63) / 64), dim3(64), 0, s, n, d_roff, (const int32_t *)d_cnt, (const int32_t *)d_boxfirst, (const int64_t *)d_lenfirst,
		                   (const GdCandBox *)ctx->m_srbox.p, slots, (const uint32_t *)ix->d_seq_len, (const uint64_t *)ix->d_seq_off, n_seq, c.D.sr, FO);
		// host copies of what the planner and the record stage read
		if ((rc = gd_host_grow(ctx, ctx->h_cand, sizeof(GdCandBox) * (size_t)nb))) return rc;
		T.cflat = (GdCandBox *)ctx->h_cand.p;
		T.qoff.resize(nb + 1), T.coff.resize(nb + 1), T.bw.resize(nb), T.ex.resize(nb);
		GD_HIP(hipMemcpyAsync(T.cflat, d_cand, sizeof(GdCandBox) * (size_t)nb, hipMemcpyDeviceToHost, s));
		GD_HIP(hipMemcpyAsync(T.qoff.data(), d_qoff, sizeof(int64_t) * ((size_t)nb + 1), hipMemcpyDeviceToHost, s));
		GD_HIP(hipMemcpyAsync(T.coff.data(), c.d_coff, sizeof(int64_t) * ((size_t)nb + 1), hipMemcpyDeviceToHost, s));
		GD_HIP(hipMemcpyAsync(T.bw.data(), d_bw, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, s));
		GD_HIP(hipMemcpyAsync(T.ex.data(), c.d_ex, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, s));
	} else T.qoff.assign(1, 0), T.coff.assign(1, 0);
	GD_HIP(hipMemcpyAsync(T.ccount.data(), d_cnt, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
	// the windows can be gathered while the tables travel (same stream: the gather kernel is queued behind the fill kernel)
	if (nb > 0) {
		if ((rc = gd_grow(ctx, ctx->m_q, (size_t)h_tot.bases + 64))) return rc;
		if ((rc = gd_grow(ctx, ctx->m_t, (size_t)h_tot.bases + 64))) return rc;
		if ((rc = gd_grow(ctx, ctx->m_cig, sizeof(uint32_t) * (2 * (size_t)h_tot.bases + 1)))) return rc;
		hipLaunchKernelGGL(map_gather_kernel, dim3(nb), dim3(64), 0, s, nb, (const MapBox *)ctx->m_boxes.p, c.B.d_reads, (const uint32_t *)ix->d_S,
		                   (uint8_t *)ctx->m_q.p, (uint8_t *)ctx->m_t.p);
	}
	GD_HIP(gd_stream_wait(ctx, s));
	for (int i = 0; i < n; ++i) T.box_first[i + 1] = T.box_first[i] + T.ccount[i];
	T.cfirst = T.box_first;
	if (T.box_first[n] != nb) { ctx->err = "box tables of the device and the host disagree"; return GDIET_E_HIP; }
	T.toff = T.qoff;
	return GDIET_OK;
}

// G1b / G2 on host threads (map_plan.h): the vote records come to the host, linking + DP boxes, the box tables
static int gd_stage_boxes_host(GdMapCall &c)
{
	gdiet_ctx *ctx = c.ctx;
	const GdBatchView &B = c.B;
	GdBoxTables &T = c.T;
	const int n = B.n;
	hipStream_t s = ctx->stream;
	const GdRefView R = c.ix->h.ref();
	auto run = [&](int m, auto f) { gd_parallel_for(ctx, ctx->lane_threads, m, f); };
	int rc;
	T.reset(n);
	const size_t vo_head = gd_vote_head_bytes(c.O); // the host copy is packed to the head of every record
	if (ctx->h_vo.size() < vo_head * (size_t)n) ctx->h_vo.resize(vo_head * (size_t)n + (vo_head * (size_t)n >> 2));
	const uint8_t *vo_raw = ctx->h_vo.data();
	GD_HIP(hipMemcpy2DAsync(ctx->h_vo.data(), vo_head, ctx->m_voteout.p, sizeof(MapVoteOut), vo_head, (size_t)n, hipMemcpyDeviceToHost, s));
	GD_HIP(gd_stream_wait(ctx, s));
	gd_lap(c, 1);
	c.mark("vote");
	// candidates of all reads in one flat array (capacity: what the vote kernel reported; the box stage may drop some).  Per-read
	// vectors would be allocated by the workers and released by this thread -- a quarter of a million cross-thread frees per
	// short-read batch, each contending for another thread's malloc arena.
	if ((rc = gd_host_grow(ctx, ctx->h_cand, sizeof(GdCandBox) * (size_t)gd_box_slots(T, n, vo_raw, vo_head)))) return rc;
	T.cflat = (GdCandBox *)ctx->h_cand.p;
	c.mark("g:prefix");
	gd_box_candidates(T, n, B.roff, vo_raw, vo_head, c.O, R, run);
	int last_bad;
	const int64_t n_failed = gd_box_fail_degenerate(T, n, B.roff, gd_fault_box(), &last_bad);
	gd_note_failed(ctx, n_failed, last_bad);
	c.mark("g:boxes");
	if ((rc = gd_host_grow(ctx, ctx->h_boxes, sizeof(MapBox) * (size_t)std::max(T.nb, 1)))) return rc;
	gd_box_fill(T, n, B.roff, c.O, c.D.sr, R, (MapBox *)ctx->h_boxes.p, run, c.mark);
	return GDIET_OK;
}

// after the host box stage: the tables go to the device and the windows are gathered (the device box stage has left both done)
static int gd_upload_boxes(GdMapCall &c)
{
	gdiet_ctx *ctx = c.ctx;
	const GdBoxTables &T = c.T;
	const int nb = T.nb;
	hipStream_t s = ctx->stream;
	int rc;
	if ((rc = gd_grow(ctx, ctx->m_boxes, sizeof(MapBox) * nb))) return rc;
	if ((rc = gd_grow(ctx, ctx->m_q, (size_t)T.qoff[nb] + 64))) return rc;
	if ((rc = gd_grow(ctx, ctx->m_t, (size_t)T.toff[nb] + 64))) return rc;
	if ((rc = gd_aux_layout(c))) return rc;
	if ((rc = gd_grow(ctx, ctx->m_cig, sizeof(uint32_t) * ((size_t)T.coff[nb] + 1)))) return rc;
	GD_HIP(hipMemcpyAsync(ctx->m_boxes.p, ctx->h_boxes.p, sizeof(MapBox) * nb, hipMemcpyHostToDevice, s));
	GD_HIP(hipMemcpyAsync(c.d_coff, T.coff.data(), sizeof(int64_t) * (nb + 1), hipMemcpyHostToDevice, s));
	GD_HIP(hipMemcpyAsync(c.d_ex, T.ex.data(), sizeof(int32_t) * nb, hipMemcpyHostToDevice, s));
	hipLaunchKernelGGL(map_gather_kernel, dim3(nb), dim3(64), 0, s, nb, (const MapBox *)ctx->m_boxes.p, c.B.d_reads, (const uint32_t *)c.ix->d_S,
	                   (uint8_t *)ctx->m_q.p, (uint8_t *)ctx->m_t.p);
	return GDIET_OK;
}

// host buffers of the DP results
static int gd_result_tables(GdMapCall &c)
{
	gdiet_ctx *ctx = c.ctx;
	const int nb = c.T.nb;
	int rc;
	// scores | CIGAR lengths come back in ONE copy with both ends 256-byte aligned.  (As two copies the second, starting at an address
	// that is not a multiple of 16, took the runtime's dword copy kernel with 1024-thread workgroups: 16 wavefronts that need four
	// free slots on every SIMD of one CU, which the DP kernel of the next batch -- five wavefronts per SIMD -- never leaves.  That
	// 37 KB copy then finished only in the tail of the other batch's DP kernel, 45-60 ms later (kernel trace, round 2): invisible in
	// the throughput with three batches in flight, but it is the batch's latency.  Pinned host buffers were tried as well and cost 8 %
	// of the step: the host stages write these tables.)
	c.nbp = ((size_t)std::max(nb, 1) + 63) & ~(size_t)63;
	if ((rc = gd_host_grow(ctx, ctx->h_res, sizeof(int32_t) * 2 * c.nbp))) return rc;
	c.h_score = (int32_t *)ctx->h_res.p, c.h_ncig = c.h_score + c.nbp;
	if ((rc = gd_host_grow(ctx, ctx->h_post, sizeof(GdPostOut) * (size_t)std::max(nb, 1)))) return rc;
	c.h_post = (const GdPostOut *)ctx->h_post.p;
	return GDIET_OK;
}

// P1's launch in one of its three forms: what gd_stage_dp enqueues behind the backtrack, and all that gdiet_hip_post_batch runs
static void gd_launch_post(bool wave, bool eqx, int nb, const MapBox *boxes, const uint8_t *q, const uint8_t *t, const int64_t *coff, uint32_t *cig, int32_t *ncig,
                           const int32_t *score, const MapPostOpt &PO, GdPostOut *post, int32_t *x_score, int32_t *x_ncig, hipStream_t s)
{
	if (wave) hipLaunchKernelGGL(map_post_wave_kernel, dim3(nb), dim3(64), 0, s, nb, boxes, q, t, coff, cig, ncig, score, PO, post, x_score, x_ncig);
	else if (eqx) hipLaunchKernelGGL(map_post_kernel<true>, dim3((nb + 63) / 64), dim3(64), 0, s, nb, boxes, q, t, coff, cig, ncig, score, PO, post, x_score, x_ncig);
	else hipLaunchKernelGGL(map_post_kernel<false>, dim3((nb + 63) / 64), dim3(64), 0, s, nb, boxes, q, t, coff, cig, ncig, score, PO, post, x_score, x_ncig);
}

// The kernel-level boundary of P1 (include/gdiet_hip.h): buffers of its own for this call, the launch above, the results back.  The
// windows must hold what every live CIGAR consumes: checked here, on the raw CIGAR (mm_fix_cigar moves bases between operations, never
// their sums), so that no input can make a kernel read outside them.
extern "C" int gdiet_hip_post_batch(gdiet_ctx *ctx, int n, const uint8_t *qseq, const int64_t *qoff, const uint8_t *tseq, const int64_t *toff, uint32_t *cigar,
                                    const int64_t *coff, int32_t *n_cigar, const int32_t *score, const int8_t *mat, int8_t q, int8_t e, int log_gap, int form,
                                    int exported, int32_t *post)
{
	if (!ctx || n < 0 || (n && (!qoff || !toff || !coff || !n_cigar || !score || !mat || !post)) || (form != 0 && form != 1)) return GDIET_E_PARAM;
	if (n == 0) return GDIET_OK;
	gd_err_clear();
	(void)hipSetDevice(ctx->device);
	if (qoff[0] < 0 || toff[0] < 0 || coff[0] < 0) { ctx->err = "gdiet_hip_post_batch: negative offset"; return GDIET_E_PARAM; }
	std::vector<MapBox> boxes((size_t)n);
	for (int b = 0; b < n; ++b) {
		if (qoff[b + 1] < qoff[b] || toff[b + 1] < toff[b] || coff[b + 1] < coff[b]) { ctx->err = "gdiet_hip_post_batch: offsets must not decrease"; return GDIET_E_PARAM; }
		memset(&boxes[(size_t)b], 0, sizeof(MapBox));
		boxes[(size_t)b].q_dst = qoff[b], boxes[(size_t)b].t_dst = toff[b];
		if (score[b] == GD_NEG_INF_SCORE_DEV || n_cigar[b] <= 0 || (int64_t)n_cigar[b] > coff[b + 1] - coff[b]) continue; // dead: never read
		int64_t ql = 0, tl = 0;
		for (int32_t k = 0; k < n_cigar[b]; ++k) {
			const uint32_t c = cigar[coff[b] + k], op = c & 0xf, len = c >> 4;
			if (op == 0) ql += len, tl += len;
			else if (op == 1) ql += len;
			else if (op == 2 || op == 3) tl += len;
		}
		if (ql > qoff[b + 1] - qoff[b] || tl > toff[b + 1] - toff[b]) {
			ctx->err = "gdiet_hip_post_batch: the CIGAR of alignment " + std::to_string(b) + " consumes more than its windows hold";
			return GDIET_E_PARAM;
		}
	}
	const size_t nq = (size_t)qoff[n], nt = (size_t)toff[n], nc = (size_t)coff[n], nbp = ((size_t)n + 63) & ~(size_t)63;
	if ((nq && !qseq) || (nt && !tseq) || (nc && !cigar)) return GDIET_E_PARAM;
	MapPostOpt PO;
	memcpy(PO.mat, mat, 25);
	PO.q = q, PO.e = e, PO.log_gap = log_gap != 0;
	DevBuf d_box, d_q, d_t, d_coff, d_cig, d_nc, d_sc, d_post, h_pin;
	int rc;
	if ((rc = gd_grow(ctx, d_box, sizeof(MapBox) * (size_t)n)) || (rc = gd_grow(ctx, d_q, std::max<size_t>(nq, 1))) || (rc = gd_grow(ctx, d_t, std::max<size_t>(nt, 1))) ||
	    (rc = gd_grow(ctx, d_coff, sizeof(int64_t) * ((size_t)n + 1))) || (rc = gd_grow(ctx, d_cig, sizeof(uint32_t) * std::max<size_t>(nc, 1))) ||
	    (rc = gd_grow(ctx, d_nc, sizeof(int32_t) * (size_t)n)) || (rc = gd_grow(ctx, d_sc, sizeof(int32_t) * (size_t)n)) ||
	    (rc = gd_grow(ctx, d_post, sizeof(GdPostOut) * (size_t)n)))
		return rc;
	hipStream_t s = ctx->stream;
	GD_HIP(hipMemcpyAsync(d_box.p, boxes.data(), sizeof(MapBox) * (size_t)n, hipMemcpyHostToDevice, s));
	if (nq) GD_HIP(hipMemcpyAsync(d_q.p, qseq, nq, hipMemcpyHostToDevice, s));
	if (nt) GD_HIP(hipMemcpyAsync(d_t.p, tseq, nt, hipMemcpyHostToDevice, s));
	GD_HIP(hipMemcpyAsync(d_coff.p, coff, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, s));
	if (nc) GD_HIP(hipMemcpyAsync(d_cig.p, cigar, sizeof(uint32_t) * nc, hipMemcpyHostToDevice, s));
	GD_HIP(hipMemcpyAsync(d_nc.p, n_cigar, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
	GD_HIP(hipMemcpyAsync(d_sc.p, score, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
	GdPostOut *o_post = (GdPostOut *)d_post.p;
	int32_t *o_score = nullptr, *o_ncig = nullptr;
	if (exported) { // laid out as gd_stage_dp lays its export buffer out: scores, CIGAR lengths, results
		const size_t need = sizeof(GdPostOut) * (size_t)n + sizeof(int32_t) * 2 * nbp;
		h_pin.kind = DevBuf::PINNED;
		GD_HIP(hipHostMalloc(&h_pin.p, need, hipHostMallocDefault));
		h_pin.cap = need;
		memset(h_pin.p, 0xff, need);
		o_score = (int32_t *)h_pin.p, o_ncig = o_score + nbp, o_post = (GdPostOut *)(o_ncig + nbp);
	}
	gd_launch_post(form == 1, false, n, (const MapBox *)d_box.p, (const uint8_t *)d_q.p, (const uint8_t *)d_t.p, (const int64_t *)d_coff.p, (uint32_t *)d_cig.p,
	               (int32_t *)d_nc.p, (const int32_t *)d_sc.p, PO, o_post, o_score, o_ncig, s);
	GD_HIP(hipGetLastError());
	if (nc) GD_HIP(hipMemcpyAsync(cigar, d_cig.p, sizeof(uint32_t) * nc, hipMemcpyDeviceToHost, s));
	if (!exported) {
		GD_HIP(hipMemcpyAsync(n_cigar, d_nc.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
		GD_HIP(hipMemcpyAsync(post, d_post.p, sizeof(GdPostOut) * (size_t)n, hipMemcpyDeviceToHost, s));
	}
	GD_HIP(hipStreamSynchronize(s));
	if (exported) {
		if (memcmp(o_score, score, sizeof(int32_t) * (size_t)n)) { ctx->err = "gdiet_hip_post_batch: the exported scores differ from the ones given"; return GDIET_E_HIP; }
		memcpy(n_cigar, o_ncig, sizeof(int32_t) * (size_t)n), memcpy(post, o_post, sizeof(GdPostOut) * (size_t)n);
	}
	return GDIET_OK;
}

// the DP batch over the gathered windows (gd_ksw_batch_dev), P1 on the device behind it, the results to the host
static int gd_stage_dp(GdMapCall &c)
{
	gdiet_ctx *ctx = c.ctx;
	const GdMapOpt &O = c.O;
	const GdBoxTables &T = c.T;
	const int nb = T.nb;
	const size_t nbp = c.nbp;
	hipStream_t s = ctx->stream;
	int rc;
	// an async lane whose batch does not fit a private arena (gd_ksw_batch_dev: own_arena) shares its parent's backtrace arena, and the
	// DP stages take turns; one whose batch fits -- a HiFi batch of 5 120 reads does, with the compact arena -- is not chained behind the others
	std::unique_lock<std::mutex> dp_lock;
	gdiet_ksw_score_t ks;
	ks.match = (int8_t)O.a, ks.mismatch = (int8_t)(O.b < 0 ? O.b : -O.b), ks.sc_ambi = 0, ks.q = (int8_t)O.q, ks.e = (int8_t)O.e, ks.q2 = (int8_t)O.q2, ks.e2 = (int8_t)O.e2;
	ks.reserved = 0, ks.flag = GDIET_EZ_APPROX_MAX;
	// In an async lane the DP stage (pre-filter, DP + backtrack kernels) runs on a stream of its own and is ENQUEUED behind the
	// DP stage of whichever lane used the shared arena last (arena_ev), so that consecutive DP kernels follow each other on the
	// GPU without a host round trip in between; dp_mu only orders the enqueueing.
	hipStream_t sd = s;
	if (ctx->parent) {
		sd = ctx->stream_dp;
		GD_HIP(hipEventRecord(ctx->gather_ev, s)); // windows gathered (and everything else queued on s)
		GD_HIP(hipStreamWaitEvent(sd, ctx->gather_ev, 0));
		dp_lock = std::unique_lock<std::mutex>(ctx->parent->dp_mu, std::defer_lock); // taken inside, after the planning
	}
	rc = gd_ksw_batch_dev(ctx, nb, (const uint8_t *)ctx->m_q.p, (const uint8_t *)ctx->m_t.p, c.d_ex, &ks, c.d_score, c.d_ncig, (uint32_t *)ctx->m_cig.p, c.d_coff,
	                      T.qoff.data(), T.toff.data(), T.bw.data(), sd, T.coff.data(), T.ex.data(), ctx->parent ? ctx->parent->arena_ev : nullptr,
	                      ctx->parent ? &dp_lock : nullptr, true /* this stage waits for sd below */);
	if (rc) { // kernels of this stage may already be queued in the shared arena: let them finish before the next lane takes its turn
		(void)hipStreamSynchronize(sd);
		return rc; // (the lock, if taken, is released by dp_lock's destructor)
	}
	c.mark("d:plan+enqueue");
	if (ctx->parent) {
		if (!ctx->own_arena) GD_HIP(hipEventRecord(ctx->parent->arena_ev, sd)); // the backtrack is done by then: the CIGARs sit in this lane's own buffer
		if (dp_lock.owns_lock()) dp_lock.unlock();
	}
	// P1 on the device, behind the backtrack of this stage (reads this lane's own windows and CIGAR slots, not the arena)
	if ((rc = gd_grow(ctx, ctx->m_post, sizeof(GdPostOut) * (size_t)nb))) { (void)hipStreamSynchronize(sd); return rc; }
	MapPostOpt PO;
	const int g_ = O.a, bb_ = O.b < 0 ? O.b : -O.b;
	for (int i = 0; i < 25; ++i) PO.mat[i] = (i / 5 == 4 || i % 5 == 4) ? 0 : (i / 5 == i % 5 ? (int8_t)g_ : (int8_t)bb_);
	PO.q = (int8_t)O.q, PO.e = (int8_t)O.e, PO.log_gap = !(O.flag & GD_F_SR);
	// A batch of wide-band alignments (the checkpointed kernels: four wavefronts of 128 registers per SIMD, i.e. no room for anything
	// else while they run): the device-to-host copies below are kernels of the runtime and would start only when DP wavefronts of
	// the NEXT batch retire -- ~1 s for 400 KB, and that second is part of the lane's cycle (kernel trace of the ONT path, round 2).
	// map_post_kernel starts in the gap between the two DP kernels, so it writes the results to page-locked host memory itself.
	// long alignments: one wavefront per alignment (mm_fix_cigar on lane 0, the walk over the bases by all lanes: 22 -> ~2 ms per HiFi
	// batch); short reads keep one alignment per thread (hundreds of thousands of 150-base walks).  GDIET_POST_WAVE=0 / 1 forces one.
	static const char *pw_env = getenv("GDIET_POST_WAVE");
	const bool eqx = c.is_sr && (O.flag & GD_F_EQX); // (--eqx: the ShortReads variant only; its rewrite is part of the thread-per-alignment kernel)
	const bool post_wave = !eqx && (pw_env ? atoi(pw_env) != 0 : T.coff[nb] / std::max(nb, 1) >= 2000);
	const bool xport = (ctx->last_mask & 8) != 0;
	if (xport) {
		const size_t need = sizeof(GdPostOut) * (size_t)nb + sizeof(int32_t) * 2 * nbp + 256;
		if (need > ctx->h_pin.cap) {
			(void)ctx->h_pin.release();
			ctx->h_pin.kind = DevBuf::PINNED;
			if (hipHostMalloc(&ctx->h_pin.p, need + need / 2, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); ctx->h_pin.p = nullptr; }
			else ctx->h_pin.cap = need + need / 2;
		}
	}
	const bool exported = xport && ctx->h_pin.p; // the DP results come to the host with map_post_kernel's own stores
	// outputs: the page-locked export buffer, else m_post (copied to h_post below, with the scores and CIGAR lengths)
	GdPostOut *o_post = (GdPostOut *)ctx->m_post.p;
	int32_t *o_score = nullptr, *o_ncig = nullptr;
	if (exported) {
		o_score = (int32_t *)ctx->h_pin.p, o_ncig = o_score + nbp, o_post = (GdPostOut *)(o_ncig + nbp);
		c.h_score = o_score, c.h_ncig = o_ncig, c.h_post = o_post;
	}
	gd_launch_post(post_wave, eqx, nb, (const MapBox *)ctx->m_boxes.p, (const uint8_t *)ctx->m_q.p, (const uint8_t *)ctx->m_t.p, (const int64_t *)c.d_coff,
	               (uint32_t *)ctx->m_cig.p, c.d_ncig, (const int32_t *)c.d_score, PO, o_post, o_score, o_ncig, sd);
	if (!exported) {
		GD_HIP(hipMemcpyAsync(ctx->h_post.p, ctx->m_post.p, sizeof(GdPostOut) * (size_t)nb, hipMemcpyDeviceToHost, sd));
		GD_HIP(hipMemcpyAsync(c.h_score, c.d_score, sizeof(int32_t) * 2 * nbp, hipMemcpyDeviceToHost, sd));
	}
	GD_HIP(gd_stream_wait(ctx, sd));
	c.mark("d:wait");
	return GDIET_OK;
}

// CIGARs are short compared with their capacity (qlen+tlen): pack them on the device, then one copy
static int gd_stage_pack(GdMapCall &c)
{
	gdiet_ctx *ctx = c.ctx;
	const GdBoxTables &T = c.T;
	const int nb = T.nb;
	std::vector<int64_t> &poff = c.poff;
	hipStream_t s = ctx->stream;
	int rc;
	for (int b = 0; b < nb; ++b) if (c.h_ncig[b] > T.coff[b + 1] - T.coff[b]) { ctx->err = "CIGAR capacity exceeded"; return GDIET_E_CIGAR_CAP; }
	poff.assign(nb + 1, 0);
	for (int b = 0; b < nb; ++b) poff[b + 1] = poff[b] + std::max(c.h_ncig[b], 0);
	if ((rc = gd_host_grow(ctx, ctx->h_cig, sizeof(uint32_t) * ((size_t)poff[nb] + 1)))) return rc;
	c.h_cig = (uint32_t *)ctx->h_cig.p;
	if (poff[nb] > 0) {
		if ((rc = gd_grow(ctx, ctx->m_pack, sizeof(uint32_t) * (size_t)poff[nb] + sizeof(int64_t) * (nb + 1) + 64))) return rc;
		int64_t *d_poff = (int64_t *)ctx->m_pack.p;
		uint32_t *d_packed = (uint32_t *)(d_poff + nb + 1);
		GD_HIP(hipMemcpyAsync(d_poff, poff.data(), sizeof(int64_t) * (nb + 1), hipMemcpyHostToDevice, s));
		hipLaunchKernelGGL(map_pack_cigar_kernel, dim3(nb), dim3(64), 0, s, nb, (const uint32_t *)ctx->m_cig.p, (const int64_t *)c.d_coff, (const int64_t *)d_poff, d_packed);
		GD_HIP(hipMemcpyAsync(c.h_cig, d_packed, sizeof(uint32_t) * (size_t)poff[nb], hipMemcpyDeviceToHost, s));
		GD_HIP(gd_stream_wait(ctx, s));
	}
	return GDIET_OK;
}

// P1-P3 (host threads): the records of every read, in slabs
static int gd_stage_records(GdMapCall &c)
{
	gdiet_ctx *ctx = c.ctx;
	const GdMapOpt &O = c.O;
	const GdBatchView &B = c.B;
	const GdBoxTables &T = c.T;
	const int n = B.n;
	const bool is_sr = c.is_sr;
	const GdRefView R = c.ix->h.ref();
	static std::atomic<uint64_t> call_counter{0};
	const uint64_t call_id = ++call_counter; // names the slabs of this call (GdRegSlab)
	std::atomic<int> no_mem{0};
	// (chunks of reads: the worker's scratch -- thread_local vectors, each access a call in a shared library -- is looked up once per chunk,
	// not six times per read; a short-read batch runs this body a quarter of a million times: chunks of 256 there)
	const int post_chunk = std::max(16, std::min(256, n / std::max(1, 8 * ctx->lane_threads))), n_post_chunks = (n + post_chunk - 1) / post_chunk; // (a long-read batch of 5 120 reads still spreads over every thread)
	gd_parallel_for(ctx, ctx->lane_threads, n_post_chunks, [&](int ch) {
		// scratch of the worker thread, reused from read to read (the workers are persistent)
		static thread_local std::vector<GdCand> C_tl;
		static thread_local std::vector<uint8_t> rev_tl;
		static thread_local std::vector<GdDpResult> dp_tl;
		static thread_local std::vector<GdReg> out_tl;
		std::vector<GdCand> &C = C_tl;
		std::vector<uint8_t> &rev = rev_tl;
		std::vector<GdDpResult> &dp = dp_tl;
		std::vector<GdReg> &out = out_tl;
		GdRegCursor &cursor = gd_reg_cursor();
		const int i_end = std::min(n, (ch + 1) * post_chunk);
		for (int i = ch * post_chunk; i < i_end; ++i) {
			c.n_regs[i] = 0, c.regs[i] = nullptr;
			const size_t nc = (size_t)T.ccount[i];
			if (!nc) continue;
			// the records grow CIGARs: this thread's copy.  (ShortReads: gd_sr_finish reads the box fields only, which gd_cand_unbox sets all of --
			// the elements are reused as they are; LongReads: fresh records, concatenate_cigars works inside them)
			if (is_sr) C.resize(nc);
			else C.assign(nc, GdCand());
			for (size_t j = 0; j < nc; ++j) gd_cand_unbox(T.cflat[(size_t)T.cfirst[i] + j], C[j]);
			const uint32_t rl = (uint32_t)(B.roff[i + 1] - B.roff[i]);
			const uint8_t *enc = B.enc + B.roff[i];
			// the reverse-complemented read: only where a reverse-strand candidate may be concatenated (P2)
			bool need_rev = false;
			for (auto &cd : C) need_rev |= cd.v.str != 0 && cd.next >= 0;
			if (need_rev) { rev.resize(rl); for (uint32_t j = 0; j < rl; ++j) rev[rl - 1 - j] = enc[j] ^ 3; }
			dp.resize(nc);
			for (size_t j = 0; j < nc; ++j) {
				const int b = T.box_first[i] + (int)j;
				dp[j].score = c.h_score[b], dp[j].n_cigar = c.h_ncig[b], dp[j].cigar = c.h_cig + c.poff[b];
			}
			out.clear();
			const GdPostOut *pre = c.h_post + T.box_first[i];
			if (is_sr) gd_sr_finish(C, dp, O, R, rl, enc, need_rev ? rev.data() : enc, out, pre);
			else gd_lr_finish(C, dp, O, R, rl, enc, need_rev ? rev.data() : enc, out, nullptr, pre);
			if (out.empty()) continue;
			bool head = false;
			void *at = gd_reg_slab_take(cursor, call_id, gd_regs_bytes(out), head);
			if (!at) { no_mem.store(1); continue; }
			gd_regs_fill(out, at, head, &c.n_regs[i], &c.regs[i]);
		}
	});
	if (no_mem.load()) { gdiet_hip_free_regs(n, c.n_regs, c.regs); ctx->err = "out of host memory for the records"; return GDIET_E_NOMEM; }
	return GDIET_OK;
}

// the whole per-read path for one slice, on ctx's own stream and buffers (ctx is a lane: the parent context or one of its children)
static int gd_map_range(gdiet_ctx *ctx, const gdiet_index *ix, const GdMapOpt &O, const GdBatchView &B, int32_t *n_regs, gdiet_reg_t **regs, GdSeedExport *sx = nullptr)
{
	GdMapCall c = {ctx, ix, O, B, n_regs, regs};
	(void)hipSetDevice(ctx->device);
	const int n = B.n;
	for (int i = 0; i < 6; ++i) ctx->stage_s[i] = 0;
	if (n == 0) return GDIET_OK;
	if (!sx) for (int i = 0; i < n; ++i) n_regs[i] = 0, regs[i] = nullptr; // whatever happens below, gdiet_hip_free_regs on these arrays is safe
	int rc;
	c.t0 = gd_now();
	if ((rc = gd_stage_setup(c))) return rc;
	gd_lap(c, 5);
	if ((rc = gd_stage_seed(c))) return rc;
	gd_lap(c, 0);
	c.mark("seed");
	if (sx) return gd_seed_export(c, *sx);
	if ((rc = gd_stage_vote(c))) return rc;
	if ((rc = c.sr_dev ? gd_stage_boxes_device(c) : gd_stage_boxes_host(c))) return rc; // (both close stage 1 behind the vote kernel, mark "vote")
	gd_lap(c, 2);
	c.mark("g:fill");
	if ((rc = gd_result_tables(c))) return rc;
	if (c.T.nb > 0) {
		if (!c.sr_dev && (rc = gd_upload_boxes(c))) return rc; // (device-side box stage: the tables are on the device already and the windows gathered)
		if ((rc = gd_stage_dp(c))) return rc;
		if ((rc = gd_stage_pack(c))) return rc;
	}
	gd_lap(c, 3);
	c.mark("d:pack");
	if ((rc = gd_stage_records(c))) return rc;
	ctx->stage_s[4] += gd_now() - c.t0;
	c.mark("post");
	if (c.mark.on) fprintf(stderr, "[gdiet stages, ms] lane=%p start=%.2f end=%.2f n=%d%s\n", (void *)ctx, 1e3 * fmod(c.mark.t0, 1000.0), 1e3 * fmod(gd_now(), 1000.0), n, c.mark.s.c_str());
	return GDIET_OK;
}


// the dispatch choices a lane (pipeline child or async lane) takes over from the context that drives it
static void gd_copy_lane_opts(gdiet_ctx *c, const gdiet_ctx *ctx)
{
	c->kernel_mode = ctx->kernel_mode, c->seed_thread_kernel = ctx->seed_thread_kernel, c->vote_wave = ctx->vote_wave;
	c->wide_two_waves = ctx->wide_two_waves, c->wide_ckpt = ctx->wide_ckpt;
}

extern "C" int gdiet_hip_set_map_lanes(gdiet_ctx *ctx, int n)
{
	if (!ctx || n < 1 || n > 16) return GDIET_E_PARAM;
	ctx->map_lanes = n;
	return GDIET_OK;
}

extern "C" int gdiet_hip_map_uploaded(gdiet_ctx *ctx, const gdiet_index *ix, const gdiet_mapopt_t *copt, gdiet_read_batch *B,
                                      int32_t *n_regs, gdiet_reg_t **regs)
{
	gd_err_clear();
	if (!ctx || !ix || !copt || !B || !n_regs || !regs) return GDIET_E_PARAM;
	(void)hipSetDevice(ctx->device);
	const int n = B->n;
	for (int i = 0; i < 6; ++i) ctx->stage_s[i] = 0;
	if (n == 0) return GDIET_OK;
	GdMapOpt O;
	gd_opt_from_c(copt, ix, O);
	{ const int rc = gd_check_opt(ctx, O); if (rc) return rc; }
	{ const int rc = gd_check_scoring(ctx, O); if (rc) return rc; }
	ctx->last_was_async = false;
	for (int i = 0; i < GD_MAX_INFLIGHT; ++i)
		if (ctx->async_busy[i]) { ctx->err = "batches submitted with gdiet_hip_map_submit are still in flight"; return GDIET_E_PARAM; }

	const int lanes = std::max(1, std::min(ctx->map_lanes, (n + 255) / 256));
	if (lanes == 1) {
		// the backtrace arena of a whole batch is ~40 % of HBM: lanes left over from a pipelined call must give theirs back first
		for (gdiet_ctx *c : ctx->children) gdiet_hip_destroy(c);
		ctx->children.clear();
		ctx->lane_threads = ctx->host_threads;
		ctx->last_mask = 0; // (a batch without a box launches no DP kernel: not the mask of an earlier call)
		GdBatchView V = {n, B->roff.data(), B->enc.data(), (const uint8_t *)B->d_reads, (const int64_t *)B->d_roff};
		return gd_map_range(ctx, ix, O, V, n_regs, regs);
	}
	// Software pipeline over slices of the batch: every lane (a child context with its own stream, workspace and host threads)
	// runs the whole chain for one slice at a time, so the latency-bound kernels (seed, vote, backtrack), the transfers and the
	// host stages of one slice overlap with the DP kernel of the others.  No result depends on the slicing.
	if (ctx->arena.p) { // ... and the parent's whole-batch arena is not needed while the lanes hold their own
		(void)hipStreamSynchronize(ctx->stream);
		(void)ctx->arena.release();
	}
	while ((int)ctx->children.size() < lanes) {
		gdiet_ctx *c = nullptr;
		int rc = gdiet_hip_init(&c, ctx->device);
		if (rc) { ctx->err = "cannot create a pipeline lane"; return rc; }
		gd_copy_lane_opts(c, ctx);
		ctx->children.push_back(c);
	}
	const int n_slices = std::min(n, lanes);
	std::atomic<int> next(0);
	std::vector<int> rcs(lanes, 0);
	std::vector<std::thread> th;
	for (int l = 0; l < lanes; ++l)
		th.emplace_back([&, l]() {
			gdiet_ctx *c = ctx->children[l];
			c->kernel_mode = ctx->kernel_mode;
			c->lane_threads = std::max(1, ctx->host_threads / lanes);
			double acc[6] = {0, 0, 0, 0, 0, 0};
			int mask = 0; // the union over this lane's slices of THIS call (a lane may take several, or none: then not what an earlier call left)
			for (;;) {
				const int sl = next.fetch_add(1);
				if (sl >= n_slices || rcs[l]) break;
				const int lo = (int)((int64_t)n * sl / n_slices), hi = (int)((int64_t)n * (sl + 1) / n_slices);
				GdBatchView V = {hi - lo, B->roff.data() + lo, B->enc.data(), (const uint8_t *)B->d_reads, (const int64_t *)B->d_roff + lo};
				c->last_mask = 0;
				rcs[l] = gd_map_range(c, ix, O, V, n_regs + lo, regs + lo);
				mask |= c->last_mask;
				for (int i = 0; i < 6; ++i) acc[i] += c->stage_s[i];
			}
			c->last_mask = mask;
			for (int i = 0; i < 6; ++i) c->stage_s[i] = acc[i];
		});
	for (auto &t : th) t.join();
	ctx->last_mask = 0, ctx->last_cells = 0, ctx->last_alg_bytes = 0, ctx->failed_last = 0;
	for (int l = 0; l < lanes; ++l) {
		gdiet_ctx *c = ctx->children[l];
		if (rcs[l]) { ctx->err = c->err; return rcs[l]; }
		if (c->failed_total) ctx->failed_last += c->failed_total, ctx->failed_total += c->failed_total, ctx->warn = c->warn, c->failed_total = 0; // (a lane maps several slices per call)
		for (int i = 0; i < 6; ++i) ctx->stage_s[i] += c->stage_s[i];
		ctx->last_mask |= c->last_mask;
	}
	return GDIET_OK;
}

// ---- several batches in flight ---------------------------------------------------------------------------------------------------
// gdiet_hip_map_submit starts the whole path for one resident batch on a lane of its own (stream, scratch) and returns;
// gdiet_hip_map_wait joins it.  The seeding / voting kernels and the host stages of one batch then run while the DP kernel of
// another owns the GPU; the DP stages themselves take turns in the shared backtrace arena.  The reference overlaps its mini-batches the same way (kt_pipeline, LR/map.c:2094-2170).  Results do not depend on it.
struct gdiet_map_ticket {
	std::thread th;
	int rc = 0, lane = 0;
	GdMapOpt O;
};

// gdiet_hip_destroy with tickets still open: their lane threads are joined (results dropped) before anything is released
static void gd_join_open_tickets(gdiet_ctx *ctx)
{
	std::vector<void *> open;
	{
		std::lock_guard<std::mutex> guard(ctx->async_mu);
		open.swap(ctx->open_tickets);
	}
	for (void *p : open) {
		gdiet_map_ticket *t = (gdiet_map_ticket *)p;
		if (t->th.joinable()) t->th.join();
		ctx->async_busy[t->lane] = false;
		delete t;
	}
}

extern "C" int gdiet_hip_set_inflight(gdiet_ctx *ctx, int n)
{
	if (!ctx || n < 1 || n > GD_MAX_INFLIGHT) return GDIET_E_PARAM;
	for (int i = 0; i < GD_MAX_INFLIGHT; ++i) if (ctx->async_busy[i]) { ctx->err = "batches are in flight"; return GDIET_E_PARAM; }
	gd_drop_async_lanes(ctx);
	ctx->async_depth = n, ctx->async_next = 0;
	// private backtrace arenas for the lanes when all of them fit beside the index and the batches' own buffers
	size_t free_b = 0, total_b = 0;
	(void)hipSetDevice(ctx->device);
	if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) (void)hipGetLastError(), total_b = 0;
	ctx->lane_arena_cap = n > 1 ? (size_t)((double)total_b * 0.70 / n) : 0;
	if (const char *e = getenv("GDIET_LANE_ARENA_GB")) ctx->lane_arena_cap = (size_t)(atof(e) * 1e9);
	return GDIET_OK;
}

extern "C" int gdiet_hip_map_submit(gdiet_ctx *ctx, const gdiet_index *ix, const gdiet_mapopt_t *copt, gdiet_read_batch *B, int32_t *n_regs,
                                    gdiet_reg_t **regs, gdiet_map_ticket **out)
{
	gd_err_clear();
	if (!ctx || !ix || !copt || !B || !n_regs || !regs || !out) return GDIET_E_PARAM;
	(void)hipSetDevice(ctx->device);
	std::lock_guard<std::mutex> guard(ctx->async_mu); // (submit and wait may come from different threads of the caller's pipeline)
	gdiet_map_ticket *t = new gdiet_map_ticket();
	gd_opt_from_c(copt, ix, t->O);
	int rc = gd_check_opt(ctx, t->O);
	if (!rc) rc = gd_check_scoring(ctx, t->O);
	if (rc) { delete t; return rc; }
	const int l = ctx->async_next % ctx->async_depth;
	if (ctx->async_busy[l]) { delete t; ctx->err = "too many batches in flight: wait for the oldest ticket first"; return GDIET_E_PARAM; }
	// the backtrace arenas are the big consumers of HBM: the intra-batch lanes give theirs back
	for (gdiet_ctx *c : ctx->children) gdiet_hip_destroy(c);
	ctx->children.clear();
	if (!ctx->async_lane[l]) {
		gdiet_ctx *c = nullptr;
		rc = gdiet_hip_init(&c, ctx->device);
		if (rc) { delete t; ctx->err = "cannot create an async lane"; return rc; }
		c->parent = ctx;
		ctx->async_lane[l] = c;
	}
	gdiet_ctx *c = ctx->async_lane[l];
	gd_copy_lane_opts(c, ctx);
	c->lane_threads = c->host_threads = ctx->host_threads; // all lanes draw from the parent's pool
	ctx->async_busy[l] = true, ctx->async_next++;
	c->last_mask = 0; // (as in gdiet_hip_map_uploaded: a batch without a box reports no kernel)
	t->lane = l;
	ctx->open_tickets.push_back(t);
	t->th = std::thread([=]() {
		GdBatchView V = {B->n, B->roff.data(), B->enc.data(), (const uint8_t *)B->d_reads, (const int64_t *)B->d_roff};
		t->rc = B->n ? gd_map_range(c, ix, t->O, V, n_regs, regs) : GDIET_OK;
	});
	*out = t;
	return GDIET_OK;
}

extern "C" int gdiet_hip_map_wait(gdiet_ctx *ctx, gdiet_map_ticket *t)
{
	gd_err_clear();
	if (!ctx || !t) return GDIET_E_PARAM;
	if (t->th.joinable()) t->th.join();
	bool rung_offered = false;
	uint64_t rung[2] = {0, 0};
	int rc;
	{
		std::lock_guard<std::mutex> guard(ctx->async_mu);
		for (size_t i = 0; i < ctx->open_tickets.size(); ++i)
			if (ctx->open_tickets[i] == t) { ctx->open_tickets.erase(ctx->open_tickets.begin() + i); break; }
		gdiet_ctx *c = ctx->async_lane[t->lane];
		rc = t->rc;
		if (rc) ctx->err = c->err;
		ctx->failed_last = c->failed_last, ctx->failed_total += c->failed_last;
		if (c->failed_last) ctx->warn = c->warn;
		for (int i = 0; i < 6; ++i) ctx->stage_s[i] = c->stage_s[i];
		ctx->last_mask = c->last_mask, ctx->last_cells = c->last_cells, ctx->last_alg_bytes = c->last_alg_bytes;
		if (!rc && c->last_cells) { // the lane's DP-stage events of this batch (its streams are idle: the thread has joined)
			ctx->last_was_async = false;
			if (gdiet_hip_last_kernel_ms(c, &ctx->async_dp_ms, &ctx->async_bt_ms) == GDIET_OK &&
			    gd_narrow_counters(c, ctx->async_narrow) == GDIET_OK) {
				ctx->last_was_async = true;
				rung_offered = c->narrow_launched && c->quarter_offered, rung[0] = ctx->async_narrow[2], rung[1] = ctx->async_narrow[3];
				if ((rc = gd_check_drained(ctx, ctx->async_narrow))) t->rc = rc;
			}
			ctx->last_arena_bytes = c->last_arena_bytes, ctx->drain_enqueued = c->drain_enqueued;
		}
		ctx->async_busy[t->lane] = false;
		delete t;
	}
	if (rung_offered && ctx->narrow_quarter < 0) { // auto mode learns from the launches that offered the quarter rung (after async_mu: a lane takes dp_mu first)
		std::lock_guard<std::mutex> guard(ctx->dp_mu);
		gd_quarter_auto_update(ctx->quarter_auto, rung[0], rung[1]);
	}
	return rc;
}

extern "C" int gdiet_hip_map_batch(gdiet_ctx *ctx, const gdiet_index *ix, const gdiet_mapopt_t *opt, int n, const char *const *seqs,
                                   const int32_t *lens, int32_t *n_regs, gdiet_reg_t **regs)
{
	gdiet_read_batch *b = nullptr;
	int rc = gdiet_hip_batch_upload(ctx, &b, n, seqs, lens);
	if (rc) return rc;
	rc = gdiet_hip_map_uploaded(ctx, ix, opt, b, n_regs, regs);
	gdiet_hip_batch_destroy(ctx, b);
	return rc;
}

// B2: the per-read level of the boundary, mm_map_frag's call shape (LR/minimap.h:390; LR/map.c:1273): one fragment of n_segs segments.
// As in the reference only segment 0 is sketched and aligned (SURVEY bug-compatibility item 7); the other segments get no records.
extern "C" int gdiet_hip_map_frag(gdiet_ctx *ctx, const gdiet_index *ix, const gdiet_mapopt_t *opt, int n_segs, const int32_t *qlens, const char *const *seqs,
                                  int32_t *n_regs, gdiet_reg_t **regs)
{
	if (!ctx || !ix || !opt || n_segs < 1 || !qlens || !seqs || !n_regs || !regs) return GDIET_E_PARAM;
	for (int i = 0; i < n_segs; ++i) n_regs[i] = 0, regs[i] = nullptr;
	if (qlens[0] <= 0) return GDIET_OK; // (LR/map.c:1288: qlen_sum == 0 returns without records)
	return gdiet_hip_map_batch(ctx, ix, opt, 1, seqs, qlens, n_regs, regs);
}

// B4: the sketch / seed level of the boundary for a batch of reads -- mm_sketch2 + mm_get_shift, mm_sketch3, mm_seed_mz_flt,
// mm_collect_matches2 (LR/mmpriv.h:65-76; LR/map.c:1296-1325) -- i.e. the output of the seeding kernel, copied out.
extern "C" int gdiet_hip_seed_batch(gdiet_ctx *ctx, const gdiet_index *ix, const gdiet_mapopt_t *copt, int n, const char *const *seqs, const int32_t *lens,
                                    int32_t *shift, uint32_t *tmp_extracted_len, uint32_t *n_mv, int64_t *seed_off, int64_t *occ_off, gdiet_seed_t **seeds,
                                    uint64_t **occ)
{
	gd_err_clear();
	if (!ctx || !ix || !copt || n < 0 || (n && (!seqs || !lens)) || !shift || !tmp_extracted_len || !n_mv || !seed_off || !occ_off || !seeds || !occ) return GDIET_E_PARAM;
	*seeds = nullptr, *occ = nullptr;
	seed_off[0] = occ_off[0] = 0;
	if (n == 0) return GDIET_OK;
	(void)hipSetDevice(ctx->device);
	for (int i = 0; i < GD_MAX_INFLIGHT; ++i)
		if (ctx->async_busy[i]) { ctx->err = "batches submitted with gdiet_hip_map_submit are still in flight"; return GDIET_E_PARAM; }
	GdMapOpt O;
	gd_opt_from_c(copt, ix, O);
	int rc = gd_check_opt(ctx, O);
	if (rc) return rc;
	{ std::string e; if (!gd_index_fetch_host(const_cast<gdiet_index *>(ix), e)) { ctx->err = e; return GDIET_E_HIP; } } // the occurrence lists are copied from the host tables
	gdiet_read_batch *b = nullptr;
	if ((rc = gdiet_hip_batch_upload(ctx, &b, n, seqs, lens))) return rc;
	for (gdiet_ctx *c : ctx->children) gdiet_hip_destroy(c);
	ctx->children.clear();
	ctx->lane_threads = ctx->host_threads;
	GdSeedExport sx;
	GdBatchView V = {n, b->roff.data(), b->enc.data(), (const uint8_t *)b->d_reads, (const int64_t *)b->d_roff};
	rc = gd_map_range(ctx, ix, O, V, nullptr, nullptr, &sx);
	gdiet_hip_batch_destroy(ctx, b);
	if (rc) return rc;
	for (int i = 0; i < n; ++i) {
		const MapSeedOut &o = sx.out[i];
		shift[i] = o.shift, tmp_extracted_len[i] = o.tel, n_mv[i] = o.n_mv;
		seed_off[i + 1] = seed_off[i] + (o.n_seeds > 0 ? o.n_seeds : 0), occ_off[i + 1] = occ_off[i] + (o.n_seeds > 0 ? o.n_a : 0);
	}
	gdiet_seed_t *sd = (gdiet_seed_t *)malloc(sizeof(gdiet_seed_t) * (size_t)std::max<int64_t>(seed_off[n], 1));
	uint64_t *oc = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)std::max<int64_t>(occ_off[n], 1));
	if (!sd || !oc) { free(sd), free(oc); ctx->err = "out of host memory"; return GDIET_E_NOMEM; }
	int64_t at = 0;
	for (int64_t j = 0; j < seed_off[n]; ++j) {
		const GdSeed &g = sx.seeds[(size_t)j];
		sd[j].n = g.n, sd[j].q_pos = g.q_pos;
		if (at + g.n > occ_off[n] || (uint64_t)g.start + g.n > ix->h.pos.size()) { free(sd), free(oc); ctx->err = "seed tables disagree"; return GDIET_E_HIP; } // (before the copy: oc holds occ_off[n])
		for (uint32_t t = 0; t < g.n; ++t) oc[at++] = ix->h.pos[(size_t)g.start + t];
	}
	if (at != occ_off[n]) { free(sd), free(oc); ctx->err = "seed tables disagree"; return GDIET_E_HIP; }
	*seeds = sd, *occ = oc;
	return GDIET_OK;
}

#include "map_diffstr_driver.hip.h"

extern "C" size_t gdiet_hip_sam_record(const gdiet_index *ix, const char *qname, const char *seq, const char *qual, int32_t l_seq,
                                       const gdiet_reg_t *regs, int32_t n_regs, int32_t reg_idx, int64_t opt_flag, char *buf, size_t cap)
{
	if (!ix) return 0;
	std::vector<GdReg> v(n_regs > 0 ? n_regs : 0);
	for (int i = 0; i < n_regs; ++i) gd_reg_from_c(regs[i], v[i]);
	std::string s;
	gd_write_sam(s, ix->h.ref(), qname, seq, qual, l_seq, v, reg_idx, opt_flag);
	if (buf && cap) { const size_t m = std::min(cap - 1, s.size()); memcpy(buf, s.data(), m); buf[m] = 0; }
	return s.size();
}

// All SAM records of a batch, in input order, formatted on the context's host threads (step 2 of the reference's pipeline prints
// them one read at a time on one thread: LR/map.c:2139-2170 -> mm_write_sam3).  A read without alignments gives its unmapped
// record; with MM_F_NO_PRINT_2ND secondary records are skipped, exactly as the reference's output loop does.
// chunk strings of the batch formatters, kept between calls (a chunk of HiFi records is megabytes: allocated fresh, every call pays
// for its pages again -- 300 MB of first touches per 5 120-read mini-batch)
static void gd_fmt_take(gdiet_ctx *ctx, std::vector<std::string> &rec)
{
	std::lock_guard<std::mutex> lk(ctx->enc_mu);
	for (std::string &r : rec) {
		if (ctx->fmt_pool.empty()) break;
		r.swap(ctx->fmt_pool.back()), ctx->fmt_pool.pop_back();
		r.clear();
	}
}
static void gd_fmt_give(gdiet_ctx *ctx, std::vector<std::string> &rec)
{
	std::lock_guard<std::mutex> lk(ctx->enc_mu);
	for (std::string &r : rec)
		if (ctx->fmt_pool.size() < 256 && r.capacity() > 4096) ctx->fmt_pool.emplace_back(), ctx->fmt_pool.back().swap(r);
}

// reads per chunk of the batch formatters: a few chunks per host thread, so that a mini-batch of 5 120 long reads keeps every thread busy
// (chunks of 512 reads gave ten), but never so small that a quarter of a million short reads become tens of thousands of strings
static int gd_fmt_chunk(const gdiet_ctx *ctx, int n_reads)
{
	const int want = n_reads / std::max(1, 6 * ctx->host_threads);
	return std::max(16, std::min(512, want));
}

static size_t gd_sam_batch_impl(gdiet_ctx *ctx, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs,
                                const char *const *quals, const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs,
                                int64_t opt_flag, char **buf_io, size_t *cap_io /* null: *buf_io is malloc'd to size */,
                                const char *const *comments = nullptr /* or entries */)
{
	// opt_flag bits read here and in gd_write_sam: MM_F_NO_PRINT_2ND, MM_F_SAM_HIT_ONLY (no record for a read without alignments,
	// LR/map.c:2177-2179), MM_F_NO_QUAL, MM_F_SOFTCLIP, MM_F_LONG_CIGAR, MM_F_COPY_COMMENT (comments are printed with it only), the cs /
	// MD bits; the context's read group (gdiet_hip_set_read_group) gives every record its RG:Z: tag
	const char *rg = ctx->rg_id.empty() ? nullptr : ctx->rg_id.c_str();
	if (!(opt_flag & GD_F_COPY_COMMENT)) comments = nullptr;
	// --cs / --MD: one difference-string call for the whole batch, on the device, before the chunks are formatted; every record's slice
	// is then appended behind its tags (mm_write_sam3 never passes qstrand: LR/format.c:594)
	GdDsText ds;
	if (gd_ds_mode(opt_flag) >= 0 && gd_ds_for_batch(ctx, ix, n_reads, seqs, lens, n_regs, regs, opt_flag & ~GD_F_QSTRAND, ds)) return 0;
	const int CH = gd_fmt_chunk(ctx, n_reads), n_ch = (n_reads + CH - 1) / CH;
	std::vector<std::string> rec((size_t)n_ch);
	gd_fmt_take(ctx, rec);
	gd_parallel_for(ctx, ctx->host_threads, n_ch, [&](int c) {
		static thread_local std::vector<GdReg> v; // per-thread scratch, reused from read to read
		std::string &s = rec[c];
		const int i1 = std::min(n_reads, (c + 1) * CH);
		size_t guess = 0;
		for (int i = c * CH; i < i1; ++i)
			guess += (2 * (size_t)lens[i] + 200 + (comments && comments[i] ? strlen(comments[i]) + 1 : 0) + ctx->rg_id.size()) * (size_t)std::max(1, n_regs[i]) + ds.bytes_of_read(i);
		s.reserve(guess);
		for (int i = c * CH; i < i1; ++i) {
			const int nr = n_regs[i];
			v.resize(nr > 0 ? nr : 0);
			for (int j = 0; j < nr; ++j) {
				gd_reg_from_c(regs[i][j], v[j]);
			}
			const char *q = quals ? quals[i] : nullptr, *cm = comments ? comments[i] : nullptr;
			if (nr <= 0) {
				if (opt_flag & GD_F_SAM_HIT_ONLY) continue;
				gd_write_sam(s, ix->h.ref(), qnames[i], seqs[i], q, lens[i], v, -1, opt_flag, nullptr, 0, rg, cm), s += '\n'; // (the writer appends)
			} else
				for (int j = 0; j < nr; ++j) {
					if ((opt_flag & GD_F_NO_PRINT_2ND) && v[j].id != v[j].parent) continue;
					gd_write_sam(s, ix->h.ref(), qnames[i], seqs[i], q, lens[i], v, j, opt_flag, ds.str(i, j), ds.len(i, j), rg, cm), s += '\n';
				}
		}
	});
	std::vector<size_t> at((size_t)n_ch + 1, 0);
	for (int c = 0; c < n_ch; ++c) at[c + 1] = at[c] + rec[c].size();
	const size_t tot = at[n_ch];
	char *buf;
	if (cap_io) { // the caller's buffer, grown when it is too small
		buf = *buf_io;
		if (!buf || *cap_io < tot + 1) {
			const size_t cap = tot + 1 + (tot >> 3);
			char *nb = (char *)realloc(buf, cap);
			if (!nb) { gd_fmt_give(ctx, rec); return 0; }
			buf = nb, *buf_io = nb, *cap_io = cap;
		}
	} else {
		buf = (char *)malloc(tot + 1);
		if (!buf) { gd_fmt_give(ctx, rec); return 0; }
		*buf_io = buf;
	}
	gd_parallel_for(ctx, ctx->host_threads, n_ch, [&](int c) { memcpy(buf + at[c], rec[c].data(), rec[c].size()); });
	buf[tot] = 0;
	gd_fmt_give(ctx, rec);
	return tot;
}

extern "C" size_t gdiet_hip_sam_batch(gdiet_ctx *ctx, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs,
                                      const char *const *quals, const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs,
                                      int64_t opt_flag, char **out)
{
	if (!ctx || !ix || n_reads < 0 || !qnames || !seqs || !lens || !n_regs || !regs || !out) return 0;
	*out = nullptr;
	return gd_sam_batch_impl(ctx, ix, n_reads, qnames, seqs, quals, lens, n_regs, regs, opt_flag, out, nullptr);
}

// the same into a buffer the caller keeps from mini-batch to mini-batch (*buf / *cap: start with NULL / 0; realloc'd when too small; free()
// it at the end): the text of a long-read mini-batch is ~150 MB, and a fresh allocation of that size is paid for page by page every time
extern "C" size_t gdiet_hip_sam_batch_into(gdiet_ctx *ctx, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs,
                                           const char *const *quals, const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs,
                                           int64_t opt_flag, char **buf, size_t *cap)
{
	if (!ctx || !ix || n_reads < 0 || !qnames || !seqs || !lens || !n_regs || !regs || !buf || !cap) return 0;
	return gd_sam_batch_impl(ctx, ix, n_reads, qnames, seqs, quals, lens, n_regs, regs, opt_flag, buf, cap);
}

// ... and with the reads' comments (gdiet_hip_fastx_read's array; NULL, or NULL entries, where there is none): -y
extern "C" size_t gdiet_hip_sam_batch_comments_into(gdiet_ctx *ctx, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs,
                                                    const char *const *quals, const char *const *comments, const int32_t *lens, const int32_t *n_regs,
                                                    gdiet_reg_t *const *regs, int64_t opt_flag, char **buf, size_t *cap)
{
	if (!ctx || !ix || n_reads < 0 || !qnames || !seqs || !lens || !n_regs || !regs || !buf || !cap) return 0;
	return gd_sam_batch_impl(ctx, ix, n_reads, qnames, seqs, quals, lens, n_regs, regs, opt_flag, buf, cap, comments);
}

// All PAF lines of a batch (mm_write_paf3, LR/format.c:326-367, as step 2 prints them when MM_F_OUT_SAM is off: LR/map.c:2163-2185).
// opt_flag: MM_F_OUT_CG adds the cg:Z: tag, MM_F_PAF_NO_HIT the lines of unmapped reads, MM_F_NO_PRINT_2ND drops secondary records,
// MM_F_COPY_COMMENT appends the read's comment to its mapped lines (:357; the unmapped line returns before it, :332).
// seqs == nullptr: gdiet_hip_paf_batch, which has no reads and hence no difference tags
static size_t gd_paf_batch_impl(gdiet_ctx *ctx, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs, const int32_t *lens,
                                const int32_t *n_regs, gdiet_reg_t *const *regs, int64_t opt_flag, char **out, const char *const *comments = nullptr)
{
	*out = nullptr;
	if (!(opt_flag & GD_F_COPY_COMMENT)) comments = nullptr;
	GdDsText ds; // --cs / --MD: as in gd_sam_batch_impl; MM_F_QSTRAND reaches the strings here (LR/format.c:355-356)
	if (seqs && gd_ds_mode(opt_flag) >= 0 && gd_ds_for_batch(ctx, ix, n_reads, seqs, lens, n_regs, regs, opt_flag, ds)) return 0;
	const int CH = 512, n_ch = (n_reads + CH - 1) / CH;
	std::vector<std::string> rec((size_t)n_ch);
	gd_parallel_for(ctx, ctx->host_threads, n_ch, [&](int c) {
		static thread_local std::vector<GdReg> v;
		std::string &s = rec[c];
		const int i1 = std::min(n_reads, (c + 1) * CH);
		for (int i = c * CH; i < i1; ++i) {
			const int nr = n_regs[i];
			v.resize(nr > 0 ? nr : 0);
			for (int j = 0; j < nr; ++j) {
				gd_reg_from_c(regs[i][j], v[j]);
			}
			if (nr <= 0) {
				if (opt_flag & GD_F_PAF_NO_HIT) gd_write_paf(s, ix->h.ref(), qnames[i], lens[i], v, -1, opt_flag), s += '\n';
			} else
				for (int j = 0; j < nr; ++j) {
					if ((opt_flag & GD_F_NO_PRINT_2ND) && v[j].id != v[j].parent) continue;
					gd_write_paf(s, ix->h.ref(), qnames[i], lens[i], v, j, opt_flag, ds.str(i, j), ds.len(i, j), comments ? comments[i] : nullptr), s += '\n';
				}
		}
	});
	size_t tot = 0;
	for (const std::string &r : rec) tot += r.size();
	char *buf = (char *)malloc(tot + 1);
	if (!buf) return 0;
	size_t at = 0;
	for (const std::string &r : rec) memcpy(buf + at, r.data(), r.size()), at += r.size();
	buf[tot] = 0;
	*out = buf;
	return tot;
}

extern "C" size_t gdiet_hip_paf_batch(gdiet_ctx *ctx, const gdiet_index *ix, int n_reads, const char *const *qnames, const int32_t *lens,
                                      const int32_t *n_regs, gdiet_reg_t *const *regs, int64_t opt_flag, char **out)
{
	if (!ctx || !ix || n_reads < 0 || !qnames || !lens || !n_regs || !regs || !out) return 0;
	return gd_paf_batch_impl(ctx, ix, n_reads, qnames, nullptr, lens, n_regs, regs, opt_flag, out);
}

// gdiet_hip_paf_batch with the reads: MM_F_OUT_CS / MM_F_OUT_CS_LONG / MM_F_OUT_MD add the cs:Z: / MD:Z: tag behind cg:Z: (LR/format.c:354-356)
extern "C" size_t gdiet_hip_paf_batch_seqs(gdiet_ctx *ctx, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs,
                                           const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs, int64_t opt_flag, char **out)
{
	if (!ctx || !ix || n_reads < 0 || !qnames || !seqs || !lens || !n_regs || !regs || !out) return 0;
	return gd_paf_batch_impl(ctx, ix, n_reads, qnames, seqs, lens, n_regs, regs, opt_flag, out);
}

// ... and with the reads' comments, as gdiet_hip_sam_batch_comments_into
extern "C" size_t gdiet_hip_paf_batch_comments(gdiet_ctx *ctx, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs,
                                               const char *const *comments, const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs,
                                               int64_t opt_flag, char **out)
{
	if (!ctx || !ix || n_reads < 0 || !qnames || !seqs || !lens || !n_regs || !regs || !out) return 0;
	return gd_paf_batch_impl(ctx, ix, n_reads, qnames, seqs, lens, n_regs, regs, opt_flag, out, comments);
}

// -R: sam_write_rg_line (LR/format.c:90-126).  The escaped line and the id live in the context: set before formatting starts
extern "C" int gdiet_hip_set_read_group(gdiet_ctx *ctx, const char *rg_line)
{
	if (!ctx) return GDIET_E_PARAM;
	ctx->rg_line.clear(), ctx->rg_id.clear();
	if (!rg_line) return GDIET_OK;
	std::string err;
	if (!gd_parse_rg_line(rg_line, ctx->rg_line, ctx->rg_id, err)) {
		gd_err_clear(); // (gdiet_hip_strerror is to return this text, not that of an earlier difference-string pass)
		ctx->err = err;
		return GDIET_E_PARAM;
	}
	return GDIET_OK;
}

// mm_write_sam_hdr (LR/format.c:128-148)
extern "C" size_t gdiet_hip_sam_header(gdiet_ctx *ctx, const gdiet_index *ix, const char *version, int argc, const char *const *argv, char **out)
{
	if (!ctx || !ix || !out || argc < 0 || (argc > 1 && !argv)) return 0;
	*out = nullptr;
	const std::string s = gd_sam_header(ix->h.ref(), ctx->rg_line, version, argc, argv);
	char *buf = (char *)malloc(s.size() + 1);
	if (!buf) return 0;
	memcpy(buf, s.c_str(), s.size() + 1);
	*out = buf;
	return s.size();
}
