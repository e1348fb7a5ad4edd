// What the accumulators over BAM records have in common: the coverage accumulator (cov_driver.hip.h), the pileup accumulator
// (pile_driver.hip.h) and the statistics accumulator (stats_driver.hip.h) derive from GdAccum and keep only their own tables, their open, their finish and their readers.  Included by
// bam_driver.hip.h behind the record encoder's driver and in front of the writer that feeds the attached accumulators (needs gdiet_ctx,
// GdLane, GdStreamMem, err_mark.h, GdAccumSet of bgzf_driver.hip.h, the BAM flattening and gd_bam_encode_device).
//
// An accumulator owns its arrays (plain hipMalloc: they live as long as the handle) and one small table that holds, among its own
// things, the cell of the first bad record.  Records reach it on THREE ROUTES, which end in its scatter kernel (GdAccum::launch) on
// whatever stream holds the records:
//   add_bam    host records: a walk for the starts (bam_starts.h), upload, scatter; on the lane gdiet_ctx::cov
//   add        a mapped batch: flattened and encoded by the BAM encoder's driver, scattered from the resident records on the encoder's
//              lane; nothing comes down
//   attached   gdiet_hip_bgzf_out_write_bam and the sorter's append hold the accumulators of their GdAccumSet (GdAccumHold), enqueue
//              the scatters behind the records they have just encoded, on the encoder's lane, before the records are compressed or
//              sorted (gd_accum_enqueue_all), and ask for the verdicts (gd_accum_verdict_all)
// On the last two routes the starts are GdbRec::out: nothing is walked, and one table of them serves every accumulator of the call.
// Every route synchronises its stream before it returns, so finish and the readers (on the lane cov) need no event.  One producer at a
// time: GdAccum::mu is held from the enqueue to the verdict.
// LOCK ORDER: bam.mu, then the coverage accumulator's mu, then the pileup accumulator's, then the statistics accumulator's (the slots of
// a GdAccumSet in order: GD_ACC_COV, GD_ACC_PILE, GD_ACC_STATS), then cov.mu of the context; cov_reg_mu is taken last and alone.
#pragma once
#include "cov.h"
#include "bam_starts.h"
#include "bam_flatten.h"

enum { GDC_MAX_BLOCKS = 8192 }; // of a scatter launch: the wavefronts stride over the table of starts

struct GdAccum {
	std::mutex mu;
	gdiet_ctx *ctx = nullptr;        // NULL once the context has been destroyed: the arrays went with it
	uint64_t *d_first_bad = nullptr; // the cell in the accumulator's table: min over a call's bad records of (index << 8 | reason).  NULL: no arrays
	uint64_t h_first_bad = ~(uint64_t)0;
	bool poisoned = false, finished = false;
	const char *const label; // "coverage" / "pileup" / "stats": the accumulator's name in every message
	explicit GdAccum(const char *name) : label(name) {}
	virtual ~GdAccum() {}
	// the scatter kernel over the n records at d_recs[0, bytes) whose starts are d_start[0, n), on s; blocks: one per four records, at most
	// GDC_MAX_BLOCKS (an accumulator whose kernel pays per block may launch fewer)
	virtual void launch(hipStream_t s, const uint8_t *d_recs, uint64_t bytes, const uint64_t *d_start, uint64_t n, unsigned blocks) = 0;
	virtual void free_arrays() = 0; // hipFree of what open allocated; the caller holds mu
};

static int gd_accum_fail(GdAccum *h, int rc, const char *who, const std::string &what) { return gd_err_fail(h ? h->ctx : nullptr, rc, std::string(who) + ": " + what); }

// 0, or -1 with why: the accumulator takes no more records
static int gd_accum_usable(GdAccum *h, std::string &why)
{
	if (!h->ctx || !h->d_first_bad) { why = std::string(h->label) + ": the context has been destroyed"; return -1; }
	if (h->poisoned) { why = std::string(h->label) + ": used after a bad record"; return -1; }
	if (h->finished) { why = std::string(h->label) + ": finished, the accumulator is read-only"; return -1; }
	return 0;
}

// h_start[0, n), n > 0, into a table of mem's on s; the caller keeps h_start alive until it has synchronised s.  0, or -1 with why
static int gd_accum_starts_up(const char *label, hipStream_t s, GdStreamMem &mem, const uint64_t *h_start, uint64_t n, uint64_t **d_start, std::string &why)
{
	hipError_t e = mem.alloc(d_start, 8 * (size_t)n + 16);
	const char *what = "starts";
	if (e == hipSuccess) e = hipMemcpyAsync(*d_start, h_start, 8 * (size_t)n, hipMemcpyHostToDevice, s), what = "starts copy";
	if (e == hipSuccess) return 0;
	why = std::string(label) + ": " + what + ": " + hipGetErrorString(e);
	return -1;
}

// The scatter of the n records at d_recs[0, bytes) whose starts are d_start[0, n) (resident, written by s or before it), enqueued on s;
// the caller holds h->mu, synchronises s and then asks gd_accum_verdict.  0, or -1 with why (the device failed).
static int gd_accum_enqueue(GdAccum *h, hipStream_t s, const uint8_t *d_recs, uint64_t bytes, const uint64_t *d_start, uint64_t n, std::string &why)
{
	hipError_t e = hipSuccess;
	auto fail = [&](hipError_t err, const char *what) {
		why = std::string(h->label) + ": " + what + ": " + hipGetErrorString(err);
		return -1;
	};
	h->h_first_bad = ~(uint64_t)0;
	if (n == 0) return 0;
	if ((e = hipMemsetAsync(h->d_first_bad, 0xff, 8, s)) != hipSuccess) return fail(e, "cell");
	h->launch(s, d_recs, bytes, d_start, n, (unsigned)std::min<uint64_t>((n + 3) / 4, GDC_MAX_BLOCKS));
	if ((e = hipGetLastError()) != hipSuccess) return fail(e, "scatter launch");
	if ((e = hipMemcpyAsync(&h->h_first_bad, h->d_first_bad, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "cell copy down");
	return 0;
}
// after the stream has been synchronised: 0, or GDIET_E_PARAM with why naming the call's first bad record (the accumulator is poisoned)
static int gd_accum_verdict(GdAccum *h, std::string &why)
{
	if (h->h_first_bad == ~(uint64_t)0) return 0;
	h->poisoned = true;
	why = std::string(h->label) + ": record " + std::to_string(h->h_first_bad >> 8) + " of the call: " + gdc_reason_text((uint32_t)(h->h_first_bad & 0xff));
	h->h_first_bad = ~(uint64_t)0;
	return GDIET_E_PARAM;
}

// ---- a call that feeds the accumulators of a set --------------------------------------------------------------------------------------
// The accumulators of a set, held for one call: locked in slot order, unlocked when the call ends.
struct GdAccumHold {
	GdAccum *a[GD_ACC_SLOTS] = {};
	std::vector<uint64_t> starts; // GdbRec::out of the call's records: alive until the stream has been synchronised
	// 0, or -1 with why and nothing held: an accumulator of the set takes no more records
	int take(const GdAccumSet &set, std::string &why)
	{
		for (int i = 0; i < GD_ACC_SLOTS; ++i) {
			GdAccum *h = set.slot[i];
			if (!h) continue;
			h->mu.lock();
			a[i] = h;
			if (gd_accum_usable(h, why)) { release(); return -1; }
		}
		return 0;
	}
	void release()
	{
		for (int i = GD_ACC_SLOTS - 1; i >= 0; --i)
			if (a[i]) a[i]->mu.unlock(), a[i] = nullptr;
	}
	~GdAccumHold() { release(); }
};
// the records of P, encoded at d_recs[0, P.bytes): one table of their starts goes up, every held accumulator's scatter runs behind it
static int gd_accum_enqueue_all(GdAccumHold &hold, hipStream_t s, const uint8_t *d_recs, const GdbPart &P, std::string &why)
{
	GdAccum *first = nullptr; // (its label names the table in a failure's text)
	for (GdAccum *h : hold.a)
		if (h && !first) first = h;
	if (!first) return 0; // (nothing without an attached accumulator)
	const size_t n = P.rec.size();
	hold.starts.resize(n);
	for (size_t k = 0; k < n; ++k) hold.starts[k] = P.rec[k].out;
	GdStreamMem mem(s); // (the table is freed behind the kernels, in stream order)
	uint64_t *d_start = nullptr;
	if (n && gd_accum_starts_up(first->label, s, mem, hold.starts.data(), n, &d_start, why)) return -1;
	for (GdAccum *h : hold.a)
		if (h && gd_accum_enqueue(h, s, d_recs, P.bytes, d_start, n, why)) return -1;
	return 0;
}
// after the stream has been synchronised.  Every held accumulator is asked before this returns, so a bad record poisons all of them; the
// text is that of the first in slot order that objects
static int gd_accum_verdict_all(GdAccumHold &hold, std::string &why)
{
	int rc = 0;
	for (GdAccum *h : hold.a) {
		std::string w;
		const int r = h ? gd_accum_verdict(h, w) : 0;
		if (r && !rc) rc = r, why = w;
	}
	return rc;
}
// gdiet_hip_bgzf_out_set_* / gdiet_hip_bam_sort_set_*: a (or none) into its slot of the holder's set
static int gd_accum_attach(gdiet_ctx *ctx, GdAccumSet &set, int slot, GdAccum *a, const char *who, const char *holder)
{
	gd_err_clear();
	if (a && (!ctx || a->ctx != ctx)) return gd_err_fail(ctx, GDIET_E_PARAM, std::string(who) + ": the " + holder + " and the accumulator need one context");
	set.slot[slot] = a;
	return GDIET_OK;
}

// ---- the entry points' common bodies: `who` is the entry point's name ------------------------------------------------------------------
static int gd_accum_add_bam(GdAccum *h, const char *who, const void *recs, size_t len)
{
	if (!h || (!recs && len)) return GDIET_E_PARAM;
	gd_err_clear();
	std::lock_guard<std::mutex> hk(h->mu);
	std::string why;
	if (gd_accum_usable(h, why)) return gd_accum_fail(h, GDIET_E_PARAM, who, why);
	std::vector<uint64_t> start;
	if (gd_record_starts(recs, len, start, why)) return gd_accum_fail(h, GDIET_E_PARAM, who, why);
	if (start.empty()) return GDIET_OK;
	gdiet_ctx *ctx = h->ctx;
	GdLane &L = ctx->cov;
	std::lock_guard<std::mutex> lk(L.mu);
	if (L.ready(ctx->device, 0, "coverage", why)) return gd_accum_fail(h, GDIET_E_HIP, who, why);
	hipStream_t s = L.stream;
	GdStreamMem mem(s);
	uint8_t *d_in;
	uint64_t *d_start;
	hipError_t e = hipSuccess;
	auto hip_fail = [&](hipError_t err, const char *what) {
		mem.fail();
		return gd_accum_fail(h, GDIET_E_HIP, who, std::string(h->label) + ": " + what + ": " + hipGetErrorString(err));
	};
	if ((e = mem.alloc(&d_in, len + 16)) != hipSuccess) return hip_fail(e, "records");
	if ((e = hipMemcpyAsync(d_in, recs, len, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e, "records copy");
	if (gd_accum_starts_up(h->label, s, mem, start.data(), start.size(), &d_start, why) || gd_accum_enqueue(h, s, d_in, len, d_start, start.size(), why)) {
		mem.fail();
		return gd_accum_fail(h, GDIET_E_HIP, who, why);
	}
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(e, "scatter kernel");
	const int rc = gd_accum_verdict(h, why);
	return rc ? gd_accum_fail(h, rc, who, why) : GDIET_OK;
}

static int gd_accum_add(GdAccum *h, const char *who, const gdiet_index *ix, int n_reads, const char *const *qnames, const char *const *seqs, const char *const *quals,
                        const int32_t *lens, const int32_t *n_regs, gdiet_reg_t *const *regs, const char *const *comments, int64_t opt_flag)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	gdiet_ctx *ctx;
	{
		std::lock_guard<std::mutex> hk(h->mu);
		ctx = h->ctx;
	}
	if (!ctx) return gd_accum_fail(h, GDIET_E_PARAM, who, std::string(h->label) + ": the context has been destroyed");
	if (!gd_bam_args_ok(ctx, ix, n_reads, qnames, seqs, lens, n_regs, regs)) return GDIET_E_PARAM;
	std::lock_guard<std::mutex> lk(ctx->bam.mu);
	GdAccumSet one; // (of this accumulator alone: any slot will do)
	one.slot[0] = h;
	GdAccumHold hold;
	std::string why;
	if (hold.take(one, why)) return gd_accum_fail(h, GDIET_E_PARAM, who, why);
	GdbPart &P = gd_bam_pool(ctx).all;
	int rc = gd_bam_flatten(ctx, ix, n_reads, qnames, seqs, quals, comments, lens, n_regs, regs, opt_flag, P, why);
	if (rc) return why.empty() ? rc : gd_accum_fail(h, rc, who, why);
	if (P.bytes == 0) return GDIET_OK;
	rc = gd_bam_encode_device(ctx, P, nullptr, 0, why, [&](uint8_t *d_stream, size_t, hipStream_t s) { // (the stream is synchronised when this has returned)
		return gd_accum_enqueue_all(hold, s, d_stream, P, why);
	});
	if (rc) return gd_accum_fail(h, GDIET_E_HIP, who, why);
	rc = gd_accum_verdict_all(hold, why);
	return rc ? gd_accum_fail(h, rc, who, why) : GDIET_OK;
}

// ---- the registry of the context: the accumulators opened on it and not yet closed ------------------------------------------------------
static void gd_accum_register(gdiet_ctx *ctx, GdAccum *h)
{
	std::lock_guard<std::mutex> rk(ctx->cov_reg_mu);
	ctx->accum_open.push_back(h);
}
static void gd_accum_free(GdAccum *h) // the caller holds h->mu (or is the only one who knows h)
{
	h->free_arrays();
	h->d_first_bad = nullptr;
}
// gdiet_hip_destroy: the arrays of the accumulators still open go with the context; their handles take nothing but close from then on
static void gd_accum_orphan_all(gdiet_ctx *ctx)
{
	std::vector<GdAccum *> open;
	{
		std::lock_guard<std::mutex> lk(ctx->cov_reg_mu);
		open.swap(ctx->accum_open);
	}
	for (GdAccum *h : open) {
		std::lock_guard<std::mutex> lk(h->mu);
		gd_accum_free(h);
		h->ctx = nullptr;
	}
}
static int gd_accum_close(GdAccum *h)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	{
		std::lock_guard<std::mutex> hk(h->mu);
		if (h->ctx) {
			(void)hipSetDevice(h->ctx->device);
			std::lock_guard<std::mutex> rk(h->ctx->cov_reg_mu);
			auto &v = h->ctx->accum_open;
			v.erase(std::remove(v.begin(), v.end(), h), v.end());
		}
		gd_accum_free(h);
	}
	delete h;
	return GDIET_OK;
}
