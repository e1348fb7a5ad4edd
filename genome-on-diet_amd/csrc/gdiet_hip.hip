// C-ABI shim (include/gdiet_hip.h) over the HIP kernels.  Host side is plain C++; no torch types anywhere.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <algorithm>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <functional>
#include <atomic>
#include <chrono>
#include <deque>
#include <unordered_map>
#include <memory>
#include <sched.h>

#include "../../include/gdiet_hip.h"
#include "err_mark.h"
#include "ksw_common.h"
#include "ksw_generic.hip.h"
#include "ksw_backtrack.hip.h"
#include "ksw_wave.hip.h"
#include "ksw_pipe.hip.h"
#include "ksw_extz2_exact.hip.h"
#include "ksw_exts2.hip.h"
#include "ksw_plan.h"

// A buffer a context keeps between batches.  It remembers which allocator made it (gd_grow: device memory, gd_host_grow: posix_memalign,
// the page-locked h_pin of map_pipeline.hip.h) and releases itself with the context that declares it.
struct DevBuf {
	enum Kind { DEVICE, PINNED, HOST };
	void *p = nullptr;
	size_t cap = 0;
	Kind kind = DEVICE;
	DevBuf() = default;
	DevBuf(const DevBuf &) = delete;
	DevBuf &operator=(const DevBuf &) = delete;
	~DevBuf() { (void)release(); }
	hipError_t release()
	{
		hipError_t e = hipSuccess;
		if (p && kind == HOST) free(p);
		else if (p) e = kind == PINNED ? hipHostFree(p) : hipFree(p);
		p = nullptr, cap = 0;
		return e;
	}
};

// A side lane of a context: a pass that runs beside the mapping path (difference strings, the reader's device mode, BGZF inflate and
// deflate, the BAM encoder) on a stream of its own behind a mutex of its own, so that its caller's thread never waits for a map call or an
// open ticket.  The stream and the events are made on first use and go with the context (gdiet_hip_destroy walks the lanes).
struct GdLane {
	std::mutex mu;
	hipStream_t stream = nullptr;
	hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; // around the steps of a call; a lane uses the first n_events
	double ms[3] = {0, 0, 0};                                                   // sums of their intervals since the context was created (under mu)
	// the caller holds mu.  0, or -1 with why = "<prefix>: stream: ..." / "<prefix>: event: ..."
	int ready(int device, int n_events, const char *prefix, std::string &why)
	{
		(void)hipSetDevice(device);
		hipError_t e = hipSuccess;
		if (!stream && (e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)) != hipSuccess) {
			why = std::string(prefix) + ": stream: " + hipGetErrorString(e);
			return -1;
		}
		for (int i = 0; i < n_events; ++i)
			if (!ev[i] && (e = hipEventCreate(&ev[i])) != hipSuccess) { ev[i] = nullptr; why = std::string(prefix) + ": event: " + hipGetErrorString(e); return -1; }
		return 0;
	}
};

// The stream-ordered allocations of one call on one stream (a plain hipMalloc / hipFree would synchronise every batch in flight).  What
// the call has not released or freed by its end is freed behind whatever it enqueued.  A call that fails with copies still in flight
// into its host vectors calls fail() first: the stream is synchronised before those vectors go out of scope.
struct GdStreamMem {
	hipStream_t s;
	std::vector<void *> held;
	explicit GdStreamMem(hipStream_t stream) : s(stream) {}
	GdStreamMem(const GdStreamMem &) = delete;
	GdStreamMem &operator=(const GdStreamMem &) = delete;
	~GdStreamMem() { drop(); }
	template <class T> hipError_t alloc(T **p, size_t bytes)
	{
		const hipError_t e = hipMallocAsync((void **)p, bytes, s);
		if (e == hipSuccess) held.push_back((void *)*p);
		else *p = nullptr;
		return e;
	}
	void release(const void *p) { held.erase(std::remove(held.begin(), held.end(), p), held.end()); } // p outlives the call: its new owner frees it
	void free_now(const void *p) { release(p), (void)hipFreeAsync(const_cast<void *>(p), s); }
	void drop()
	{
		for (void *p : held) (void)hipFreeAsync(p, s);
		held.clear();
	}
	void fail() { (void)hipStreamSynchronize(s), drop(); }
};

#define GD_MAX_INFLIGHT 8 // batches in flight per context (gdiet_hip_set_inflight)
struct GdAccum; // accum_driver.hip.h
struct gdiet_ctx {
	int device = 0;
	hipStream_t stream = nullptr;
	std::string err;
	char name[256] = {0};
	int kernel_mode = 0;
	int last_mask = 0;
	DevBuf arena;               // backtrace matrices
	DevBuf tasks, ids, status;  // per-batch descriptors
	DevBuf diag;                // per-alignment score of the main diagonal (ksw_exact_match_kernel -> ksw_backtrack_kernel)
	DevBuf pipes, pipe_runs, pipe_dst; // PipeWave / PipeRun records of the batch and the compacted id lists of its runs (ksw_pipe.hip.h)
	DevBuf qseq, tseq, score, ncig, cigar; // host-API staging
	hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
	hipStream_t stream_dp = nullptr;   // stream of the DP stage in an async lane
	int wave_slots = 5120;
	int dp_waves = 5;                  // wavefronts per SIMD the 64-lane DP kernel is launched for (gdiet_hip_set_dp_waves: 5 or 4)
	int wide_ckpt = -1;                // GDIET_WIDE_CKPT: 1 / 0 force / forbid the checkpointed wide-band kernel, default by batch size
	int wide_two_waves = -1;           // GDIET_WIDE_TWO_WAVES: 1 / 0 force the two-wavefront / two-blocks-per-lane kernel for wide bands, default by count
	int vote_wave = 1;                 // GDIET_VOTE_WAVE=0: the sequential vote kernel for long reads too
	int index_on_device = 1;           // GDIET_INDEX_BUILD=host: gdiet_hip_index_build sketches and sorts on host threads instead
	bool single_affine = false;        // set for the duration of a gdiet_hip_ksw_extz2_batch call: single-affine kernel variants
	GdPlan plan;                       // of the most recent DP batch (ksw_plan.h); its vectors are reused from batch to batch
	// per-read mapping path (map_pipeline.hip.h)
	DevBuf m_sc, m_mv, m_u64, m_seed, m_seedout, m_voteout, m_hitoff, m_hits, m_boxes, m_q, m_t, m_aux, m_cig, m_pack, m_post, m_seedids;
	DevBuf m_srbox, m_srtab, m_srscan, m_srcand; // device-side box stage of the ShortReads variant (map_pipeline.hip.h)
	int sr_boxes_on_device = 1;        // GDIET_SR_BOXES=host: candidate geometry of the ShortReads variant on host threads instead
	std::vector<uint8_t> h_vo;  // host copy of the vote records' heads, kept between batches
	DevBuf h_pin; // page-locked: scores, CIGAR lengths and P1 results of a wide-band batch, written by map_post_kernel itself
	DevBuf h_boxes, h_cand, h_tasks, h_seedout, h_res, h_cig, h_post; // HOST buffers kept between batches (gd_host_grow): the per-batch tables of a
	                                                           // short-read batch are tens of MB each, and allocated fresh they cost page faults
	int host_threads = 8;
	int lane_threads = 8;              // host threads this lane may use inside gd_map_range
	void *pool = nullptr;              // GdPool (map_pipeline.hip.h), created on first use
	// batches in flight (gdiet_hip_map_submit / _wait): up to GD_MAX_INFLIGHT lane contexts (own stream and scratch) that share THIS
	// context's backtrace arena, one DP stage at a time
	gdiet_ctx *parent = nullptr;       // set in an async lane
	std::mutex dp_mu;                  // orders the lanes' DP stages: held while one ENQUEUES its stage behind arena_ev
	hipEvent_t gather_ev = nullptr;    // this lane's windows are gathered (its DP stream waits for it)
	hipEvent_t wait_ev = nullptr;      // hipEventBlockingSync: the long waits of the mapping path sleep instead of spinning (gd_stream_wait)
	int blocking_wait = 0;             // GDIET_SYNC=block: wait on a hipEventBlockingSync event instead of hipStreamSynchronize
	hipEvent_t arena_ev = nullptr;     // recorded after the last DP stage that was enqueued: the arena is free once it has completed
	size_t lane_arena_cap = 0;         // a lane whose batch needs no more backtrace than this works in an arena of its own (set with the depth)
	bool own_arena = false;            // (lane) the last DP stage did
	bool shared_sticky = false;        // (lane) a recent batch did not fit a private arena
	gdiet_ctx *async_lane[GD_MAX_INFLIGHT] = {};
	bool async_busy[GD_MAX_INFLIGHT] = {};
	std::mutex async_mu;               // guards the ticket bookkeeping of submit / wait
	std::vector<void *> open_tickets;  // gdiet_map_ticket* submitted and not yet waited for (joined by gdiet_hip_destroy)
	std::vector<std::vector<uint8_t>> enc_pool; // host buffers of destroyed read batches, reused by the next uploads
	std::vector<std::string> fmt_pool;           // chunk strings of gdiet_hip_sam_batch / _paf_batch, reused (guarded by enc_mu)
	std::mutex enc_mu;
	int async_next = 0, async_depth = 2;
	bool last_was_async = false;       // gdiet_hip_last_kernel_ms then reports the lane's events, copied at gdiet_hip_map_wait
	float async_dp_ms = 0, async_bt_ms = 0;
	int map_lanes = 1;                 // software-pipeline depth of gdiet_hip_map_uploaded
	std::vector<gdiet_ctx *> children; // the lanes (child contexts on the same device)
	int seed_thread_kernel = 0;
	double stage_s[6] = {0, 0, 0, 0, 0, 0};
	uint64_t last_cells = 0, last_alg_bytes = 0; // of the most recent DP launch
	int narrow_band = 1;               // GDIET_NARROW_BAND=0: the 64-lane DP kernel runs every alignment at its full band (ksw_wave.hip.h, "NARROW BAND FIRST")
	DevBuf narrow_cnt;                 // six counters of the most recent 64-lane DP launch: alignments that tried a narrow band, certified ones; the same per rung (239, 495)
	bool narrow_launched = false;      // that launch had a 64-lane kernel at all
	uint64_t async_narrow[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; // the lane's counters, copied at gdiet_hip_map_wait
	DevBuf h_pending;                  // page-locked, one word: the length of the pending list, read back when the main launch has ended (gd_dp_launch)
	int drain_enqueued = 0;            // drain launches the most recent DP launch enqueued (a lane's: copied to the root at gdiet_hip_map_wait)
	size_t last_arena_bytes = 0;       // backtrace arena of the most recent planned batch (a lane's: copied to the root at gdiet_hip_map_wait)
	int narrow_quarter = -1;           // GDIET_NARROW_QUARTER: 0 never offers the quarter rung (band 239), 1 always, unset (-1): auto
	GdQuarterAuto quarter_auto;        // (root) auto mode: whether the next launches offer the rung (ksw_plan.h; read and written under dp_mu)
	bool quarter_offered = false;      // this context's most recent DP launch offered the rung
	// reads the most recent map call gave up on (a DP box outside its read / contig: undefined behaviour in the reference); they come back
	// with n_regs = 0 while the rest of the batch is mapped.  failed_total: since the context was created.
	int64_t failed_last = 0, failed_total = 0;
	std::string warn;                  // what the last such read was (gdiet_hip_map_failed_reads)
	// The side lanes (GdLane), each one apart from the mapping path's streams and from the others because:
	//   ds   cs / MD difference strings (map_diffstr_driver.hip.h): the formatters call it from a writer thread while map tickets are open
	//   fx   FASTQ blocks parsed and BAM blocks unpacked on the device (fastx_dev_driver.hip.h, bam_in_driver.hip.h): the reader thread of a
	//        file route calls it while map tickets are open
	//   bz   BGZF members inflated on the device (bgzf_driver.hip.h): the reader's I/O thread inflates the next block while its reader
	//        thread parses the current one under fx.mu.  ev[0..3]: copy up | kernel | copy down
	//   bzd  BGZF members written on the device (bgzf_driver.hip.h): a writer thread compresses the text of batch i while batch i + 1 maps
	//        and the reader inflates.  ev[0..5]: copy up | deflate kernel || pack kernel | copy down; ms: copy up, the two kernels, copy down
	//   bam  BAM records encoded, or SAM lines formatted (sam_driver.hip.h), on the device (bam_driver.hip.h): the same writer thread encodes batch i while batch i + 1 maps; it takes
	//        bam.mu, then bzd.mu when the deflate kernel reads the records where they are.  ev[0..3]: copy up | encode kernel | copy down
	//   bsort BAM records put into coordinate order on the device (bam_sort_driver.hip.h): apart from bam, so that a caller that sorts a buffer
	//        never holds the encoder's mutex.  ev[0..2]: key, sort and scan | gather
	//   cov  the accumulators' own lane (accum_driver.hip.h): coverage or a pileup accumulated from host records, coverage's scan and window
	//        reduction, the pileup's calls (cov_driver.hip.h, pile_driver.hip.h): apart from bam, so that a caller that finishes or reads one
	//        accumulator never holds the encoder's mutex.  No events
	GdLane ds, fx, bz, bzd, bam, bsort, cov;
	template <class F> void each_lane(F f) { f(ds), f(fx), f(bz), f(bzd), f(bam), f(bsort), f(cov); }
	std::vector<GdAccum *> accum_open; // the coverage, pileup and statistics accumulators opened on this context and not yet closed: their arrays go with it (accum_driver.hip.h; under cov_reg_mu)
	std::mutex cov_reg_mu;
	DevBuf ds_rec, ds_cig, ds_len, ds_off, ds_scan, ds_text, ds_reads, ds_roff; // (under ds.mu)
	std::vector<uint8_t> ds_enc;       // host copy of the reads a difference-string call without a resident batch encodes
	DevBuf fx_scan;                    // the scan's scratch of the FASTQ parser (under fx.mu)
	std::shared_ptr<void> bam_pool;    // GdbPool (bam_driver.hip.h): the flattened chunks of a batch and their merged table, kept from call to call (under bam.mu)
	std::shared_ptr<void> sam_pool;    // GdsPool (sam_driver.hip.h): the same for SAM lines formatted on the device (under bam.mu)
	std::string rg_line, rg_id;        // -R: the escaped @RG header line and its ID (gdiet_hip_set_read_group; read by the SAM formatters)
};

#define GD_HIP(call)                                                                              \
	do {                                                                                          \
		hipError_t e__ = (call);                                                                  \
		if (e__ != hipSuccess) {                                                                  \
			ctx->err = std::string(#call) + ": " + hipGetErrorString(e__);                        \
			return GDIET_E_HIP;                                                                   \
		}                                                                                         \
	} while (0)

// The long waits of the mapping path (a lane waits ~100 ms for a HiFi DP stage).  Default: hipStreamSynchronize -- measured on the
// GPU box it costs no CPU time worth mentioning (56.2 s of process CPU either way over a 20 s bench run: the runtime sleeps on the
// completion signal after a short spin) and wakes up faster.  GDIET_SYNC=block waits on a hipEventBlockingSync event instead
// (-2 % HiFi, -11 % ShortReads throughput): for hosts where the runtime's wait does spin.
static hipError_t gd_stream_wait(gdiet_ctx *ctx, hipStream_t s)
{
	if (!ctx->blocking_wait || !ctx->wait_ev) return hipStreamSynchronize(s);
	hipError_t e = hipEventRecord(ctx->wait_ev, s);
	if (e != hipSuccess) return e;
	return hipEventSynchronize(ctx->wait_ev);
}

static int gd_grow(gdiet_ctx *ctx, DevBuf &b, size_t bytes)
{
	if (bytes <= b.cap) return GDIET_OK;
	// growth is rare (first batches); it synchronises the stream because older work may still read the buffer
	GD_HIP(hipStreamSynchronize(ctx->stream));
	GD_HIP(b.release());
	b.kind = DevBuf::DEVICE;
	size_t want = bytes + (bytes >> 3) + 4096;
	hipError_t e = hipMalloc(&b.p, want);
	if (e != hipSuccess) {
		(void)hipGetLastError();
		want = bytes;
		e = hipMalloc(&b.p, want);
	}
	if (e != hipSuccess) {
		(void)hipGetLastError();
		ctx->err = "hipMalloc of " + std::to_string(bytes) + " bytes failed: " + hipGetErrorString(e);
		b.p = nullptr;
		return GDIET_E_NOMEM;
	}
	b.cap = want;
	if (getenv("GDIET_TRACE_ALLOC")) fprintf(stderr, "[gdiet] device buffer grown to %zu bytes\n", want);
	return GDIET_OK;
}

// CPUs this process may really use: the smallest of the hardware count, the affinity mask and the cgroup CPU quota (a container
// with a 16-CPU quota on a 256-thread host must not run 256 workers: they are throttled together every scheduling period)
static int gd_effective_cpus()
{
	int n = (int)std::max(1u, std::thread::hardware_concurrency());
	cpu_set_t set;
	CPU_ZERO(&set);
	if (sched_getaffinity(0, sizeof(set), &set) == 0 && CPU_COUNT(&set) > 0) n = std::min(n, CPU_COUNT(&set));
	if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) { // cgroup v2: "<quota|max> <period>"
		char q[64];
		long long period = 0;
		if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") && period > 0) n = std::min<long long>(n, std::max<long long>(1, (atoll(q) + period - 1) / period));
		fclose(f);
	} else {
		long long quota = -1, period = 0;
		if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(g, "%lld", &quota) != 1) quota = -1; fclose(g); }
		if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(g, "%lld", &period) != 1) period = 0; fclose(g); }
		if (quota > 0 && period > 0) n = std::min<long long>(n, std::max<long long>(1, (quota + period - 1) / period));
	}
	return n;
}

extern "C" int gdiet_hip_effective_cpus(void) { return gd_effective_cpus(); }

extern "C" int gdiet_hip_init(gdiet_ctx **out, int device)
{
	if (!out) return GDIET_E_PARAM;
	*out = nullptr;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return GDIET_E_NODEVICE;
	gdiet_ctx *ctx = new gdiet_ctx();
	ctx->device = device;
	hipDeviceProp_t prop;
	if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) {
		delete ctx;
		return GDIET_E_NODEVICE;
	}
	snprintf(ctx->name, sizeof(ctx->name), "%s (%s)", prop.name, prop.gcnArchName);
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) { // the code object is gfx950-only; fail loudly, no fallback
		delete ctx;
		return GDIET_E_NODEVICE;
	}
	if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
		delete ctx;
		return GDIET_E_HIP;
	}
	for (int i = 0; i < 4; ++i)
		if (hipEventCreate(&ctx->ev[i]) != hipSuccess) {
			delete ctx;
			return GDIET_E_HIP;
		}
	{
		int lo = 0, hi = 0; // numerically lower = higher priority
		(void)hipDeviceGetStreamPriorityRange(&lo, &hi);
		// the least priority: a raised one measured no gain, the separate stream is what matters
		if (hipStreamCreateWithPriority(&ctx->stream_dp, hipStreamNonBlocking, lo) != hipSuccess) { delete ctx; return GDIET_E_HIP; }
	}
	if (hipEventCreateWithFlags(&ctx->wait_ev, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) { delete ctx; return GDIET_E_HIP; }
	{ const char *sy = getenv("GDIET_SYNC"); if (sy) ctx->blocking_wait = strcmp(sy, "block") == 0; }
	if (hipEventCreateWithFlags(&ctx->arena_ev, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ctx->gather_ev, hipEventDisableTiming) != hipSuccess) { delete ctx; return GDIET_E_HIP; }
	ctx->wave_slots = prop.multiProcessorCount * 4 * 5; // CUs x SIMDs x resident wavefronts of the 64-lane DP kernel (94 VGPRs)
	ctx->host_threads = std::min(64, gd_effective_cpus());
	{
		const char *e = getenv("GDIET_SEED_KERNEL");
		ctx->seed_thread_kernel = e && !strcmp(e, "thread") ? 1 : e && !strcmp(e, "wave") ? 2 : 0; // 0: by read length
		const char *tw = getenv("GDIET_WIDE_TWO_WAVES");
		if (tw) ctx->wide_two_waves = atoi(tw) != 0;
		const char *wc = getenv("GDIET_WIDE_CKPT");
		if (wc) ctx->wide_ckpt = atoi(wc) != 0;
		const char *vw = getenv("GDIET_VOTE_WAVE");
		if (vw) ctx->vote_wave = atoi(vw) != 0;
		const char *ib = getenv("GDIET_INDEX_BUILD");
		if (ib) ctx->index_on_device = strcmp(ib, "host") != 0;
		const char *sb = getenv("GDIET_SR_BOXES");
		if (sb) ctx->sr_boxes_on_device = strcmp(sb, "host") != 0;
		const char *nb = getenv("GDIET_NARROW_BAND");
		if (nb) ctx->narrow_band = atoi(nb) != 0;
		const char *nq = getenv("GDIET_NARROW_QUARTER");
		if (nq) ctx->narrow_quarter = atoi(nq) != 0;
	}
	*out = ctx;
	return GDIET_OK;
}

static void gd_pool_free(void *pool); // map_pipeline.hip.h
template <class F> static void gd_parallel_for(gdiet_ctx *ctx, int n_threads, int n, F f); // map_pipeline.hip.h
static void gd_join_open_tickets(gdiet_ctx *ctx);
static void gd_accum_orphan_all(gdiet_ctx *ctx); // accum_driver.hip.h

extern "C" void gdiet_hip_destroy(gdiet_ctx *ctx)
{
	if (!ctx) return;
	gd_join_open_tickets(ctx); // batches still in flight run to their end first: their lanes use this context's pool, arena and streams
	if (ctx->pool) gd_pool_free(ctx->pool), ctx->pool = nullptr;
	for (gdiet_ctx *c : ctx->children) gdiet_hip_destroy(c);
	ctx->children.clear();
	for (int i = 0; i < GD_MAX_INFLIGHT; ++i)
		if (ctx->async_lane[i]) gdiet_hip_destroy(ctx->async_lane[i]), ctx->async_lane[i] = nullptr;
	(void)hipSetDevice(ctx->device);
	if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
	gd_accum_orphan_all(ctx); // the arrays of the coverage, pileup and statistics accumulators that are still open
	std::vector<hipEvent_t> events(ctx->ev, ctx->ev + 4);
	events.insert(events.end(), {ctx->arena_ev, ctx->wait_ev, ctx->gather_ev});
	std::vector<hipStream_t> streams{ctx->stream_dp, ctx->stream};
	ctx->each_lane([&](GdLane &l) { // (a lane that was never used has neither)
		if (l.stream) (void)hipStreamSynchronize(l.stream);
		events.insert(events.end(), l.ev, l.ev + 6), streams.push_back(l.stream);
	});
	delete ctx; // every DevBuf of the context releases itself here: before the streams and events go
	for (hipEvent_t e : events)
		if (e) (void)hipEventDestroy(e);
	for (hipStream_t s : streams)
		if (s) (void)hipStreamDestroy(s);
}

#ifdef GD_CLOCK_STAMP
// measurement build only (tools/clock_probe.py; not declared in include/gdiet_hip.h): the raw per-wavefront stamps
extern "C" int gdiet_hip_debug_clock_stamps(unsigned long long *out, int n_slots)
{
	if (n_slots > GD_CLOCK_SLOTS) n_slots = GD_CLOCK_SLOTS;
	return hipMemcpyFromSymbol(out, HIP_SYMBOL(gd_clock_stamps), sizeof(unsigned long long) * 4 * (size_t)n_slots) == hipSuccess ? n_slots : -1;
}
#endif
// the clock stamps of the 64-lane DP kernel's wavefronts (ksw_wave.hip.h), reduced: per wavefront sclk = ticks(s_memtime) /
// ticks(s_memrealtime) x 100 MHz.  Call after the batch has completed.
extern "C" int gdiet_hip_last_dp_clock(gdiet_ctx *ctx, double *sclk_mhz_median, double *sclk_mhz_min, double *wavefront_ms_median)
{
	if (!ctx) return GDIET_E_PARAM;
	(void)hipSetDevice(ctx->device);
	std::vector<unsigned long long> st((size_t)GD_CLOCK_SLOTS * 4);
	GD_HIP(hipMemcpyFromSymbol(st.data(), HIP_SYMBOL(gd_clock_stamps), sizeof(unsigned long long) * st.size()));
	std::vector<double> f, ms;
	for (int i = 0; i < GD_CLOCK_SLOTS; ++i) {
		const unsigned long long mt0 = st[4 * i], rt0 = st[4 * i + 1], mt1 = st[4 * i + 2], rt1 = st[4 * i + 3];
		if (rt1 > rt0 && mt1 > mt0 && rt1 - rt0 > 1000) f.push_back((double)(mt1 - mt0) / (double)(rt1 - rt0) * 100.0), ms.push_back((double)(rt1 - rt0) * 1e-5); // (>= 10 us)
	}
	if (f.empty()) { ctx->err = "no 64-lane DP kernel has run yet"; return GDIET_E_PARAM; }
	std::sort(f.begin(), f.end()), std::sort(ms.begin(), ms.end());
	if (sclk_mhz_median) *sclk_mhz_median = f[f.size() / 2];
	if (sclk_mhz_min) *sclk_mhz_min = f.front();
	if (wavefront_ms_median) *wavefront_ms_median = ms[ms.size() / 2];
	return GDIET_OK;
}


extern "C" const char *gdiet_hip_strerror(const gdiet_ctx *ctx)
{
	if (const char *mine = gd_err_text(ctx)) return mine; // this thread's last failure on the context (or without one) was on a side lane (err_mark.h)
	return ctx ? ctx->err.c_str() : "no context";
}

extern "C" int gdiet_hip_device_name(const gdiet_ctx *ctx, char *buf, size_t len)
{
	if (!ctx || !buf || !len) return GDIET_E_PARAM;
	snprintf(buf, len, "%s", ctx->name);
	return GDIET_OK;
}

extern "C" int gdiet_hip_last_kernel_mask(const gdiet_ctx *ctx) { return ctx ? ctx->last_mask : 0; }

extern "C" int gdiet_hip_set_kernel_mode(gdiet_ctx *ctx, int mode)
{
	if (!ctx || mode < 0 || mode > 2) return GDIET_E_PARAM;
	ctx->kernel_mode = mode;
	return GDIET_OK;
}

extern "C" int gdiet_hip_set_dp_waves(gdiet_ctx *ctx, int waves_per_simd)
{
	if (!ctx || (waves_per_simd != 4 && waves_per_simd != 5)) return GDIET_E_PARAM;
	ctx->dp_waves = waves_per_simd;
	return GDIET_OK;
}

extern "C" int gdiet_hip_reserve(gdiet_ctx *ctx, size_t bytes)
{
	if (!ctx) return GDIET_E_PARAM;
	(void)hipSetDevice(ctx->device);
	return gd_grow(ctx, ctx->arena, bytes);
}

// ---- planning ----------------------------------------------------------------------------------------------

// what the planner (ksw_plan.h) takes from the environment
static const int gd_group_lanes = getenv("GDIET_GROUP_LANES") ? atoi(getenv("GDIET_GROUP_LANES")) : 0; // 16: always four alignments per wavefront
// GDIET_SR_PIPE=0: no skewed pipelines (ksw_pipe.hip.h), short alignments on the grouped kernels only
static const bool gd_use_pipe = !(getenv("GDIET_SR_PIPE") && atoi(getenv("GDIET_SR_PIPE")) == 0);
// GDIET_BT_COMPACT=0: every backtrace slot is sized for the full-band rows, no overflow pool, no drain launches (ksw_plan.h)
static const bool gd_bt_compact = !(getenv("GDIET_BT_COMPACT") && atoi(getenv("GDIET_BT_COMPACT")) == 0);
// GDIET_BT_OVERFLOW_MB: size of the overflow pool of the compact arena (default: a sixteenth of the slots)
static const int64_t gd_bt_overflow_bytes = getenv("GDIET_BT_OVERFLOW_MB") ? (int64_t)(atof(getenv("GDIET_BT_OVERFLOW_MB")) * 1048576.0) : -1;

extern "C" size_t gdiet_hip_ksw_workspace_bytes(int n, const int64_t *qoff, const int64_t *toff, const int32_t *w)
{
	size_t tot = 0;
	GdPlanOpt plan_opt;
	plan_opt.group_lanes = gd_group_lanes, plan_opt.use_pipe = gd_use_pipe;
	for (int i = 0; i < n; ++i) {
		const int qlen = (int)(qoff[i + 1] - qoff[i]), tlen = (int)(toff[i + 1] - toff[i]);
		if (qlen <= 0 || tlen <= 0) continue;
		int32_t kind, rb;
		gd_plan_one(plan_opt, qlen, tlen, w[i], kind, rb);
		const size_t a = (size_t)(qlen + tlen - 1) * (size_t)rb;
		const size_t b = (size_t)(qlen + tlen - 1) * (size_t)gd_ncol16(qlen, tlen, w[i]) * 16; // forced-generic worst case
		tot += gd_align256(std::max(a, b) + 64);
	}
	return tot;
}

static int gd_consts(gdiet_ctx *ctx, const gdiet_ksw_score_t *sc, KswConst &K)
{
	if (!sc) { ctx->err = "scoring is NULL"; return GDIET_E_PARAM; }
	if (sc->flag != GDIET_EZ_APPROX_MAX) {
		ctx->err = "only flag == GDIET_EZ_APPROX_MAX (the live path's mode) is implemented";
		return GDIET_E_PARAM;
	}
	K = gd_derive_consts(sc->match, sc->mismatch, sc->sc_ambi, sc->q, sc->e, sc->q2, sc->e2).K; // (ksw_common.h: shared with the host emulators)
	const int q = K.q, e = K.e, q2 = K.q2, e2 = K.e2;
	// :96-100 early return "if (-min_sc > 2 * (q + e)) return" leaves score = NEG_INF for every pair; the live
	// path can never get there (mm_check_opt), so it is reported as a parameter error instead.
	int min_sc = std::min<int>(std::min<int>(sc->mismatch, sc->match), std::min<int>(sc->sc_ambi, 0));
	if (-min_sc > 2 * (q + e)) { ctx->err = "-min_sc > 2*(q+e): the reference returns without aligning"; return GDIET_E_PARAM; }
	if ((q + e) + (q2 + e2) > 127) { ctx->err = "(q+e)+(q2+e2) > 127 (mm_check_opt, options.c:218)"; return GDIET_E_PARAM; }
	return GDIET_OK;
}

// host buffer that only grows and is kept between batches (contents are not preserved).  Plain pageable memory: pinning these
// was measured -- neutral for short reads, and 2-3 % slower for HiFi batches (the asynchronous device-to-host copy of the DP
// results then waits behind the other batches' kernels instead of being staged at once).
static int gd_host_grow(gdiet_ctx *ctx, DevBuf &b, size_t bytes)
{
	if (bytes <= b.cap) return GDIET_OK;
	(void)b.release();
	b.kind = DevBuf::HOST;
	const size_t want = bytes + (bytes >> 2) + 4096;
	if (posix_memalign(&b.p, 256, want)) b.p = nullptr; // (256-byte aligned: the runtime's copy kernels pick their form by the alignment of both ends)
	if (!b.p) { ctx->err = "out of host memory (" + std::to_string(want) + " bytes)"; return GDIET_E_NOMEM; }
	b.cap = want;
	return GDIET_OK;
}

// ---- device-pointer entry point ----------------------------------------------------------------------------

static double gd_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// GDIET_TRACE_STAGES=1: wall time of the host-side steps of a call to stderr (development aid).  trace("name") closes a step; the
// caller prints `s` behind a head of its own, one line per call.
static bool gd_trace_stages() { static const bool on = getenv("GDIET_TRACE_STAGES") != nullptr; return on; }
struct GdStageTrace {
	const bool on = gd_trace_stages();
	const double t0 = on ? gd_now() : 0;
	double t = t0;
	std::string s;
	GdStageTrace() = default;
	GdStageTrace(const GdStageTrace &) = delete; // (the steps of a call add up in ONE trace: pass it by reference)
	void operator()(const char *what)
	{
		if (!on) return;
		const double now = gd_now();
		char b[64];
		snprintf(b, sizeof b, " %s %.2f", what, 1e3 * (now - t));
		s += b, t = now;
	}
};

// The launches of a planned batch on `stream`, its descriptors uploaded: the exact-match pre-filter, the DP kernels of the four kinds over
// their id lists, the walks they left, the score bias; ctx->ev[0..2] before the first, after the DP and after the last.
static int gd_dp_launch(gdiet_ctx *ctx, const GdPlan &P, int n, const KswConst &K, const gdiet_ksw_score_t *sc, const uint8_t *d_qseq, const uint8_t *d_tseq,
                        uint8_t *d_bt, int32_t *d_score, int32_t *d_n_cigar, uint32_t *d_cigar, hipStream_t stream, hipEvent_t arena_free,
                        bool host_decides /* the caller waits for `stream` anyway and nothing of another batch is queued behind this stage: see the drain launches */)
{
	int rc;
	const KswTask *d_tasks = (const KswTask *)ctx->tasks.p;
	const int32_t *d_ids = (const int32_t *)ctx->ids.p;
	int32_t *d_status = (int32_t *)ctx->status.p;

	if (arena_free) GD_HIP(hipStreamWaitEvent(stream, arena_free, 0)); // descriptors are across; only the kernels queue behind the arena's last user
	GD_HIP(hipEventRecord(ctx->ev[0], stream));
	// (GDIET_DIAG_SHORTCUT=0: every short alignment goes through the DP and is walked back, also those the pre-filter could answer from the
	// main diagonal's score -- see ksw_exact_match_kernel)
	static const bool diag_shortcut = !(getenv("GDIET_DIAG_SHORTCUT") && atoi(getenv("GDIET_DIAG_SHORTCUT")) == 0);
	const int score_bias = gd_derive_consts(sc->match, sc->mismatch, sc->sc_ambi, sc->q, sc->e, sc->q2, sc->e2).score_bias; // 0 unless the caller passed the larger gap model first: ksw_score_bias_kernel
	int32_t *d_diag = nullptr;
	if (diag_shortcut && P.n_kind[GD_KIND_WAVE16]) {
		if ((rc = gd_grow(ctx, ctx->diag, sizeof(int32_t) * (size_t)n))) return rc;
		d_diag = (int32_t *)ctx->diag.p;
	}
	hipLaunchKernelGGL(ksw_exact_match_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_tasks, n, d_qseq, d_tseq,
	                   d_status, d_score, d_n_cigar, d_cigar, d_diag, (int)K.sc_mch, (int)K.sc_mis, d_diag && K.sc_mis <= K.sc_mch && K.q + K.e > 0 ? (int)(K.sc_mch + 2 * (K.q + K.e)) + 1 : 0, score_bias);
	// The 64-lane, two-wavefront and two-blocks-per-lane kernels walk their own alignments back (status TRACED: the backtrack below skips them).
	const int n64 = (int)P.n_kind[GD_KIND_WAVE64];
	const bool single = ctx->single_affine && K.q == K.q2 && K.e == K.e2;
	ctx->narrow_launched = false;
	ctx->last_was_async = false; // this context's own launch is now its most recent one (a lane's flag is never set; gdiet_hip_map_wait sets the root's after the lane's batch)
	ctx->drain_enqueued = 0;
	if (n64 > 0) {
		// (ksw_wave_core.h: the ladder's six, the compact arena's, one claim counter per launch; behind them the pending list, a word per id)
		const size_t n_cnt = (size_t)GD_CNT_CLAIM + 1 + (size_t)P.n_drain, n_list = P.n_drain > 0 ? (size_t)n64 : 0;
		if ((rc = gd_grow(ctx, ctx->narrow_cnt, (n_cnt + n_list) * sizeof(uint32_t)))) return rc;
		uint32_t *d_cnt = (uint32_t *)ctx->narrow_cnt.p;
		GD_HIP(hipMemsetAsync(d_cnt, 0, n_cnt * sizeof(uint32_t), stream));
		ctx->narrow_launched = true;
		const int dp_waves = ctx->parent ? ctx->parent->dp_waves : ctx->dp_waves;
		gd_launch_wave64(d_tasks, d_ids + P.id_off[GD_KIND_WAVE64], n64, d_qseq, d_tseq, d_bt, d_status, d_score, K, stream, single, d_n_cigar, d_cigar,
		                 dp_waves, (ctx->parent ? ctx->parent->narrow_band : ctx->narrow_band) ? GD_W_NARROW : 0,
		                 d_cnt, ctx->quarter_offered ? GD_W_QUARTER : 0, 0, P.n_drain == 0, (int64_t)P.pool_off, P.n_compact ? (int64_t)P.pool_bytes : -1, n_list ? (int)n_cnt : 0);
		// The compact arena: boxes that found no room in the overflow pool are still pending, their ids in the pending list.  Drain launches
		// take them up behind the main launch and BEFORE the kernels of the other kinds, whose slots they may overwrite: the main launch's
		// rows are dead (its walks are done), those kernels write theirs afterwards.
		// A drain launch is the 96-register kernel: every wavefront of it needs a DP wavefront slot, and with two batches in flight the other
		// batch's main launch holds them all for 10 ms and more (profiles/r13_batch_tail.md).  So where the caller waits for this stream
		// anyway (host_decides) the host waits HERE, reads the list's length, and enqueues drain launches only if it is not zero -- it
		// almost always is zero -- and then over the pending boxes alone.  Elsewhere (a caller's stream that is never waited for; the shared
		// arena, where the next lane's kernels are already queued behind this stage) they are enqueued up front, a wavefront per id.
		int n_rounds = P.n_drain, n_slots = n64;
		if (P.n_drain > 0 && host_decides) {
			if (!ctx->h_pending.p) {
				ctx->h_pending.kind = DevBuf::PINNED;
				if (hipHostMalloc(&ctx->h_pending.p, 64, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); ctx->h_pending.p = nullptr; ctx->err = "hipHostMalloc of the pending count failed"; return GDIET_E_NOMEM; }
				ctx->h_pending.cap = 64;
			}
			GD_HIP(hipMemcpyAsync(ctx->h_pending.p, d_cnt + GD_CNT_PENDING, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
			GD_HIP(gd_stream_wait(ctx, stream));
			const uint32_t n_pending = *(volatile uint32_t *)ctx->h_pending.p;
			n_slots = (int)std::min<uint32_t>(n_pending, (uint32_t)n64);
			n_rounds = gd_drain_rounds(GdDrainSet{(size_t)n_slots, P.full_total, P.full_max}, P.bt);
		}
		for (int k = 1; k <= n_rounds; ++k)
			gd_launch_wave64(d_tasks, (const int32_t *)(d_cnt + n_cnt), n_slots, d_qseq, d_tseq, d_bt, d_status, d_score, K, stream, single, d_n_cigar, d_cigar,
			                 dp_waves, 0, d_cnt, 0, k, k == n_rounds, 0, (int64_t)P.bt, (int)n_cnt);
		ctx->drain_enqueued = n_rounds;
	}
	if (P.n_kind[GD_KIND_WAVE16]) {
		// The short-alignment kernels CAN walk their own alignments back (every group's first lane, gd_bt_thread_walk), but it does not pay:
		// a wavefront then holds its slot for a few hundred dependent steps of six lanes -- DP kernel 7.6 -> 10.8 ms per 262 144 short reads
		// against 1.65 ms of the separate backtrack kernel it saves (17.9 -> 15.1 M reads/s whole path; K3 alone 35.5 -> 26.6 M pairs/s).
		// GDIET_FUSE_BT_GROUPS=1 switches it on (same results: the GPU suite passes either way).
		static const bool fuse_groups = getenv("GDIET_FUSE_BT_GROUPS") && atoi(getenv("GDIET_FUSE_BT_GROUPS")) != 0;
		int32_t *g_nc = fuse_groups ? d_n_cigar : nullptr;
		uint32_t *g_cg = fuse_groups ? d_cigar : nullptr;
		gd_launch_wave_groups<16>(d_tasks, d_ids + P.group_off[0], (int)(P.n_group[0] / 4), d_qseq, d_tseq, d_bt, d_status, d_score, K, stream, single, g_nc, g_cg);
		gd_launch_wave_groups<10>(d_tasks, d_ids + P.group_off[1], (int)(P.n_group[1] / 6), d_qseq, d_tseq, d_bt, d_status, d_score, K, stream, single, g_nc, g_cg);
		gd_launch_wave_groups<8>(d_tasks, d_ids + P.group_off[2], (int)(P.n_group[2] / 8), d_qseq, d_tseq, d_bt, d_status, d_score, K, stream, single, g_nc, g_cg);
		int max_run = 0;
		for (const PipeRun &R : P.pipe_runs) max_run = std::max(max_run, (int)R.m);
		gd_launch_pipe(d_tasks, d_ids, (PipeRun *)ctx->pipe_runs.p, (int)P.pipe_runs.size(), max_run, (int32_t *)ctx->pipe_dst.p, (PipeWave *)ctx->pipes.p,
		               (int)P.pipes.size(), d_qseq, d_tseq, d_bt, d_status, d_score, K, stream, single);
	}
	if (P.n_kind[GD_KIND_WAVE128]) {
		// few wide-band alignments (the arena bounds how many 50 kbp ONT alignments fit): two wavefronts share one, halving the
		// serial chain; plenty of them: one wavefront each, two blocks per lane, no barrier
		const int n128 = (int)P.n_kind[GD_KIND_WAVE128];
		const int32_t *d_ids128 = d_ids + P.id_off[GD_KIND_WAVE128];
		const bool two = !P.wide_ck && (ctx->wide_two_waves == 1 || (ctx->wide_two_waves < 0 && n128 < ctx->wave_slots / 2));
		if (P.wide_ck) {
			if (P.n_ring96) gd_launch_wave96c(d_tasks, d_ids128, (int)P.n_ring96, d_qseq, d_tseq, d_bt, d_status, d_score, K, stream, d_n_cigar, d_cigar);
			if ((size_t)n128 > P.n_ring96)
				gd_launch_wave128(d_tasks, d_ids128 + P.n_ring96, n128 - (int)P.n_ring96, d_qseq, d_tseq, d_bt, d_status, d_score, K, stream, d_n_cigar, d_cigar, true);
		} else if (two)
			gd_launch_wave2x64(d_tasks, d_ids128, n128, d_qseq, d_tseq, d_bt, d_status, d_score, K, stream, d_n_cigar, d_cigar);
		else
			gd_launch_wave128(d_tasks, d_ids128, n128, d_qseq, d_tseq, d_bt, d_status, d_score, K, stream, d_n_cigar, d_cigar);
	}
	if (P.n_kind[GD_KIND_GENERIC]) {
		const size_t lds = (size_t)P.max_cap * 7;
		if (lds > 64 * 1024)
			GD_HIP(hipFuncSetAttribute((const void *)ksw_extd2_generic_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
		hipLaunchKernelGGL(ksw_extd2_generic_kernel, dim3((unsigned)P.n_kind[GD_KIND_GENERIC]), dim3(64), lds, stream,
		                   d_tasks, d_ids + P.id_off[GD_KIND_GENERIC], d_qseq, d_tseq, d_bt, d_status, d_score, K, P.max_cap);
	}
	GD_HIP(hipEventRecord(ctx->ev[1], stream));
	// the walks the DP kernels left, over the lists of the four kinds (back to back in d_ids)
	const int n_ids = (int)P.ids.size();
	if (n_ids > 0) {
		if (P.cells / (uint64_t)n > 200000) // long walks: one wavefront each; short reads: one walk per thread
			hipLaunchKernelGGL(ksw_backtrack_wave_kernel, dim3((n_ids + 3) / 4), dim3(256), 0, stream, d_tasks, n_ids, d_bt, d_status, d_score, d_n_cigar, d_cigar, d_ids);
		else
			hipLaunchKernelGGL(ksw_backtrack_kernel, dim3((n_ids + 63) / 64), dim3(64), 0, stream, d_tasks, n_ids, d_bt, d_status, d_score, d_n_cigar, d_cigar, d_ids,
			                   (const int32_t *)nullptr, (const int32_t *)d_diag);
	}
	if (score_bias) hipLaunchKernelGGL(ksw_score_bias_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, n, d_tasks, d_status, d_score, score_bias);
	GD_HIP(hipEventRecord(ctx->ev[2], stream));
	GD_HIP(hipGetLastError());
	return GDIET_OK;
}

// The work of gdiet_hip_ksw_extd2_batch_dev.  h_cigar_off / h_exact_score: host copies of the two small device arrays the
// planner needs; a caller that has them (the mapping pipeline) passes them and the call then never waits for the stream --
// which is what lets it be enqueued behind another batch's DP stage.
static int gd_ksw_batch_dev(gdiet_ctx *ctx, int n, const uint8_t *d_qseq, const uint8_t *d_tseq, const int32_t *d_exact_score,
                            const gdiet_ksw_score_t *sc, int32_t *d_score, int32_t *d_n_cigar, uint32_t *d_cigar, const int64_t *d_cigar_off,
                            const int64_t *h_qoff, const int64_t *h_toff, const int32_t *h_w, void *stream_, const int64_t *h_cigar_off,
                            const int32_t *h_exact_score, hipEvent_t arena_free = nullptr /* the kernels (not the descriptor copies) wait for it */,
                            std::unique_lock<std::mutex> *arena_turn = nullptr /* locked here once the planning is done, left locked */,
                            bool may_wait = false /* the caller waits for the stream behind this call anyway: the call may wait for the main DP launch (gd_dp_launch, host_decides) */)
{
	if (!ctx) return GDIET_E_PARAM;
	if (n <= 0) return GDIET_OK;
	if (!d_qseq || !d_tseq || !d_score || !d_n_cigar || !d_cigar || !h_qoff || !h_toff || !h_w) {
		ctx->err = "NULL argument";
		return GDIET_E_PARAM;
	}
	(void)hipSetDevice(ctx->device);
	hipStream_t stream = stream_ ? (hipStream_t)stream_ : ctx->stream;
	KswConst K;
	int rc = gd_consts(ctx, sc, K);
	if (rc) return rc;
	// d_cigar_off / d_exact_score are small: planning needs them on the host
	std::vector<int64_t> h_cig_own;
	std::vector<int32_t> h_ex_own;
	if (!h_cigar_off || (d_exact_score && !h_exact_score)) {
		h_cig_own.resize(n + 1);
		GD_HIP(hipMemcpyAsync(h_cig_own.data(), d_cigar_off, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, stream));
		if (d_exact_score) {
			h_ex_own.resize(n);
			GD_HIP(hipMemcpyAsync(h_ex_own.data(), d_exact_score, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream));
		}
		GD_HIP(hipStreamSynchronize(stream));
		h_cigar_off = h_cig_own.data(), h_exact_score = d_exact_score ? h_ex_own.data() : nullptr;
	}

	GdStageTrace mark; // where the planner's time goes
	if ((rc = gd_host_grow(ctx, ctx->h_tasks, sizeof(KswTask) * (size_t)n))) return rc;
	KswTask *h_tasks = (KswTask *)ctx->h_tasks.p;
	GdPlanOpt O;
	O.kernel_mode = ctx->kernel_mode, O.wave_scoring_ok = gd_wave_scoring_ok(K), O.single_affine = ctx->single_affine && K.q == K.q2 && K.e == K.e2;
	O.wide_ckpt = ctx->wide_ckpt, O.wave_slots = ctx->wave_slots, O.lane = ctx->parent != nullptr, O.group_lanes = gd_group_lanes, O.use_pipe = gd_use_pipe;
	// the compact arena, where the launch offers the narrow band (gd_dp_launch passes the same switch to the kernel; the CIGAR buffers are always given here)
	O.compact = gd_bt_compact && (ctx->parent ? ctx->parent->narrow_band : ctx->narrow_band), O.overflow_bytes = gd_bt_overflow_bytes;
	GdPlan &P = ctx->plan;
	gd_plan_batch(P, O, n, h_qoff, h_toff, h_w, h_cigar_off, d_exact_score ? h_exact_score : nullptr, h_tasks,
	              [&](int n_sl, auto f) { gd_parallel_for(ctx, ctx->lane_threads, n_sl, f); }, mark);
	ctx->last_mask = P.mask;
	if (!P.err && P.n_drain < 0) { ctx->err = "DP planner: the arena is smaller than the largest full-band slot"; return GDIET_E_PARAM; }
	if (!P.err) ctx->last_arena_bytes = P.bt;
	if (P.err == 1) { ctx->err = "empty sequence in batch (the reference returns without aligning)"; return GDIET_E_PARAM; }
	if (P.err == 2) { ctx->err = "alignment does not fit the wave kernel"; return GDIET_E_PARAM; }
	if (P.err == 4) { ctx->err = "band wider than the LDS window of the generic kernel"; return GDIET_E_PARAM; }
	ctx->last_cells = P.cells, ctx->last_alg_bytes = P.alg_bytes;
	const size_t bt = P.bt;
	// An async lane works in its parent's arena, taking turns behind parent->arena_ev -- unless the batch's backtrace is small
	// enough for every lane in flight to hold one of its own (long-read batches of few reads: their DP kernels then overlap, which
	// fills the GPU while one batch's longest alignments are still running).
	// (sticky: a lane that had to fall back to the shared arena stays there until its batches are clearly below the cap again --
	// giving a 50 GB arena back and allocating it anew every other batch costs more than taking turns)
	if (ctx->parent && bt > ctx->parent->lane_arena_cap) ctx->shared_sticky = true;
	else if (ctx->parent && bt <= ctx->parent->lane_arena_cap / 4 * 3) ctx->shared_sticky = false;
	bool own = ctx->parent && bt <= ctx->parent->lane_arena_cap && !ctx->shared_sticky;
	if (own && bt > ctx->arena.cap) { // grown in big steps: freeing device memory stalls every lane
		const size_t want = std::min(ctx->parent->lane_arena_cap, std::max<size_t>(bt + (bt >> 2), (size_t)1 << 30));
		if (gd_grow(ctx, ctx->arena, std::max(bt, want - (want >> 3) - 4096)) && gd_grow(ctx, ctx->arena, bt)) own = false, ctx->err.clear(); // no room: take turns in the shared one
	}
	if (ctx->parent && !own && ctx->arena.p) (void)ctx->arena.release();
	ctx->own_arena = own;
	if (own) arena_free = nullptr, arena_turn = nullptr;
	DevBuf &arena = ctx->parent && !own ? ctx->parent->arena : ctx->arena;
	{ // does this launch offer the quarter rung?  (the root's switch and auto state; dp_mu is not yet held by this thread)
		gdiet_ctx *root = ctx->parent ? ctx->parent : ctx;
		ctx->quarter_offered = root->narrow_band && root->narrow_quarter != 0;
		if (ctx->quarter_offered && root->narrow_quarter < 0 && P.n_kind[GD_KIND_WAVE64]) {
			std::lock_guard<std::mutex> guard(root->dp_mu);
			ctx->quarter_offered = gd_quarter_auto_offer(root->quarter_auto);
		}
	}
	if (arena_turn) arena_turn->lock(); // everything above was this batch's own planning: only the use of the arena is ordered
	if (ctx->parent && !own && bt > arena.cap) GD_HIP(hipEventSynchronize(ctx->parent->arena_ev)); // growing it: the previous user must be done
	if ((rc = gd_grow(ctx, arena, bt))) {
		// a context working synchronously after batches were in flight: its idle lanes may still hold private arenas
		// (a lane that takes its turn in the shared arena reclaims the private arenas of its idle siblings the same way)
		bool freed = false;
		if (rc == GDIET_E_NOMEM) {
			gdiet_ctx *owner = ctx->parent ? ctx->parent : ctx;
			std::lock_guard<std::mutex> guard(owner->async_mu); // async_busy[] belongs to submit / wait
			for (int i = 0; i < GD_MAX_INFLIGHT; ++i) {
				gdiet_ctx *c = owner->async_lane[i];
				if (c && c != ctx && !owner->async_busy[i] && c->arena.p) (void)c->arena.release(), freed = true;
			}
		}
		if (!freed || (rc = gd_grow(ctx, arena, bt))) return rc;
		ctx->err.clear();
	}
	mark("arena");
	if ((rc = gd_grow(ctx, ctx->tasks, sizeof(KswTask) * n))) return rc;
	if ((rc = gd_grow(ctx, ctx->ids, sizeof(int32_t) * P.ids.size()))) return rc;
	if ((rc = gd_grow(ctx, ctx->status, sizeof(int32_t) * n))) return rc;
	GD_HIP(hipMemcpyAsync(ctx->tasks.p, h_tasks, sizeof(KswTask) * n, hipMemcpyHostToDevice, stream));
	GD_HIP(hipMemcpyAsync(ctx->ids.p, P.ids.data(), sizeof(int32_t) * P.ids.size(), hipMemcpyHostToDevice, stream));
	if (!P.pipes.empty()) {
		if ((rc = gd_grow(ctx, ctx->pipes, sizeof(PipeWave) * P.pipes.size()))) return rc;
		if ((rc = gd_grow(ctx, ctx->pipe_runs, sizeof(PipeRun) * P.pipe_runs.size()))) return rc;
		if ((rc = gd_grow(ctx, ctx->pipe_dst, sizeof(int32_t) * P.n_pipe_ids))) return rc;
		GD_HIP(hipMemcpyAsync(ctx->pipes.p, P.pipes.data(), sizeof(PipeWave) * P.pipes.size(), hipMemcpyHostToDevice, stream));
		GD_HIP(hipMemcpyAsync(ctx->pipe_runs.p, P.pipe_runs.data(), sizeof(PipeRun) * P.pipe_runs.size(), hipMemcpyHostToDevice, stream));
	}
	mark("upload");
	if ((rc = gd_dp_launch(ctx, P, n, K, sc, d_qseq, d_tseq, (uint8_t *)arena.p, d_score, d_n_cigar, d_cigar, stream, arena_free,
	                       may_wait && !(ctx->parent && !own) /* (in the shared arena the lanes take turns: the next lane's kernels queue behind this stage as it was enqueued) */))) return rc;
	mark("launch");
	if (mark.on) fprintf(stderr, "[gdiet dp planner, ms] n=%d%s\n", n, mark.s.c_str());
	return GDIET_OK;
}

extern "C" int gdiet_hip_ksw_extd2_batch_dev(gdiet_ctx *ctx, int n, const uint8_t *d_qseq, const int64_t *d_qoff,
                                             const uint8_t *d_tseq, const int64_t *d_toff, const int32_t *d_w,
                                             const int32_t *d_exact_score, const gdiet_ksw_score_t *sc,
                                             int32_t *d_score, int32_t *d_n_cigar, uint32_t *d_cigar,
                                             const int64_t *d_cigar_off, const int64_t *h_qoff, const int64_t *h_toff,
                                             const int32_t *h_w, void *stream_)
{
	(void)d_qoff, (void)d_toff, (void)d_w;
	return gd_ksw_batch_dev(ctx, n, d_qseq, d_tseq, d_exact_score, sc, d_score, d_n_cigar, d_cigar, d_cigar_off, h_qoff, h_toff, h_w, stream_, nullptr, nullptr);
}

extern "C" int gdiet_hip_last_dp_work(const gdiet_ctx *ctx, uint64_t *cells, uint64_t *alg_bytes)
{
	if (!ctx) return GDIET_E_PARAM;
	if (cells) *cells = ctx->last_cells;
	if (alg_bytes) *alg_bytes = ctx->last_alg_bytes;
	return GDIET_OK;
}

// v[0..6): the ladder's counters; v[GD_CNT_POOL], v[GD_CNT_DRAINED], v[GD_CNT_LEFT]: the compact arena's (ksw_wave.hip.h)
static int gd_narrow_counters(gdiet_ctx *ctx, uint64_t v[10])
{
	for (int i = 0; i < 10; ++i) v[i] = 0;
	if (ctx->last_was_async) {
		for (int i = 0; i < 10; ++i) v[i] = ctx->async_narrow[i];
	} else if (ctx->narrow_launched && ctx->narrow_cnt.p) {
		uint32_t h[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
		(void)hipSetDevice(ctx->device);
		GD_HIP(hipMemcpy(h, ctx->narrow_cnt.p, sizeof(h), hipMemcpyDeviceToHost));
		for (int i = 0; i < 10; ++i) v[i] = h[i];
	}
	return GDIET_OK;
}
// after a batch has completed: a box the last drain launch could not serve has no alignment (gd_drain_launches rules it out)
static int gd_check_drained(gdiet_ctx *ctx, const uint64_t v[10])
{
	if (v[GD_CNT_LEFT] == 0) return GDIET_OK;
	ctx->err = "DP planner bug: " + std::to_string(v[GD_CNT_LEFT]) + " alignments found no full-band rows after the last drain launch";
	return GDIET_E_HIP;
}

// the narrow-band counters of the most recent DP launch (call after the batch has completed)
extern "C" int gdiet_hip_last_narrow_band(gdiet_ctx *ctx, uint64_t *tried, uint64_t *certified)
{
	if (!ctx) return GDIET_E_PARAM;
	uint64_t v[10];
	int rc;
	if ((rc = gd_narrow_counters(ctx, v))) return rc;
	if (tried) *tried = v[0];
	if (certified) *certified = v[1];
	return GDIET_OK;
}

// the same per rung of the ladder: out[0] / [1] alignments that evaluated the certificate at band 239 (quarter-block rows) / for which it
// held, out[2] / [3] the same at band 495 (half-block rows)
extern "C" int gdiet_hip_last_narrow_rungs(gdiet_ctx *ctx, uint64_t out[4])
{
	if (!ctx || !out) return GDIET_E_PARAM;
	uint64_t v[10];
	int rc;
	if ((rc = gd_narrow_counters(ctx, v))) return rc;
	for (int i = 0; i < 4; ++i) out[i] = v[2 + i];
	return GDIET_OK;
}

// the compact arena of the most recent DP launch (call after the batch has completed): out[0] boxes that claimed full-band rows from the
// overflow pool, out[1] boxes served by a drain launch, out[2] bytes of backtrace arena the batch was planned with
extern "C" int gdiet_hip_last_arena(gdiet_ctx *ctx, uint64_t out[3])
{
	if (!ctx || !out) return GDIET_E_PARAM;
	uint64_t v[10];
	int rc;
	if ((rc = gd_narrow_counters(ctx, v))) return rc;
	out[0] = v[GD_CNT_POOL], out[1] = v[GD_CNT_DRAINED], out[2] = ctx->last_arena_bytes;
	return gd_check_drained(ctx, v);
}

// drain launches the most recent DP launch enqueued: 0 where the host saw an empty pending list (or the batch has no compact arena), the
// planner's worst case where they are enqueued before the main launch has ended (gd_dp_launch)
extern "C" int gdiet_hip_last_drain_launches(gdiet_ctx *ctx, int *enqueued)
{
	if (!ctx || !enqueued) return GDIET_E_PARAM;
	*enqueued = ctx->drain_enqueued;
	return GDIET_OK;
}

extern "C" int gdiet_hip_last_kernel_ms(gdiet_ctx *ctx, float *dp_ms, float *bt_ms)
{
	if (!ctx) return GDIET_E_PARAM;
	if (ctx->last_was_async) {
		if (dp_ms) *dp_ms = ctx->async_dp_ms;
		if (bt_ms) *bt_ms = ctx->async_bt_ms;
		return GDIET_OK;
	}
	float a = 0, b = 0;
	GD_HIP(hipEventElapsedTime(&a, ctx->ev[0], ctx->ev[1]));
	GD_HIP(hipEventElapsedTime(&b, ctx->ev[0], ctx->ev[2]));
	b -= a; // what remains after the last DP wavefront
	if (dp_ms) *dp_ms = a;
	if (bt_ms) *bt_ms = b;
	return GDIET_OK;
}

// ---- host-pointer entry point ------------------------------------------------------------------------------

// The synchronous kernel-level entry points grow and write the context's arena / sequence buffers on ctx->stream; the batches in flight
// of gdiet_hip_map_submit share that arena (dp_mu / arena_ev), so such a call while tickets are open could free the arena under a
// lane's running DP kernel.  Refused, as gdiet_hip_map_uploaded refuses it.
static bool gd_tickets_open(gdiet_ctx *ctx)
{
	std::lock_guard<std::mutex> guard(ctx->async_mu);
	for (int i = 0; i < GD_MAX_INFLIGHT; ++i)
		if (ctx->async_busy[i]) { ctx->err = "batches submitted with gdiet_hip_map_submit are still in flight: wait for their tickets first"; return true; }
	return false;
}

// after the results of a kernel-level batch are back on the host: does every CIGAR fit its slot?
static int gd_check_cigar_caps(gdiet_ctx *ctx, int n, const int32_t *n_cigar, const int64_t *cigar_off)
{
	for (int i = 0; i < n; ++i)
		if (n_cigar[i] > cigar_off[i + 1] - cigar_off[i]) {
			ctx->err = "CIGAR of alignment " + std::to_string(i) + " needs " + std::to_string(n_cigar[i]) + " ops";
			return GDIET_E_CIGAR_CAP;
		}
	return GDIET_OK;
}

// The descriptors of a batch whose alignments all go to one LDS-resident kernel (ksw_extz2_exact.hip.h, ksw_exts2.hip.h), in ctx->h_tasks:
// band w[i] (w == nullptr: -1, no band), rows of the reference's n_col_ blocks, the backtrace matrices back to back (with_bt == false:
// none, every bt_off 0).  bt: bytes of arena; max_cap: the largest gd_generic_cap.
static int gd_literal_tasks(gdiet_ctx *ctx, int n, const int64_t *qoff, const int64_t *toff, const int32_t *w, const int64_t *cigar_off, bool with_bt,
                            size_t &bt, int &max_cap)
{
	const int rc = gd_host_grow(ctx, ctx->h_tasks, sizeof(KswTask) * (size_t)n);
	if (rc) return rc;
	KswTask *h_tasks = (KswTask *)ctx->h_tasks.p;
	bt = 0, max_cap = 0;
	for (int i = 0; i < n; ++i) {
		KswTask &T = h_tasks[i];
		T.qoff = qoff[i], T.toff = toff[i], T.qlen = (int)(qoff[i + 1] - qoff[i]), T.tlen = (int)(toff[i + 1] - toff[i]), T.w = w ? w[i] : -1;
		if (T.qlen <= 0 || T.tlen <= 0) { ctx->err = "empty sequence in batch (the reference returns without aligning)"; return GDIET_E_PARAM; }
		T.cig_off = cigar_off[i], T.cig_cap = (int32_t)std::min<int64_t>(cigar_off[i + 1] - cigar_off[i], 0x7fffffff);
		T.exact_score = GD_NEG_INF, T.kind = GD_KIND_GENERIC, T.pad = 0;
		T.row_bytes = gd_ncol16(T.qlen, T.tlen, T.w) * 16; // (w < 0: (min(qlen, tlen) + 15) / 16 + 1 blocks, n_col_ of ksw_exts2, :80)
		T.bt_off = (int64_t)bt;
		if (with_bt) bt += gd_align256((size_t)(T.qlen + T.tlen - 1) * (size_t)T.row_bytes + 64);
		max_cap = std::max(max_cap, gd_generic_cap(T.qlen, T.tlen, T.w));
	}
	return GDIET_OK;
}

extern "C" int gdiet_hip_ksw_extd2_batch(gdiet_ctx *ctx, int n, const uint8_t *qseq, const int64_t *qoff,
                                         const uint8_t *tseq, const int64_t *toff, const int32_t *w,
                                         const int32_t *exact_score, const gdiet_ksw_score_t *sc, int32_t *score,
                                         int32_t *n_cigar, uint32_t *cigar, const int64_t *cigar_off)
{
	if (!ctx) return GDIET_E_PARAM;
	if (n <= 0) return GDIET_OK;
	if (!qseq || !qoff || !tseq || !toff || !w || !score || !n_cigar || !cigar || !cigar_off) {
		ctx->err = "NULL argument";
		return GDIET_E_PARAM;
	}
	if (gd_tickets_open(ctx)) return GDIET_E_PARAM;
	(void)hipSetDevice(ctx->device);
	int rc;
	hipStream_t s = ctx->stream;
	const size_t qb = (size_t)qoff[n], tb = (size_t)toff[n], cb = (size_t)cigar_off[n];
	// layout of the small per-batch arrays behind the sequences: [cigar_off (n+1) i64][exact (n) i32]
	const size_t aux = sizeof(int64_t) * (n + 1) + sizeof(int32_t) * n;
	if ((rc = gd_grow(ctx, ctx->qseq, qb + 64))) return rc;
	if ((rc = gd_grow(ctx, ctx->tseq, tb + 64 + aux + 16))) return rc;
	if ((rc = gd_grow(ctx, ctx->score, sizeof(int32_t) * n))) return rc;
	if ((rc = gd_grow(ctx, ctx->ncig, sizeof(int32_t) * n))) return rc;
	if ((rc = gd_grow(ctx, ctx->cigar, sizeof(uint32_t) * (cb + 1)))) return rc;
	uint8_t *d_q = (uint8_t *)ctx->qseq.p, *d_t = (uint8_t *)ctx->tseq.p;
	int64_t *d_cigoff = (int64_t *)(d_t + ((tb + 64 + 15) & ~(size_t)15));
	int32_t *d_ex = (int32_t *)(d_cigoff + n + 1);
	GD_HIP(hipMemcpyAsync(d_q, qseq, qb, hipMemcpyHostToDevice, s));
	GD_HIP(hipMemcpyAsync(d_t, tseq, tb, hipMemcpyHostToDevice, s));
	GD_HIP(hipMemcpyAsync(d_cigoff, cigar_off, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, s));
	if (exact_score) GD_HIP(hipMemcpyAsync(d_ex, exact_score, sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
	rc = gd_ksw_batch_dev(ctx, n, d_q, d_t, exact_score ? d_ex : nullptr, sc, (int32_t *)ctx->score.p, (int32_t *)ctx->ncig.p, (uint32_t *)ctx->cigar.p, d_cigoff,
	                      qoff, toff, w, s, nullptr, nullptr, nullptr, nullptr, true /* this call waits for s below */);
	if (rc) return rc;
	GD_HIP(hipMemcpyAsync(score, ctx->score.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
	GD_HIP(hipMemcpyAsync(n_cigar, ctx->ncig.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
	GD_HIP(hipMemcpyAsync(cigar, ctx->cigar.p, sizeof(uint32_t) * cb, hipMemcpyDeviceToHost, s));
	GD_HIP(hipStreamSynchronize(s));
	if (ctx->plan.n_drain > 0) { // (a batch with a compact arena: one more small copy)
		uint64_t v[10];
		if ((rc = gd_narrow_counters(ctx, v)) || (rc = gd_check_drained(ctx, v))) return rc;
	}
	return gd_check_cigar_caps(ctx, n, n_cigar, cigar_off);
}

// ---- K3: single-affine form ----------------------------------------------------------------------------------
static int gd_extz2_literal(gdiet_ctx *ctx, int n, const uint8_t *qseq, const int64_t *qoff, const uint8_t *tseq, const int64_t *toff,
                            const int32_t *w, const gdiet_ksw_score_t *sc, int32_t flag, int32_t zdrop, int32_t end_bonus,
                            gdiet_ksw_extz_t *ez, int32_t *n_cigar, uint32_t *cigar, const int64_t *cigar_off);

extern "C" int gdiet_hip_ksw_extz2_batch(gdiet_ctx *ctx, int n, const uint8_t *qseq, const int64_t *qoff, const uint8_t *tseq,
                                         const int64_t *toff, const int32_t *w, const gdiet_ksw_score_t *sc, int32_t *score,
                                         int32_t *n_cigar, uint32_t *cigar, const int64_t *cigar_off)
{
	if (!ctx) return GDIET_E_PARAM;
	if (n <= 0) return GDIET_OK;
	if (!sc) { ctx->err = "scoring is NULL"; return GDIET_E_PARAM; }
	gdiet_ksw_score_t s2 = *sc;
	s2.q2 = sc->q, s2.e2 = sc->e;
	KswConst K;
	int rc = gd_consts(ctx, &s2, K); // (the same parameter checks at every scoring, whichever form runs)
	if (rc) return rc;
	if (gd_wave_scoring_ok(K)) {
		// ksw_extz2(q,e) == ksw_extd2(q,e,q,e) cell for cell at every scoring the register-resident kernels take (see include/gdiet_hip.h)
		ctx->single_affine = true; // the 16- and 64-lane kernels then run their single-affine form (no X2 / Y2 half)
		rc = gdiet_hip_ksw_extd2_batch(ctx, n, qseq, qoff, tseq, toff, w, nullptr, &s2, score, n_cigar, cigar, cigar_off);
		ctx->single_affine = false;
		return rc;
	}
	// elsewhere the two can differ: ksw_extz2_sse's own recurrence, APPROX_MAX branch (ksw_extz2_exact.hip.h)
	if (!score) { ctx->err = "NULL argument"; return GDIET_E_PARAM; }
	std::vector<gdiet_ksw_extz_t> ez((size_t)n);
	if ((rc = gd_extz2_literal(ctx, n, qseq, qoff, tseq, toff, w, sc, GD_EZ_APPROX_MAX, -1, 0, ez.data(), n_cigar, cigar, cigar_off))) return rc;
	for (int i = 0; i < n; ++i) score[i] = ez[i].score;
	return GDIET_OK;
}

// exact-max mode of ksw_extz2 (flag without APPROX_MAX): ksw_extz2_exact.hip.h
extern "C" int gdiet_hip_ksw_extz2_batch_ex(gdiet_ctx *ctx, int n, const uint8_t *qseq, const int64_t *qoff, const uint8_t *tseq,
                                            const int64_t *toff, const int32_t *w, const gdiet_ksw_score_t *sc, int32_t zdrop, int32_t end_bonus,
                                            gdiet_ksw_extz_t *ez, int32_t *n_cigar, uint32_t *cigar, const int64_t *cigar_off)
{
	if (!ctx) return GDIET_E_PARAM;
	if (n <= 0) return GDIET_OK;
	if (sc && (sc->flag & ~GD_EZ_EXTZ_ONLY)) {
		ctx->err = "gdiet_hip_ksw_extz2_batch_ex takes flag 0 or KSW_EZ_EXTZ_ONLY (exact maximum); APPROX_MAX: gdiet_hip_ksw_extz2_batch";
		return GDIET_E_PARAM;
	}
	return gd_extz2_literal(ctx, n, qseq, qoff, tseq, toff, w, sc, sc ? sc->flag : 0, zdrop, end_bonus, ez, n_cigar, cigar, cigar_off);
}

// ksw_extz2_sse with ksw_backtrack, literally: flag 0 / KSW_EZ_EXTZ_ONLY (exact maximum) or KSW_EZ_APPROX_MAX (sc->flag is not read)
static int gd_extz2_literal(gdiet_ctx *ctx, int n, const uint8_t *qseq, const int64_t *qoff, const uint8_t *tseq, const int64_t *toff,
                            const int32_t *w, const gdiet_ksw_score_t *sc, int32_t flag, int32_t zdrop, int32_t end_bonus,
                            gdiet_ksw_extz_t *ez, int32_t *n_cigar, uint32_t *cigar, const int64_t *cigar_off)
{
	if (!qseq || !qoff || !tseq || !toff || !w || !sc || !ez || !n_cigar || !cigar || !cigar_off) { ctx->err = "NULL argument"; return GDIET_E_PARAM; }
	static_assert(sizeof(gdiet_ksw_extz_t) == sizeof(GdExtzOut), "public and kernel record differ");
	if (gd_tickets_open(ctx)) return GDIET_E_PARAM;
	(void)hipSetDevice(ctx->device);
	hipStream_t s = ctx->stream;
	KswzConst K;
	K.q = sc->q, K.e = sc->e, K.sc_mch = sc->match, K.sc_mis = sc->mismatch, K.sc_N = sc->sc_ambi == 0 ? -sc->e : sc->sc_ambi;
	K.zdrop = zdrop, K.end_bonus = end_bonus, K.flag = flag;
	{ // :88-90: the reference returns without aligning
		const int min_sc = std::min<int>(std::min<int>(sc->mismatch, sc->match), std::min<int>(sc->sc_ambi, 0));
		if (-min_sc > 2 * (K.q + K.e)) { ctx->err = "-min_sc > 2*(q+e): the reference returns without aligning"; return GDIET_E_PARAM; }
	}
	int rc, max_cap;
	size_t bt;
	if ((rc = gd_literal_tasks(ctx, n, qoff, toff, w, cigar_off, true, bt, max_cap))) return rc;
	const size_t lds = (size_t)max_cap * (flag & GD_EZ_APPROX_MAX ? 5 : 9); // u v x y s, and the int32 H ring of the exact maximum
	if (lds > 160 * 1024 - 1024) { ctx->err = "band wider than the LDS window of the literal ksw_extz2 kernel"; return GDIET_E_PARAM; }
	const size_t qb = (size_t)qoff[n], tb = (size_t)toff[n], cb = (size_t)cigar_off[n];
	if ((rc = gd_grow(ctx, ctx->arena, bt))) return rc;
	if ((rc = gd_grow(ctx, ctx->tasks, sizeof(KswTask) * n))) return rc;
	if ((rc = gd_grow(ctx, ctx->status, sizeof(int32_t) * n))) return rc;
	if ((rc = gd_grow(ctx, ctx->qseq, qb + 64))) return rc;
	if ((rc = gd_grow(ctx, ctx->tseq, tb + 64))) return rc;
	if ((rc = gd_grow(ctx, ctx->score, sizeof(int32_t) * 3 * (size_t)n + sizeof(GdExtzOut) * (size_t)n))) return rc; // score | start (2n) | ez
	if ((rc = gd_grow(ctx, ctx->ncig, sizeof(int32_t) * n))) return rc;
	if ((rc = gd_grow(ctx, ctx->cigar, sizeof(uint32_t) * (cb + 1)))) return rc;
	int32_t *d_score = (int32_t *)ctx->score.p, *d_start = d_score + n;
	GdExtzOut *d_ez = (GdExtzOut *)(d_start + 2 * (size_t)n);
	GD_HIP(hipMemcpyAsync(ctx->qseq.p, qseq, qb, hipMemcpyHostToDevice, s));
	GD_HIP(hipMemcpyAsync(ctx->tseq.p, tseq, tb, hipMemcpyHostToDevice, s));
	GD_HIP(hipMemcpyAsync(ctx->tasks.p, ctx->h_tasks.p, sizeof(KswTask) * n, hipMemcpyHostToDevice, s));
	if (lds > 64 * 1024) GD_HIP(hipFuncSetAttribute((const void *)ksw_extz2_exact_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	ctx->last_mask = 2, ctx->last_was_async = false;
	GD_HIP(hipEventRecord(ctx->ev[0], s));
	hipLaunchKernelGGL(ksw_extz2_exact_kernel, dim3(n), dim3(64), lds, s, (const KswTask *)ctx->tasks.p, n, (const uint8_t *)ctx->qseq.p, (const uint8_t *)ctx->tseq.p,
	                   (uint8_t *)ctx->arena.p, (int32_t *)ctx->status.p, d_score, d_ez, d_start, K, max_cap);
	GD_HIP(hipEventRecord(ctx->ev[1], s));
	hipLaunchKernelGGL(ksw_backtrack_kernel, dim3((n + 63) / 64), dim3(64), 0, s, (const KswTask *)ctx->tasks.p, n, (const uint8_t *)ctx->arena.p,
	                   (const int32_t *)ctx->status.p, d_score, (int32_t *)ctx->ncig.p, (uint32_t *)ctx->cigar.p, (const int32_t *)nullptr, (const int32_t *)d_start);
	GD_HIP(hipEventRecord(ctx->ev[2], s));
	GD_HIP(hipMemcpyAsync(ez, d_ez, sizeof(GdExtzOut) * n, hipMemcpyDeviceToHost, s));
	GD_HIP(hipMemcpyAsync(n_cigar, ctx->ncig.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
	GD_HIP(hipMemcpyAsync(cigar, ctx->cigar.p, sizeof(uint32_t) * cb, hipMemcpyDeviceToHost, s));
	GD_HIP(hipStreamSynchronize(s));
	GD_HIP(hipGetLastError());
	return gd_check_cigar_caps(ctx, n, n_cigar, cigar_off);
}

// ksw_exts2 (splice-aware extension; not called by GDiet): ksw_exts2.hip.h
extern "C" int gdiet_hip_ksw_exts2_batch(gdiet_ctx *ctx, int n, const uint8_t *qseq, const int64_t *qoff, const uint8_t *tseq, const int64_t *toff,
                                         const uint8_t *junc, const int8_t *mat, int8_t q, int8_t e, int8_t q2, int8_t noncan, int32_t zdrop,
                                         int8_t junc_bonus, int32_t flag, gdiet_ksw_extz_t *ez, int32_t *n_cigar, uint32_t *cigar, const int64_t *cigar_off)
{
	if (!ctx) return GDIET_E_PARAM;
	if (n <= 0) return GDIET_OK;
	if (!qseq || !qoff || !tseq || !toff || !mat || !ez || !n_cigar || !cigar || !cigar_off) { ctx->err = "NULL argument"; return GDIET_E_PARAM; }
	const int32_t known = GD_EZ_SCORE_ONLY | GD_EZ_RIGHT | GD_EZ_GENERIC_SC | GD_EZ_APPROX_MAX | GD_EZ_APPROX_DROP | GD_EZ_EXTZ_ONLY | GD_EZ_REV_CIGAR |
	                      GD_EZ_SPLICE_FOR | GD_EZ_SPLICE_REV | GD_EZ_SPLICE_FLANK;
	if (flag & ~known) { ctx->err = "gdiet_hip_ksw_exts2_batch: unknown flag bit"; return GDIET_E_PARAM; }
	if (q2 <= q + e || e <= 0) { ctx->err = "ksw_exts2 needs q2 > q + e (and e > 0): the reference returns without aligning"; return GDIET_E_PARAM; } // :72
	if (gd_tickets_open(ctx)) return GDIET_E_PARAM;
	(void)hipSetDevice(ctx->device);
	hipStream_t s = ctx->stream;
	KswsConst K;
	K.q = q, K.e = e, K.q2 = q2, K.noncan = noncan, K.zdrop = zdrop, K.junc_bonus = junc_bonus, K.flag = flag;
	K.sc_mch = mat[0], K.sc_mis = mat[1], K.sc_N = mat[24] == 0 ? -e : mat[24];
	memcpy(K.mat, mat, 25);
	{ // :86-90
		int min_sc = mat[1];
		for (int t = 1; t < 25; ++t) min_sc = std::min<int>(min_sc, mat[t]);
		if (-min_sc > 2 * (q + e)) { ctx->err = "-min_sc > 2*(q+e): the reference returns without aligning"; return GDIET_E_PARAM; }
	}
	K.long_thres = (q2 - q) / e - 1; // :92-95
	if (q2 > q + e + K.long_thres * e) ++K.long_thres;
	K.long_diff = K.long_thres * e - (q2 - q);
	int rc, max_cap;
	size_t bt;
	if ((rc = gd_literal_tasks(ctx, n, qoff, toff, nullptr, cigar_off, !(flag & GD_EZ_SCORE_ONLY), bt, max_cap))) return rc;
	const size_t lds = (size_t)max_cap * 10 + 16;
	if (lds > 160 * 1024 - 1024) { ctx->err = "alignment longer than the LDS window of the ksw_exts2 kernel (min(qlen, tlen) <= ~8000)"; return GDIET_E_PARAM; }
	const size_t qb = (size_t)qoff[n], tb = (size_t)toff[n], cb = (size_t)cigar_off[n];
	if ((rc = gd_grow(ctx, ctx->arena, bt + 256))) return rc;
	if ((rc = gd_grow(ctx, ctx->tasks, sizeof(KswTask) * n))) return rc;
	if ((rc = gd_grow(ctx, ctx->qseq, qb + 64))) return rc;
	if ((rc = gd_grow(ctx, ctx->tseq, 2 * tb + 128))) return rc; // target | junction annotation
	if ((rc = gd_grow(ctx, ctx->score, sizeof(GdExtzOut) * (size_t)n))) return rc;
	if ((rc = gd_grow(ctx, ctx->ncig, sizeof(int32_t) * n))) return rc;
	if ((rc = gd_grow(ctx, ctx->cigar, sizeof(uint32_t) * (cb + 1)))) return rc;
	uint8_t *d_junc = junc ? (uint8_t *)ctx->tseq.p + tb + 64 : nullptr;
	GD_HIP(hipMemcpyAsync(ctx->qseq.p, qseq, qb, hipMemcpyHostToDevice, s));
	GD_HIP(hipMemcpyAsync(ctx->tseq.p, tseq, tb, hipMemcpyHostToDevice, s));
	if (junc) GD_HIP(hipMemcpyAsync(d_junc, junc, tb, hipMemcpyHostToDevice, s));
	GD_HIP(hipMemcpyAsync(ctx->tasks.p, ctx->h_tasks.p, sizeof(KswTask) * n, hipMemcpyHostToDevice, s));
	if (lds > 64 * 1024) GD_HIP(hipFuncSetAttribute((const void *)ksw_exts2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	ctx->last_mask = 2, ctx->last_was_async = false;
	GD_HIP(hipEventRecord(ctx->ev[0], s));
	hipLaunchKernelGGL(ksw_exts2_kernel, dim3(n), dim3(64), lds, s, (const KswTask *)ctx->tasks.p, n, (const uint8_t *)ctx->qseq.p, (const uint8_t *)ctx->tseq.p,
	                   (const uint8_t *)d_junc, (uint8_t *)ctx->arena.p, (GdExtzOut *)ctx->score.p, (int32_t *)ctx->ncig.p, (uint32_t *)ctx->cigar.p, K, max_cap);
	GD_HIP(hipEventRecord(ctx->ev[1], s));
	GD_HIP(hipEventRecord(ctx->ev[2], s));
	GD_HIP(hipMemcpyAsync(ez, ctx->score.p, sizeof(GdExtzOut) * n, hipMemcpyDeviceToHost, s));
	GD_HIP(hipMemcpyAsync(n_cigar, ctx->ncig.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
	GD_HIP(hipMemcpyAsync(cigar, ctx->cigar.p, sizeof(uint32_t) * cb, hipMemcpyDeviceToHost, s));
	GD_HIP(hipStreamSynchronize(s));
	GD_HIP(hipGetLastError());
	return gd_check_cigar_caps(ctx, n, n_cigar, cigar_off);
}

#include "map_pipeline.hip.h"
#include "map_multi.h"

// ---- SURVEY 8f rank 4, chaining half: mg_lchain_dp for a batch of reads (lchain.hip.h on the device, lchain_host.h on host threads) ----
#include "lchain.hip.h"
#include "lchain_host.h"
extern "C" int gdiet_hip_lchain_dp_batch(gdiet_ctx *ctx, int n_reads, const uint64_t *a, const int64_t *aoff, int32_t max_dist_x, int32_t max_dist_y,
                                         int32_t bw, int32_t max_skip, int32_t max_iter, int32_t min_cnt, int32_t min_sc, float chn_pen_gap,
                                         float chn_pen_skip, int32_t is_cdna, int32_t n_seg, int32_t *n_u, int64_t *n_v, uint64_t *u, uint64_t *a_out)
{
	if (!ctx) return GDIET_E_PARAM;
	if (n_reads <= 0) return GDIET_OK;
	if (!a || !aoff || !n_u || !n_v || !u || !a_out) { ctx->err = "NULL argument"; return GDIET_E_PARAM; }
	const int64_t tot = aoff[n_reads];
	for (int i = 0; i < n_reads; ++i) {
		if (aoff[i + 1] < aoff[i] || aoff[i + 1] - aoff[i] > 0x7fffffff) { ctx->err = "anchor offsets must ascend (at most 2^31 - 1 anchors per read)"; return GDIET_E_PARAM; }
		n_u[i] = 0, n_v[i] = 0;
	}
	if (tot == 0) return GDIET_OK;
	if (gd_tickets_open(ctx)) return GDIET_E_PARAM;
	(void)hipSetDevice(ctx->device);
	hipStream_t s = ctx->stream;
	GdChainOpt O;
	O.max_dist_x = max_dist_x < bw ? bw : max_dist_x; // SR/lchain.c:136-137
	O.max_dist_y = (max_dist_y < bw && !is_cdna) ? bw : max_dist_y;
	O.bw = bw, O.max_skip = max_skip, O.max_iter = max_iter, O.min_cnt = min_cnt, O.min_sc = min_sc;
	O.chn_pen_gap = chn_pen_gap, O.chn_pen_skip = chn_pen_skip, O.is_cdna = is_cdna, O.n_seg = n_seg;
	int rc;
	// device: anchors | offsets | f | p | v | t   (qseq / tseq / score / status buffers of the context reused as plain workspace)
	if ((rc = gd_grow(ctx, ctx->qseq, sizeof(uint64_t) * 2 * (size_t)tot + 64))) return rc;
	if ((rc = gd_grow(ctx, ctx->tasks, sizeof(int64_t) * ((size_t)n_reads + 1) + 64))) return rc;
	if ((rc = gd_grow(ctx, ctx->score, sizeof(int32_t) * 4 * (size_t)tot + 64))) return rc;
	if ((rc = gd_host_grow(ctx, ctx->h_res, sizeof(int32_t) * 3 * (size_t)tot + 64))) return rc;
	int32_t *d_f = (int32_t *)ctx->score.p, *d_p = d_f + tot, *d_v = d_p + tot, *d_t = d_v + tot;
	int32_t *h_f = (int32_t *)ctx->h_res.p, *h_p = h_f + tot, *h_v = h_p + tot;
	GD_HIP(hipMemcpyAsync(ctx->qseq.p, a, sizeof(uint64_t) * 2 * (size_t)tot, hipMemcpyHostToDevice, s));
	GD_HIP(hipMemcpyAsync(ctx->tasks.p, aoff, sizeof(int64_t) * ((size_t)n_reads + 1), hipMemcpyHostToDevice, s));
	ctx->last_mask = 0, ctx->last_was_async = false;
	GD_HIP(hipEventRecord(ctx->ev[0], s));
	hipLaunchKernelGGL(lchain_fill_kernel, dim3(n_reads), dim3(64), 0, s, n_reads, (const uint64_t *)ctx->qseq.p, (const int64_t *)ctx->tasks.p, O, d_f, d_p, d_v, d_t);
	GD_HIP(hipEventRecord(ctx->ev[1], s));
	GD_HIP(hipEventRecord(ctx->ev[2], s));
	GD_HIP(hipMemcpyAsync(h_f, d_f, sizeof(int32_t) * 3 * (size_t)tot, hipMemcpyDeviceToHost, s));
	GD_HIP(hipStreamSynchronize(s));
	GD_HIP(hipGetLastError());
	gd_parallel_for(ctx, ctx->lane_threads, n_reads, [&](int i) {
		static thread_local std::vector<GdlPair> z, b;
		static thread_local std::vector<int32_t> t;
		static thread_local std::vector<uint64_t> u2;
		const int64_t o = aoff[i], n = aoff[i + 1] - o;
		if (n <= 0) return;
		n_u[i] = gdl_chains_of_read(n, (const GdlPair *)a + o, h_f + o, h_p + o, h_v + o, min_cnt, min_sc, u + o, (GdlPair *)a_out + o, &n_v[i], z, t, b, u2);
	});
	return GDIET_OK;
}

#ifdef GD_SEED_PROF
extern "C" int gdiet_hip_debug_seed_prof(unsigned long long *out8) { return (int)hipMemcpyFromSymbol(out8, HIP_SYMBOL(gd_seed_prof), 64); }
#endif
// ---- read input (input half) ---------------------------------------------------------------------------
#include "fastx_reader.h"
#include "fastx_dev_driver.hip.h" // struct gdiet_fastx; the device mode of the reader.  It includes bgzf_driver.hip.h: the BGZF drivers, gdiet_bgzf_out, gdiet_hip_bgzf_*
#include "bam_in_driver.hip.h"    // BAM input: the unpack kernel's driver, gdiet_hip_bam_in_unpack
#include "ref_fasta_driver.hip.h" // reference input: FASTA blocks parsed on the device, gdiet_hip_index_open / _index_info / _index_open_stats / _ref_block
static int gd_fx_read_failed(gdiet_fastx *fx);

extern "C" int gdiet_hip_fastx_open(gdiet_fastx **fx, const char *path)
{
	if (!fx) return GDIET_E_PARAM;
	*fx = nullptr;
	GdFastx *r = gd_fastx_open(path);
	if (!r) return GDIET_E_PARAM;
	*fx = new gdiet_fastx();
	(*fx)->r = r;
	return GDIET_OK;
}

extern "C" int gdiet_hip_fastx_read(gdiet_fastx *fx, int64_t chunk_size, int with_qual, int with_comment, int frag_mode, int32_t *n_reads,
                                    const char *const **names, const char *const **comments, const char *const **seqs,
                                    const char *const **quals, const int32_t **lens)
{
	if (!fx || !fx->r || !n_reads || !names || !seqs || !lens) return GDIET_E_PARAM;
	bool bad = false;
	const int n = fx->r->read_batch(chunk_size, with_qual != 0, with_comment != 0, frag_mode != 0, &bad);
	if (n < 0) return gd_fx_read_failed(fx);
	fx->r->u_to_t_on_host(); // (an attached reader without a resident batch: nobody encodes these reads on the device)
	gd_fx_release_done(*fx->r);
	*n_reads = n;
	*names = fx->r->v_name.data(), *seqs = fx->r->v_seq.data(), *lens = fx->r->v_len.data();
	if (comments) *comments = fx->r->v_comment.data();
	if (quals) *quals = fx->r->v_qual.data();
	return bad ? GDIET_W_TRUNCATED : GDIET_OK;
}

extern "C" int gdiet_hip_fastx_attach(gdiet_fastx *fx, gdiet_ctx *ctx)
{
	if (!fx || !fx->r) return GDIET_E_PARAM;
	fx->ctx = ctx;
	if (ctx) fx->r->dev = std::make_shared<GdFxExecutor>(ctx);
	else fx->r->dev.reset();
	return GDIET_OK;
}

extern "C" int gdiet_hip_fastx_read_resident(gdiet_fastx *fx, int64_t chunk_size, int with_qual, int with_comment, int frag_mode, int32_t *n_reads,
                                             const char *const **names, const char *const **comments, const char *const **seqs,
                                             const char *const **quals, const int32_t **lens, gdiet_read_batch **batch)
{
	if (!fx || !fx->r || !n_reads || !names || !seqs || !lens || !batch) return GDIET_E_PARAM;
	*batch = nullptr;
	if (!fx->ctx) return GDIET_E_PARAM; // the batch belongs to a context: attach first
	bool bad = false;
	const int n = fx->r->read_batch(chunk_size, with_qual != 0, with_comment != 0, frag_mode != 0, &bad);
	if (n < 0) return gd_fx_read_failed(fx);
	if (n > 0) {
		const int rc = gd_fx_build_batch(fx->ctx, *fx->r, batch);
		if (rc) return rc;
	}
	gd_fx_release_done(*fx->r);
	*n_reads = n;
	*names = fx->r->v_name.data(), *seqs = fx->r->v_seq.data(), *lens = fx->r->v_len.data();
	if (comments) *comments = fx->r->v_comment.data();
	if (quals) *quals = fx->r->v_qual.data();
	return bad ? GDIET_W_TRUNCATED : GDIET_OK;
}

extern "C" int gdiet_hip_fastx_stats(const gdiet_fastx *fx, int64_t *records_device, int64_t *records_host, int64_t *blocks, int64_t *blocks_handed_over)
{
	if (!fx || !fx->r) return GDIET_E_PARAM;
	if (records_device) *records_device = fx->r->n_rec_device;
	if (records_host) *records_host = fx->r->n_rec_host;
	if (blocks) *blocks = fx->r->n_blocks;
	if (blocks_handed_over) *blocks_handed_over = fx->r->n_blocks_handed;
	return GDIET_OK;
}

extern "C" int gdiet_hip_fastx_format(const gdiet_fastx *fx) { return fx && fx->r && fx->r->format == 1 ? 1 : 0; }

// a read error of the reader, kept where gdiet_hip_strerror finds it
static int gd_fx_read_failed(gdiet_fastx *fx)
{
	const int rc = fx->r->dev_error ? GDIET_E_HIP : GDIET_E_PARAM;
	if (fx->ctx && !fx->r->io_msg.empty()) return gd_err_fail(fx->ctx, rc, "read error: " + fx->r->io_msg);
	return rc;
}

extern "C" const char *gdiet_hip_fastx_strerror(const gdiet_fastx *fx) { return fx && fx->r ? fx->r->io_msg.c_str() : "no reader"; }

extern "C" int gdiet_hip_fastx_bgzf_stats(const gdiet_fastx *fx, int64_t *members_device, int64_t *members_host, int64_t *bytes_in, int64_t *bytes_out)
{
	if (!fx || !fx->r) return GDIET_E_PARAM;
	if (members_device) *members_device = fx->r->bz_members_device;
	if (members_host) *members_host = fx->r->bz_members_host;
	if (bytes_in) *bytes_in = fx->r->bz_bytes_in;
	if (bytes_out) *bytes_out = fx->r->bz_bytes_out;
	return GDIET_OK;
}

// measurement only (tools/map_file.py; not declared in include/gdiet_hip.h): seconds the reader's I/O thread spent on a BGZF file -- reading raw
// members; inflating (attached: the copies and the kernel; unattached: zlib and the checks together); checking lengths and CRCs (attached
// only) -- and, of the attached reader's context since it was created, the device's side of inflating: copy up, kernel, copy down (HIP events)
extern "C" int gdiet_hip_debug_bgzf_seconds(const gdiet_fastx *fx, double *out6)
{
	if (!fx || !fx->r || !out6) return GDIET_E_PARAM;
	for (int i = 0; i < 3; ++i) out6[i] = 1e-9 * (double)fx->r->bz_ns[i], out6[3 + i] = 0;
	if (fx->ctx) {
		std::lock_guard<std::mutex> lk(fx->ctx->bz.mu);
		for (int i = 0; i < 3; ++i) out6[3 + i] = 1e-3 * fx->ctx->bz.ms[i];
	}
	return GDIET_OK;
}

#include "bam_driver.hip.h" // BAM: the record encoder's driver, gdiet_hip_bam_header / _bam_batch_into / _bgzf_out_write_bam; brings accum_driver.hip.h, what the two accumulators share
#include "sam_driver.hip.h" // SAM text on the device: the line formatter's driver, gdiet_hip_sam_batch_device_into / _bgzf_out_write_sam
#include "cov_driver.hip.h" // coverage and depth accumulated from the resident records: gdiet_hip_cov_*
#include "pile_driver.hip.h" // base counts per position and variant sites from the resident records: gdiet_hip_pile_*
#include "stats_driver.hip.h" // read and alignment statistics from the resident records: gdiet_hip_stats_*
#include "bam_sort_driver.hip.h" // BAM records in coordinate order: the sort pass's driver, gdiet_hip_bam_sort_records

extern "C" int gdiet_hip_batch_export(gdiet_ctx *ctx, const gdiet_read_batch *b, int32_t *n, int64_t *roff, uint8_t *enc_host, uint8_t *enc_device)
{
	if (!ctx || !b) return GDIET_E_PARAM;
	if (n) *n = b->n;
	if (roff) memcpy(roff, b->roff.data(), sizeof(int64_t) * ((size_t)b->n + 1));
	const size_t total = (size_t)b->roff[(size_t)b->n];
	if (enc_host && total) memcpy(enc_host, b->enc.data(), total);
	if (enc_device && total) {
		(void)hipSetDevice(ctx->device);
		GD_HIP(hipMemcpy(enc_device, b->d_reads, total, hipMemcpyDeviceToHost));
	}
	return GDIET_OK;
}

struct gdiet_fastx_batch { GdFastxBatch *b; };
extern "C" gdiet_fastx_batch *gdiet_hip_fastx_detach(gdiet_fastx *fx)
{
	if (!fx || !fx->r) return nullptr;
	return new gdiet_fastx_batch{gd_fastx_detach(fx->r)};
}
extern "C" void gdiet_hip_fastx_batch_free(gdiet_fastx_batch *b)
{
	if (!b) return;
	delete b->b;
	delete b;
}

extern "C" int gdiet_hip_fastx_set_threads(gdiet_fastx *fx, int n)
{
	if (!fx || !fx->r || n < 1 || n > 64) return GDIET_E_PARAM;
	fx->r->n_threads = n;
	return GDIET_OK;
}

extern "C" void gdiet_hip_fastx_close(gdiet_fastx *fx)
{
	if (!fx) return;
	gd_fastx_close(fx->r);
	delete fx;
}
