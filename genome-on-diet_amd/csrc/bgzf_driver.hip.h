// Drivers of the BGZF kernels (bgzf_inflate.hip.h, bgzf_deflate.hip.h) and the entry points over them: gdiet_hip_bgzf_inflate,
// gdiet_hip_bgzf_deflate and the stream writer gdiet_hip_bgzf_out_*.  Included by fastx_dev_driver.hip.h, whose reader inflates through it
// (needs gdiet_ctx, GdLane, GdStreamMem, gd_parallel_for, err_mark.h).  Inflating runs on the lane gdiet_ctx::bz, deflating on
// gdiet_ctx::bzd; device memory is stream-ordered.  Failures leave their text with the calling thread (gd_err_fail).
#pragma once
#include "bgzf_inflate.hip.h"
#include "bgzf_deflate.hip.h"
#include "bgzf_out.h"
#include <fcntl.h>

// BGZF members on the device (bgzf_inflate.hip.h): the raw members and their table up, one wavefront per member, the inflated range down
// into the block the reader asked for.  The stream is synchronised before the host touches the bytes (it checks every member's length
// and CRC next).  Returns 0, -1 (the device failed) or -2 (a member's stream is not valid deflate), with the reason in why.
static int gd_bz_inflate_device(gdiet_ctx *ctx, const unsigned char *raw, size_t raw_len, const GdBgzfMember *m, size_t n, unsigned char *dst, size_t dst_len, uint32_t *out_len,
                                std::string &why)
{
	if (n == 0) return 0;
	for (size_t i = 0; i < n; ++i) // the kernel takes every range from this table: none may leave its buffer
		if (m[i].in_off > raw_len || m[i].in_len > raw_len - m[i].in_off || m[i].isize > GD_BGZF_MAX_ISIZE || m[i].out_off > dst_len || m[i].isize > dst_len - m[i].out_off) {
			why = "BGZF member " + std::to_string(i) + ": outside its buffers";
			return -2;
		}
	GdLane &L = ctx->bz;
	std::lock_guard<std::mutex> lk(L.mu);
	if (L.ready(ctx->device, 4, "device inflate", why)) return -1;
	hipStream_t s = L.stream;
	hipError_t e = hipSuccess;
	GdStreamMem mem(s);
	uint8_t *d_raw, *d_out;
	GdBgzfMember *d_tab;
	GdzResult *d_res;
	auto fail = [&](hipError_t err, const char *what) {
		mem.fail();
		why = std::string("device inflate: ") + what + ": " + hipGetErrorString(err);
		return -1;
	};
	std::vector<GdzResult> res(n);
	if ((e = mem.alloc(&d_raw, raw_len + 16)) != hipSuccess) return fail(e, "members");
	if ((e = mem.alloc(&d_out, dst_len + 16)) != hipSuccess) return fail(e, "output");
	if ((e = mem.alloc(&d_tab, sizeof(GdBgzfMember) * n)) != hipSuccess) return fail(e, "table");
	if ((e = mem.alloc(&d_res, sizeof(GdzResult) * n)) != hipSuccess) return fail(e, "results");
	(void)hipEventRecord(L.ev[0], s);
	if ((e = hipMemcpyAsync(d_raw, raw, raw_len, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "members copy");
	if ((e = hipMemcpyAsync(d_tab, m, sizeof(GdBgzfMember) * n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "table copy");
	if ((e = hipMemsetAsync(d_res, 0xff, sizeof(GdzResult) * n, s)) != hipSuccess) return fail(e, "results");
	(void)hipEventRecord(L.ev[1], s);
	hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((unsigned)n), dim3(64), 0, s, (const uint8_t *)d_raw, (const GdBgzfMember *)d_tab, (uint32_t)n, d_out, d_res);
	if ((e = hipGetLastError()) != hipSuccess) return fail(e, "launch");
	(void)hipEventRecord(L.ev[2], s);
	if (dst_len && (e = hipMemcpyAsync(dst, d_out, dst_len, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "output copy");
	if ((e = hipMemcpyAsync(res.data(), d_res, sizeof(GdzResult) * n, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "results copy");
	(void)hipEventRecord(L.ev[3], s);
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "kernel");
	for (int i = 0; i < 3; ++i) { // (for measurements: gdiet_hip_debug_bgzf_seconds)
		float ms = 0;
		if (hipEventElapsedTime(&ms, L.ev[i], L.ev[i + 1]) == hipSuccess) L.ms[i] += ms;
	}
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
// out[0, *out_len) back.  The stream is synchronised twice: once for the 8 bytes per member that the host's prefix sum needs (it also
// sizes the copy down), once before the host touches the bytes.  out_cap must be at least 65536 bytes per member.  Returns 0 or -1 (the
// device failed) with the reason in why.
static int gd_bzd_ready(gdiet_ctx *ctx, std::string &why) { return ctx->bzd.ready(ctx->device, 6, "device deflate", why); }
// The middle of it: members from an input that is already resident, d_in[0, in_len) in device memory (the BAM route encodes its records
// there: bam_driver.hip.h).  The caller holds bzd.mu, has made the stream and the events (gd_bzd_ready) and recorded ev[0] and [1]
// around whatever brought the input up; d_in stays the caller's.  On failure the stream has been synchronised.
static int gd_bz_deflate_resident(gdiet_ctx *ctx, const uint8_t *d_in, size_t in_len, unsigned char *out, size_t out_cap, size_t *out_len, std::string &why)
{
	const size_t n = (in_len + GDD_MAX_IN - 1) / GDD_MAX_IN;
	GdLane &L = ctx->bzd;
	hipStream_t s = L.stream;
	hipError_t e = hipSuccess;
	GdStreamMem mem(s);
	uint8_t *d_slots, *d_out;
	GddResult *d_res;
	uint64_t *d_off; // off[n], then len[n] as 32-bit words
	auto fail = [&](hipError_t err, const char *what) {
		mem.fail();
		why = std::string("device deflate: ") + what + ": " + hipGetErrorString(err);
		return -1;
	};
	std::vector<GddResult> res(n);
	if ((e = mem.alloc(&d_slots, n * GDD_SLOT)) != hipSuccess) return fail(e, "slots");
	if ((e = mem.alloc(&d_res, sizeof(GddResult) * n)) != hipSuccess) return fail(e, "results");
	if ((e = hipMemsetAsync(d_res, 0xff, sizeof(GddResult) * n, s)) != hipSuccess) return fail(e, "results");
	(void)hipEventRecord(L.ev[1], s);
	hipLaunchKernelGGL(bgzf_deflate_kernel, dim3((unsigned)n), dim3(64), 0, s, d_in, (uint64_t)in_len, (uint32_t)n, d_slots, d_res);
	if ((e = hipGetLastError()) != hipSuccess) return fail(e, "launch");
	(void)hipEventRecord(L.ev[2], s);
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
	if ((e = mem.alloc(&d_off, sizeof(uint64_t) * tab.size())) != hipSuccess) return fail(e, "offsets");
	if ((e = mem.alloc(&d_out, total + 16)) != hipSuccess) return fail(e, "output");
	if ((e = hipMemcpyAsync(d_off, tab.data(), sizeof(uint64_t) * tab.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "offsets copy");
	(void)hipEventRecord(L.ev[3], s);
	hipLaunchKernelGGL(bgzf_pack_kernel, dim3((unsigned)n), dim3(256), 0, s, (const uint8_t *)d_slots, (const uint64_t *)d_off, (const uint32_t *)(d_off + n), (uint32_t)n, d_out);
	if ((e = hipGetLastError()) != hipSuccess) return fail(e, "pack launch");
	(void)hipEventRecord(L.ev[4], s);
	if ((e = hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e, "output copy");
	(void)hipEventRecord(L.ev[5], s);
	if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "pack kernel");
	{ // (for measurements: gdiet_hip_debug_bgzf_deflate_seconds)
		float ms = 0;
		if (hipEventElapsedTime(&ms, L.ev[0], L.ev[1]) == hipSuccess) L.ms[0] += ms;
		if (hipEventElapsedTime(&ms, L.ev[1], L.ev[2]) == hipSuccess) L.ms[1] += ms;
		if (hipEventElapsedTime(&ms, L.ev[3], L.ev[4]) == hipSuccess) L.ms[1] += ms;
		if (hipEventElapsedTime(&ms, L.ev[4], L.ev[5]) == hipSuccess) L.ms[2] += ms;
	}
	*out_len = total;
	return 0;
}

static int gd_bz_deflate_device(gdiet_ctx *ctx, const unsigned char *in, size_t in_len, unsigned char *out, size_t out_cap, size_t *out_len, std::string &why)
{
	*out_len = 0;
	const size_t n = (in_len + GDD_MAX_IN - 1) / GDD_MAX_IN;
	if (n == 0) return 0;
	if (n > ((size_t)1 << 30) || out_cap / GDD_SLOT < n) { why = "device deflate: the output holds fewer than 65536 bytes per member"; return -1; }
	GdLane &L = ctx->bzd;
	std::lock_guard<std::mutex> lk(L.mu);
	if (gd_bzd_ready(ctx, why)) return -1;
	hipStream_t s = L.stream;
	hipError_t e = hipSuccess;
	GdStreamMem mem(s);
	uint8_t *d_in;
	auto fail = [&](hipError_t err, const char *what) {
		mem.fail();
		why = std::string("device deflate: ") + what + ": " + hipGetErrorString(err);
		return -1;
	};
	if ((e = mem.alloc(&d_in, in_len + 16)) != hipSuccess) return fail(e, "input");
	(void)hipEventRecord(L.ev[0], s);
	if ((e = hipMemcpyAsync(d_in, in, in_len, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "input copy");
	return gd_bz_deflate_resident(ctx, d_in, in_len, out, out_cap, out_len, why);
}

extern "C" int gdiet_hip_bgzf_inflate(gdiet_ctx *ctx, const uint8_t *raw, size_t raw_len, uint8_t *out, size_t out_cap, size_t *out_len)
{
	if (!ctx || (!raw && raw_len) || !out_len) return GDIET_E_PARAM;
	*out_len = 0;
	gd_err_clear(); // (an earlier refusal on this thread is not this call's text)
	auto fail = [&](int rc, const std::string &what) { return gd_err_fail(ctx, rc, "gdiet_hip_bgzf_inflate: " + what); };
	std::vector<GdBgzfMember> tab;
	size_t inc = 0, bad_at = 0;
	std::string why;
	if (gd_bgzf_scan(raw, raw_len, tab, &inc, &bad_at, &why) != GD_BGZF_OK) return fail(GDIET_E_PARAM, "offset " + std::to_string(bad_at) + ": " + why);
	if (inc != raw_len) return fail(GDIET_E_PARAM, "offset " + std::to_string(inc) + ": the range ends inside a member");
	const size_t total = tab.empty() ? 0 : (size_t)(tab.back().out_off + tab.back().isize);
	*out_len = total;
	if (!out) return GDIET_OK; // sizes first
	if (total > out_cap) return fail(GDIET_E_PARAM, "the members inflate to " + std::to_string(total) + " bytes, out holds " + std::to_string(out_cap));
	std::vector<uint32_t> lens(tab.size(), 0);
	const int rc = gd_bz_inflate_device(ctx, raw, raw_len, tab.data(), tab.size(), out, total, lens.data(), why);
	if (rc < 0) return fail(rc == -1 ? GDIET_E_HIP : GDIET_E_PARAM, why);
	std::vector<std::string> msg(tab.size());
	std::vector<uint8_t> ok(tab.size(), 1);
	gd_parallel_for(ctx, ctx->host_threads, (int)tab.size(), [&](int k) { ok[(size_t)k] = gd_bgzf_check(tab[(size_t)k], (size_t)k, out + tab[(size_t)k].out_off, lens[(size_t)k], &msg[(size_t)k]); });
	for (size_t k = 0; k < tab.size(); ++k)
		if (!ok[k]) return fail(GDIET_E_PARAM, msg[k]);
	return GDIET_OK;
}

// ---- BGZF output -------------------------------------------------------------------------------------------------------------------
extern "C" int gdiet_hip_bgzf_deflate(gdiet_ctx *ctx, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap, size_t *out_len, int flags)
{
	if (!ctx || !out_len) return GDIET_E_PARAM;
	*out_len = 0;
	gd_err_clear();
	if (!in && in_len) return gd_err_fail(ctx, GDIET_E_PARAM, "gdiet_hip_bgzf_deflate: no input for " + std::to_string(in_len) + " bytes");
	const size_t n = (in_len + GDD_MAX_IN - 1) / GDD_MAX_IN, bound = n * GDD_SLOT + GD_BGZF_EOF_LEN;
	if (!out) { *out_len = bound; return GDIET_OK; } // sizes first
	if (out_cap < bound) return gd_err_fail(ctx, GDIET_E_PARAM, "gdiet_hip_bgzf_deflate: out holds " + std::to_string(out_cap) + " bytes, the bound is " + std::to_string(bound));
	size_t got = 0;
	std::string why;
	const int rc = gd_bz_deflate_device(ctx, in, in_len, out, out_cap, &got, why);
	if (rc < 0) return gd_err_fail(ctx, GDIET_E_HIP, "gdiet_hip_bgzf_deflate: " + why);
	if (flags & 1) memcpy(out + got, GD_BGZF_EOF, GD_BGZF_EOF_LEN), got += GD_BGZF_EOF_LEN;
	*out_len = got;
	return GDIET_OK;
}

struct GdBzdExecutor : GdBgzfDeflater {
	gdiet_ctx *ctx;
	explicit GdBzdExecutor(gdiet_ctx *c) : ctx(c) {}
	int deflate(const unsigned char *in, size_t in_len, unsigned char *out, size_t out_cap, size_t *out_len, std::string &why) override
	{
		return gd_bz_deflate_device(ctx, in, in_len, out, out_cap, out_len, why);
	}
	int deflate_resident(const void *d_in, size_t in_len, unsigned char *out, size_t out_cap, size_t *out_len, std::string &why) override
	{
		*out_len = 0;
		const size_t n = (in_len + GDD_MAX_IN - 1) / GDD_MAX_IN;
		if (n == 0) return 0;
		if (n > ((size_t)1 << 30) || out_cap / GDD_SLOT < n) { why = "device deflate: the output holds fewer than 65536 bytes per member"; return -1; }
		std::lock_guard<std::mutex> lk(ctx->bzd.mu);
		if (gd_bzd_ready(ctx, why)) return -1;
		(void)hipEventRecord(ctx->bzd.ev[0], ctx->bzd.stream); // nothing goes up: the input is there
		return gd_bz_deflate_resident(ctx, (const uint8_t *)d_in, in_len, out, out_cap, out_len, why);
	}
};
// The accumulators attached to a writer or a sorter (accum_driver.hip.h): fixed slots, and the slot order is the order in which a call
// locks them.  An empty slot costs nothing.
struct GdAccum;
enum { GD_ACC_COV = 0, GD_ACC_PILE, GD_ACC_STATS, GD_ACC_SLOTS };
struct GdAccumSet { GdAccum *slot[GD_ACC_SLOTS] = {}; };
struct gdiet_bgzf_out { GdBgzfOut w; gdiet_ctx *ctx = nullptr; GdAccumSet acc; /* gdiet_hip_bgzf_out_set_coverage / _set_pileup / _set_stats */ };

extern "C" int gdiet_hip_bgzf_out_open(gdiet_ctx *ctx, const char *path, int level, int threads, gdiet_bgzf_out **out)
{
	if (!path || !out || level < -1 || level > 9) return GDIET_E_PARAM;
	*out = nullptr;
	gd_err_clear();
	const int fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
	if (fd < 0) return gd_err_fail(ctx, GDIET_E_PARAM, std::string("gdiet_hip_bgzf_out_open: ") + path + ": " + strerror(errno));
	gdiet_bgzf_out *h = new gdiet_bgzf_out();
	h->ctx = ctx, h->w.fd = fd, h->w.level = level, h->w.threads = threads < 1 ? 1 : threads;
	if (ctx) h->w.dev = std::make_shared<GdBzdExecutor>(ctx);
	*out = h;
	return GDIET_OK;
}
static int gd_bzo_done(gdiet_bgzf_out *h, int rc)
{
	if (!rc) return GDIET_OK;
	return gd_err_fail(h->ctx, h->w.dev_error ? GDIET_E_HIP : GDIET_E_PARAM, "BGZF writer: " + (h->w.msg.empty() ? std::string("used after an error or after close") : h->w.msg));
}
extern "C" int gdiet_hip_bgzf_out_write(gdiet_bgzf_out *h, const void *bytes, size_t n)
{
	if (!h || (!bytes && n)) return GDIET_E_PARAM;
	gd_err_clear();
	return gd_bzo_done(h, h->w.write((const unsigned char *)bytes, n));
}
extern "C" int gdiet_hip_bgzf_out_flush(gdiet_bgzf_out *h)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	return gd_bzo_done(h, h->w.flush());
}
extern "C" int gdiet_hip_bgzf_out_close(gdiet_bgzf_out *h)
{
	if (!h) return GDIET_E_PARAM;
	gd_err_clear();
	const int rc = gd_bzo_done(h, h->w.close());
	delete h;
	return rc;
}
extern "C" int gdiet_hip_bgzf_out_stats(const gdiet_bgzf_out *h, int64_t *members_device, int64_t *members_host, int64_t *bytes_in, int64_t *bytes_out)
{
	if (!h) return GDIET_E_PARAM;
	if (members_device) *members_device = h->w.members_device;
	if (members_host) *members_host = h->w.members_host;
	if (bytes_in) *bytes_in = h->w.bytes_in;
	if (bytes_out) *bytes_out = h->w.bytes_out;
	return GDIET_OK;
}
// measurement only (tools/map_file.py; not declared in include/gdiet_hip.h): the device's side of compressing since the context was
// created, in seconds: copy up, the deflate and pack kernels, copy down (HIP events)
extern "C" int gdiet_hip_debug_bgzf_deflate_seconds(gdiet_ctx *ctx, double *out3)
{
	if (!ctx || !out3) return GDIET_E_PARAM;
	std::lock_guard<std::mutex> lk(ctx->bzd.mu);
	for (int i = 0; i < 3; ++i) out3[i] = 1e-3 * ctx->bzd.ms[i];
	return GDIET_OK;
}
