// BGZF output (the writing side of bgzf.h): a stream writer that cuts what it is given into members of 65280 input bytes, compresses the
// members of one write side by side and writes them to a file descriptor.  Plain C++ + zlib; no HIP in here.  Who compresses: a
// GdBgzfDeflater if one is attached (the device: gd_bz_deflate_device behind gdiet_hip_bgzf_out_open, one wavefront per member,
// bgzf_deflate.hip.h), otherwise zlib's raw deflate at `level` on `threads` host threads with zlib's crc32 -- the same split the reader
// has (fastx_reader.h), and what lets the writer be tested without a GPU.
//
// Members are full (65280 bytes) except the one a flush or the close ends; close writes the 28-byte end-of-file member.  A write()
// to the file that comes back short or fails is an error; the writer then refuses everything but its destruction.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <string.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>
#include <zlib.h>
#include "bgzf.h"

enum { GD_BGZF_MEMBER_IN = 65280, GD_BGZF_SLOT = 65536 };

struct GdBgzfDeflater {
	virtual ~GdBgzfDeflater() {}
	// in[0, in_len) cut every 65280 bytes -> the members, one behind the other, in out[0, *out_len); out_cap is at least
	// ceil(in_len / 65280) * 65536.  Returns 0 or a negative code with the reason in why.
	virtual int deflate(const unsigned char *in, size_t in_len, unsigned char *out, size_t out_cap, size_t *out_len, std::string &why) = 0;
	// the same for an input the deflater's device already holds (d_in: a device pointer); only a device deflater can
	virtual int deflate_resident(const void *d_in, size_t in_len, unsigned char *out, size_t out_cap, size_t *out_len, std::string &why)
	{
		(void)d_in, (void)in_len, (void)out, (void)out_cap, (void)out_len;
		why = "this deflater takes no resident input";
		return -1;
	}
};

// one member through zlib: header with the BC subfield, raw deflate at `level`, CRC32 and ISIZE; a stored block if the level's stream
// does not fit (bgzip does the same).  out has room for 65536 bytes; returns the member's size, 0 if zlib fails.
static inline size_t gd_bgzf_member_host(const unsigned char *in, uint32_t n, unsigned char *out, int level)
{
	static const unsigned char head[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 'B', 'C', 0x02, 0};
	memcpy(out, head, 16);
	size_t stream = 0;
	for (int attempt = 0; attempt < 2; ++attempt) {
		z_stream z;
		memset(&z, 0, sizeof(z));
		if (deflateInit2(&z, attempt ? 0 : level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return 0;
		unsigned char none = 0;
		z.next_in = n ? const_cast<unsigned char *>(in) : &none, z.avail_in = n;
		z.next_out = out + 18, z.avail_out = GD_BGZF_SLOT - 18 - 8;
		const int rc = deflate(&z, Z_FINISH);
		stream = (GD_BGZF_SLOT - 18 - 8) - z.avail_out;
		deflateEnd(&z);
		if (rc == Z_STREAM_END) break;
		if (attempt) return 0;
	}
	const size_t total = 18 + stream + 8;
	const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), in, n);
	out[16] = (unsigned char)((total - 1) & 255), out[17] = (unsigned char)((total - 1) >> 8);
	for (int k = 0; k < 4; ++k) out[18 + stream + k] = (unsigned char)(crc >> (8 * k)), out[18 + stream + 4 + k] = (unsigned char)(n >> (8 * k));
	return total;
}

struct GdBgzfOut {
	int fd = -1;
	int level = -1, threads = 1;
	std::shared_ptr<GdBgzfDeflater> dev;
	std::vector<unsigned char> tail, obuf; // input that has not filled a member yet; the members of one write
	int64_t members_device = 0, members_host = 0, bytes_in = 0, bytes_out = 0;
	bool failed = false, dev_error = false;
	std::string msg;
	// internal hook of the sorted-BAM writer (bam_sorter.h): {input bytes, file bytes} of every member written, in file order, from which
	// the index builder makes virtual offsets.  Not set by anything else.
	std::vector<std::pair<uint64_t, uint64_t>> *member_log = nullptr;
	void log_members(const unsigned char *out, size_t out_len, size_t in_len)
	{
		for (size_t at = 0; member_log && at + 18 <= out_len;) { // BSIZE, the member's size - 1, sits at offset 16
			const size_t m = ((size_t)out[at + 16] | (size_t)out[at + 17] << 8) + 1, in = std::min<size_t>(in_len, GD_BGZF_MEMBER_IN);
			member_log->push_back(std::make_pair((uint64_t)in, (uint64_t)m));
			at += m, in_len -= in;
		}
	}

	int fail(const std::string &what) { failed = true, msg = what; return -1; }
	int put(const unsigned char *p, size_t n)
	{
		while (n) {
			const ssize_t k = ::write(fd, p, n);
			if (k < 0 && errno == EINTR) continue;
			if (k <= 0) return fail(k < 0 ? std::string("write: ") + strerror(errno) : std::string("write: short write"));
			if ((size_t)k < n) return fail("write: short write (" + std::to_string(k) + " of " + std::to_string(n) + " bytes)");
			p += k, n -= (size_t)k, bytes_out += k;
		}
		return 0;
	}
	// whole members of p[0, n): n is a multiple of 65280, or this is what a flush ends
	int members(const unsigned char *p, size_t n)
	{
		if (n == 0) return 0;
		const size_t k = (n + GD_BGZF_MEMBER_IN - 1) / GD_BGZF_MEMBER_IN;
		if (obuf.size() < k * GD_BGZF_SLOT) obuf.resize(k * GD_BGZF_SLOT);
		size_t out_len = 0;
		if (dev) {
			std::string why;
			if (dev->deflate(p, n, obuf.data(), obuf.size(), &out_len, why) != 0) { dev_error = true; return fail(why); }
			members_device += (int64_t)k;
		} else {
			std::vector<size_t> len(k, 0);
			std::atomic<size_t> next(0);
			auto work = [&]() {
				for (size_t i; (i = next.fetch_add(1)) < k;) {
					const size_t at = i * GD_BGZF_MEMBER_IN;
					len[i] = gd_bgzf_member_host(p + at, (uint32_t)std::min<size_t>(GD_BGZF_MEMBER_IN, n - at), obuf.data() + i * GD_BGZF_SLOT, level);
				}
			};
			const size_t nt = std::min<size_t>(threads < 1 ? 1 : (size_t)threads, k);
			std::vector<std::thread> th;
			for (size_t t = 1; t < nt; ++t) th.emplace_back(work);
			work();
			for (std::thread &t : th) t.join();
			for (size_t i = 0; i < k; ++i) {
				if (!len[i]) return fail("zlib: deflate failed");
				if (out_len != i * GD_BGZF_SLOT) memmove(obuf.data() + out_len, obuf.data() + i * GD_BGZF_SLOT, len[i]);
				out_len += len[i];
			}
			members_host += (int64_t)k;
		}
		bytes_in += (int64_t)n;
		log_members(obuf.data(), out_len, n);
		return put(obuf.data(), out_len);
	}
	// whole members of an input resident on the deflater's device: d_in[0, n), n a multiple of 65280.  (The BAM route: the caller has put
	// the waiting tail in front of what it encoded there, takes the tail away and sets the new one: gdiet_hip_bgzf_out_write_bam.)
	int members_resident(const void *d_in, size_t n)
	{
		if (failed || fd < 0 || !dev || n % GD_BGZF_MEMBER_IN) return -1;
		if (n == 0) return 0;
		const size_t k = n / GD_BGZF_MEMBER_IN;
		if (obuf.size() < k * GD_BGZF_SLOT) obuf.resize(k * GD_BGZF_SLOT);
		size_t out_len = 0;
		std::string why;
		if (dev->deflate_resident(d_in, n, obuf.data(), obuf.size(), &out_len, why) != 0) { dev_error = true; return fail(why); }
		members_device += (int64_t)k, bytes_in += (int64_t)n;
		log_members(obuf.data(), out_len, n);
		return put(obuf.data(), out_len);
	}
	int write(const unsigned char *p, size_t n)
	{
		if (failed || fd < 0) return -1;
		if (!tail.empty()) { // fill the waiting member first
			const size_t take = std::min<size_t>(n, GD_BGZF_MEMBER_IN - tail.size());
			tail.insert(tail.end(), p, p + take), p += take, n -= take;
			if (tail.size() < GD_BGZF_MEMBER_IN) return 0;
			if (members(tail.data(), tail.size())) return -1;
			tail.clear();
		}
		const size_t whole = n / GD_BGZF_MEMBER_IN * GD_BGZF_MEMBER_IN;
		if (members(p, whole)) return -1;
		tail.assign(p + whole, p + n);
		return 0;
	}
	int flush()
	{
		if (failed || fd < 0) return -1;
		if (members(tail.data(), tail.size())) return -1;
		tail.clear();
		return 0;
	}
	int close()
	{
		if (fd < 0) return failed ? -1 : 0;
		int rc = failed ? -1 : flush();
		if (!rc) log_members(GD_BGZF_EOF, GD_BGZF_EOF_LEN, 0), rc = put(GD_BGZF_EOF, GD_BGZF_EOF_LEN);
		if (::close(fd) != 0 && !rc) rc = fail(std::string("close: ") + strerror(errno));
		fd = -1;
		return rc;
	}
	~GdBgzfOut() { if (fd >= 0) ::close(fd); }
};
