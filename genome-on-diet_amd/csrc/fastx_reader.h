// Input half of SURVEY 8(f) rank 2: FASTA / FASTQ (plain or gzip) -> mini-batches, with the record grammar of the reference's
// kseq_read (LR/kseq.h:191-232) and the batching rule of mm_bseq_read3 (LR/bseq.c:80-121), so that a batch holds exactly the
// reads, names, comments and quality strings the reference would hand to its worker threads.  Plain C++ + zlib; no HIP.
//
// What differs from the reference is the mechanics: one large buffer refilled by gzread, lines located with memchr, all strings
// of a batch parsed straight into one arena (no allocation per read), plain files read without zlib's extra copy.
//
// Optional device mode (GdFastx::dev, installed by gdiet_hip_fastx_attach): the strict four-line FASTQ prefix of every block is parsed
// by an executor -- on the GPU, fastx_dev.hip.h -- and the sequential grammar below takes over at the first record that is not strict,
// exactly as it does behind a wrong seam.  This header itself stays free of HIP.
//
// BGZF input (bgzf.h) is a third source next to the plain file and zlib's gzread: a regular file whose first member is a BGZF member and
// whose last 28 bytes are the BGZF end-of-file member is read raw, its members are located by their headers, and the members of one read
// are inflated side by side -- by zlib's raw inflate on n_threads threads, or, attached, by GdFastxDevice::inflate -- into the block the
// reader asked for (the file is read ahead until the members in hand inflate to the block's size, so a read is short of it by less than
// one member whatever the compression ratio); behind that the reader sees plain bytes.  Every member, whoever inflated it, must come out ISIZE bytes long with the
// trailer's CRC32 (checked on the reader's threads): anything else is a read error (io_error, io_msg; read_batch < 0), and so is a member
// without a BC subfield in the middle of such a file (mixed streams are not read: GDIET_BGZF=0, read at open, sends every file through
// gzread, as do stdin, single-stream gzip and a BGZF file without its end marker).  A read error surfaces when the block that holds it is
// taken, so the number of reads of earlier blocks handed out before it is not gzread's count, which stops at the failing byte.
//
// BAM input (bam_in.h) is a second grammar behind the same three sources: a stream whose first four bytes are "BAM\1" is walked record by
// record (parse_bam) in place of parse_range / find_seam, and every kept record's SEQ and QUAL are unpacked into the chunk's arena -- by the
// reader's threads, records side by side, or, attached, by GdFastxDevice::bam_unpack.  Chunks, batches and detaching are the same.  A
// malformed record is a read error that surfaces behind the records in front of it (GdFastxChunk::fail).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <algorithm>
#include <atomic>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include <zlib.h>
#include <errno.h>
#include <fcntl.h>
#include <unistd.h>
#include <time.h>
#include <sys/stat.h>
#include "fastx_dev.h"
#include "bgzf.h"
#include "bam_in.h"

// Record parser over a byte range held in memory (kseq_read's grammar); the reader below feeds it blocks of the file.
struct GdFastxParser {
	const unsigned char *b = nullptr;
	size_t begin = 0, end = 0;
	bool eof = false;  // ran off the end of the range (kseq's end-of-file behaviour applies from then on)
	int last_char = 0; // kseq_t::last_char: the header character of the next record has been consumed already
	std::string arena, scratch; // every string of the parsed records, NUL-terminated
	bool fill() { eof = true; return false; }
	int getc_()
	{
		if (begin >= end && !fill()) return -1;
		return b[begin++];
	}
	// ks_getuntil2 (LR/kseq.h:102-149) for KS_SEP_LINE (line = true) and KS_SEP_SPACE, appending to s, whose current field starts
	// at `base`; returns the length of the field, or -1 at the end of the file with nothing read
	long getuntil(bool line, std::string &s, size_t base, int *dret)
	{
		bool gotany = false;
		if (dret) *dret = 0;
		for (;;) {
			if (begin >= end && !fill()) break;
			size_t i;
			if (line) {
				const void *p = memchr(b + begin, '\n', end - begin);
				i = p ? (size_t)((const unsigned char *)p - b) : end;
			} else {
				for (i = begin; i < end; ++i) {
					const unsigned char c = b[i];
					if (c == ' ' || (c >= '\t' && c <= '\r')) break; // isspace() in the C locale
				}
			}
			gotany = true;
			s.append((const char *)b + begin, i - begin);
			begin = i + 1;
			if (i < end) { if (dret) *dret = b[i]; break; }
		}
		if (!gotany && eof) return -1;
		if (line && s.size() - base > 1 && s.back() == '\r') s.pop_back();
		return (long)(s.size() - base);
	}
	// kseq_read (LR/kseq.h:191-232) into the arena: >= 0 sequence length, -1 end of file, -2 truncated quality string.  On success
	// o[0..3] are the offsets of name, comment, seq, qual (-1: none kept); on failure the arena is as before.
	long read_record(bool with_qual, bool with_comment, int64_t o[4])
	{
		int c;
		if (last_char == 0) { // jump to the next header line
			while ((c = getc_()) != -1 && c != '>' && c != '@') {}
			if (c == -1) return -1;
			last_char = c;
		}
		const size_t start = arena.size();
		o[0] = (int64_t)start, o[1] = o[3] = -1;
		if (getuntil(false, arena, start, &c) < 0) { arena.resize(start); return -1; }
		arena.push_back('\0');
		if (c != '\n') { // FASTA/Q comment: the rest of the header line
			if (with_comment) {
				const size_t cs = arena.size();
				if (getuntil(true, arena, cs, nullptr) > 0) o[1] = (int64_t)cs, arena.push_back('\0');
				else arena.resize(cs);
			} else scratch.clear(), getuntil(true, scratch, 0, nullptr);
		}
		const size_t ss = arena.size();
		o[2] = (int64_t)ss;
		while ((c = getc_()) != -1 && c != '>' && c != '+' && c != '@') {
			if (c == '\n') continue; // skip empty lines
			arena.push_back((char)c);
			getuntil(true, arena, ss, nullptr); // the rest of the line
		}
		if (c == '>' || c == '@') last_char = c;
		const size_t l_seq = arena.size() - ss;
		for (size_t i = ss; i < arena.size(); ++i) if (arena[i] == 'u' || arena[i] == 'U') --arena[i]; // U -> T (kseq2bseq, LR/bseq.c:71-73)
		arena.push_back('\0');
		if (c != '+') return (long)l_seq; // FASTA
		while ((c = getc_()) != -1 && c != '\n') {} // the rest of the '+' line
		if (c == -1) { arena.resize(start); return -2; }
		const size_t qs = arena.size();
		while (getuntil(true, arena, qs, nullptr) >= 0 && arena.size() - qs < l_seq) {}
		last_char = 0;
		if (arena.size() - qs != l_seq) { arena.resize(start); return -2; }
		if (with_qual && l_seq) o[3] = (int64_t)qs, arena.push_back('\0');
		else arena.resize(qs);
		return (long)l_seq;
	}
};

// Block buffers of device-parsed chunks on their way back to the reader.  A chunk of a batch in flight dies on the thread that frees the
// batch, long after the reader has moved on (or has been closed: the pool belongs to whoever holds it last); fresh pages for every 8 MiB
// block would cost more than parsing it.
struct GdFastxBufPool {
	std::mutex mu;
	std::vector<std::vector<unsigned char>> bufs;
};

// The parsed records of one stretch of the file, in file order
struct GdFastxChunk {
	std::string arena;
	// a device-parsed chunk owns the bytes of its block in place of an arena: the strings are the lines themselves, NUL-terminated in place
	std::vector<unsigned char> buf;
	const char *text = nullptr;   // the block inside buf (off[] counts from here)
	std::vector<GdxRec> rec;      // the device's record table
	std::shared_ptr<void> dev;    // the executor's copy of the block and of the table, alive until every record is handed out and its batch built
	bool on_device = false;
	std::shared_ptr<GdFastxBufPool> home; // where buf goes when the chunk dies
	const char *base() const { return on_device ? text : arena.data(); }
	GdFastxChunk() = default;
	GdFastxChunk(const GdFastxChunk &) = delete;
	GdFastxChunk &operator=(const GdFastxChunk &) = delete;
	~GdFastxChunk()
	{
		if (!home || !buf.capacity()) return;
		std::lock_guard<std::mutex> lk(home->mu);
		if (home->bufs.size() < 24) home->bufs.push_back(std::move(buf));
	}
	std::vector<int64_t> off;     // 4 per record: name, comment, seq, qual (-1 = none)
	std::vector<int32_t> len;     // sequence length per record
	std::vector<uint8_t> err;     // per record: a malformed record (kseq_read < -1) FOLLOWED this one ...
	bool err_first = false;       // ... or preceded the first one
	size_t next = 0;              // records handed out so far
	std::string fail;             // BAM: a malformed record followed the last one of this chunk: the read error once they are handed out
};

// What parses the strict prefix of a block (fastx_dev.h) somewhere else.  parse() fills rec with the records [0, n_acc) of b[0, n) and
// returns n_acc (0: nothing for the device in this block; < 0: the device failed); dev keeps its copy of the block for the batches.
struct GdFastxDevice {
	virtual ~GdFastxDevice() {}
	virtual long parse(const unsigned char *b, size_t n, std::vector<GdxRec> &rec, std::shared_ptr<void> &dev) = 0;
	// BGZF: the deflate streams of the members m[0, n) of raw[0, raw_len) into dst[m[i].out_off ..), dst_len bytes in all; out_len[i] is what
	// member i produced (the caller checks it, and the CRC).  0; -1 with the reason in why when the device failed (dev_error); -2 when a
	// member's stream is not valid deflate (a read error).  Either way the read fails: nothing is inflated elsewhere for the same file.
	virtual int inflate(const unsigned char *raw, size_t raw_len, const GdBgzfMember *m, size_t n, unsigned char *dst, size_t dst_len, uint32_t *out_len, std::string &why)
	{
		(void)raw, (void)raw_len, (void)m, (void)n, (void)dst, (void)dst_len, (void)out_len;
		why = "this device does not inflate";
		return -1;
	}
	// BAM: the text of the rows (bam_in.h; already checked against the block b[0, n)) into text[0, text_len); dev keeps the device's copy
	// of the text and a GdxRec table over it for the batches.  0; -1 with the reason in why when the device failed (dev_error).
	virtual int bam_unpack(const unsigned char *b, size_t n, const GdiRow *rows, size_t n_rows, uint64_t text_len, char *text, std::shared_ptr<void> &dev, std::string &why)
	{
		(void)b, (void)n, (void)rows, (void)n_rows, (void)text_len, (void)text, (void)dev;
		why = "this device does not unpack BAM";
		return -1;
	}
};

struct GdFastx {
	gzFile fp = nullptr; // gzip input, or stdin
	std::shared_ptr<GdFastxDevice> dev; // device mode, from the next block on
	std::shared_ptr<GdFastxBufPool> bufpool = std::make_shared<GdFastxBufPool>();
	bool dev_error = false;
	int64_t n_rec_device = 0, n_rec_host = 0, n_blocks = 0, n_blocks_handed = 0; // who parsed what since the reader was opened
	int fd = -1;         // plain file: read() straight into the block (gzread would copy it once more)
	bool file_end = false, io_error = false;
	// BGZF: fd is read raw; raw[raw_pos, raw_fill) is what no read has taken yet (an incomplete trailing member stays for the next one)
	bool bgzf = false, raw_eof = false, io_dev_err = false;
	std::vector<unsigned char> raw;
	size_t raw_pos = 0, raw_fill = 0;
	uint64_t raw_base = 0; // file offset of raw[0]
	std::string io_msg;    // what the read error was
	std::deque<z_stream> bz_zs; // (a deque: zlib refuses a stream that has moved, and more threads may be asked for in mid-file)
	std::atomic<int64_t> bz_members_device{0}, bz_members_host{0}, bz_bytes_in{0}, bz_bytes_out{0};
	std::atomic<int64_t> bz_ns[3] = {{0}, {0}, {0}}; // nanoseconds in: raw read, inflate (attached: copies and kernel), length / CRC check
	int n_threads = 1;
	size_t block_size = (size_t)8 << 20; // per parser thread
	// The block being parsed is bp[0, fill) = the unparsed tail of the previous block + fresh bytes; bp points into block.  While it
	// is parsed, an I/O thread reads the next stretch of the file into `other` (behind room for the tail, which is copied in front
	// of it once known), so reading and parsing overlap and no block is ever moved.
	std::vector<unsigned char> block, other;
	const unsigned char *bp = nullptr;
	size_t fill = 0;
	std::thread io;
	bool io_pending = false;
	size_t io_base = 0, io_tail = 0, io_got = 0; // other[io_base - io_tail, io_base) = tail, other[io_base, io_base + io_got) = fresh
	bool io_eof = false, io_err = false;
	std::deque<std::shared_ptr<GdFastxChunk>> ready; // parsed, not yet (completely) handed out
	std::vector<std::shared_ptr<GdFastxChunk>> lent; // every chunk the last batch points into: alive until the next call (or, detached, longer)
	std::vector<std::shared_ptr<GdFastxChunk>> pool; // used chunks, kept for their memory (fresh pages cost several times the parsing)
	std::mutex pool_mu;
	bool with_qual = true, with_comment = false, flags_set = false;
	// BAM (bam_in.h): format is decided on the first four bytes of the stream (-1: not yet; 0: FASTA / FASTQ; 1: BAM)
	int format = -1;
	bool bam_header_done = false;
	uint64_t bam_base = 0, bam_ordinal = 0; // stream offset of bp[0]; records walked so far
	std::vector<const char *> v_name, v_comment, v_seq, v_qual;
	std::vector<int32_t> v_len;
	std::vector<int32_t> v_chunk, v_rec; // where read i of the batch came from: lent[v_chunk[i]], its record v_rec[i]

	static size_t qname_len(const char *s) // mm_qname_len (LR/bseq.h:30-36)
	{
		const size_t l = strlen(s);
		return l >= 3 && s[l - 1] >= '0' && s[l - 1] <= '9' && s[l - 2] == '/' ? l - 2 : l;
	}
	// read up to `want` bytes to dst; sets eof / err
	void io_read(unsigned char *dst, size_t want, size_t *got_, bool *eof_, bool *err_, bool use_dev)
	{
		size_t got = 0;
		*eof_ = *err_ = false;
		if (bgzf) { bgzf_read(dst, want, got_, eof_, err_, use_dev); return; }
		while (got < want) {
			long n;
			if (fd >= 0) {
				do n = (long)::read(fd, dst + got, want - got); while (n < 0 && errno == EINTR);
			} else n = gzread(fp, dst + got, (unsigned)std::min<size_t>(want - got, (size_t)1 << 30));
			if (n < 0) { *err_ = true, *eof_ = true; break; }
			if (n == 0) { *eof_ = true; break; }
			got += (size_t)n;
		}
		*got_ = got;
	}
	template <class F> void bz_parallel(size_t nt, size_t n, F f)
	{
		const size_t t = std::min<size_t>(nt, n);
		if (t <= 1) { for (size_t k = 0; k < n; ++k) f(k, (size_t)0); return; }
		std::atomic<size_t> next{0};
		std::vector<std::thread> th;
		auto run = [&](size_t w) { for (size_t k; (k = next++) < n;) f(k, w); };
		for (size_t w = 1; w < t; ++w) th.emplace_back(run, w);
		run(0);
		for (auto &x : th) x.join();
	}
	static int64_t now_ns()
	{
		struct timespec ts;
		clock_gettime(CLOCK_MONOTONIC, &ts);
		return (int64_t)ts.tv_sec * 1000000000 + ts.tv_nsec;
	}
	// io_read of a BGZF file: whole members while the sum of their ISIZE stays within `want`, at least one (dst has room for want + 64 KiB:
	// room_for), inflated to dst.  Returns with got > 0, or at the end of the file, or with an error.
	void bgzf_read(unsigned char *dst, size_t want, size_t *got_, bool *eof_, bool *err_, bool use_dev)
	{
		*got_ = 0;
		auto fail = [&](const std::string &what) { io_msg = what, *err_ = true, *eof_ = true; };
		std::vector<GdBgzfMember> tab;
		const size_t nt = (size_t)std::max(1, n_threads); // (once per read: gdiet_hip_fastx_set_threads may write it meanwhile)
		// A member is at most 64 KiB: with `need` bytes unread, one is complete.  The first guess is that the members of `want` output bytes take
		// half as many; when the walk below runs out of bytes before it has `want` output bytes, the file is read further and walked again,
		// up to `cap` (data that does not compress: a stored member is 36 bytes larger than its output), so that a read is only short of
		// `want` by less than one member, whatever the compression ratio.  The file is always read a quarter MiB past `need`, so that small
		// reads do not move the rest of the buffer every time.
		const size_t cap = want + want / 8 + 4 * (size_t)GD_BGZF_MAX_ISIZE;
		size_t need = std::min(cap, want / 2 + (size_t)GD_BGZF_MAX_ISIZE);
		for (;;) {
			const size_t goal = need + ((size_t)4 << 16);
			if (!raw_eof && raw_fill - raw_pos < need) {
				const int64_t t0 = now_ns();
				if (raw_pos) memmove(raw.data(), raw.data() + raw_pos, raw_fill - raw_pos), raw_fill -= raw_pos, raw_base += raw_pos, raw_pos = 0;
				if (raw.size() < goal) raw.resize(goal);
				while (raw_fill < goal) {
					long n;
					do n = (long)::read(fd, raw.data() + raw_fill, goal - raw_fill); while (n < 0 && errno == EINTR);
					if (n < 0) { fail(std::string("read: ") + strerror(errno)); return; }
					if (n == 0) { raw_eof = true; break; }
					raw_fill += (size_t)n;
				}
				bz_ns[0] += now_ns() - t0;
			}
			const unsigned char *r = raw.data() + raw_pos;
			const size_t avail = raw_fill - raw_pos;
			size_t taken = 0, bad_at = 0;
			std::string why;
			bool full = false;
			const int rc = gd_bgzf_scan(r, avail, tab, &taken, &bad_at, &why, want, &full);
			if (rc == GD_BGZF_OK && !full && !raw_eof && need < cap) { need = std::min(cap, std::max(2 * need, avail + ((size_t)4 << 16))); continue; } // more members may fit: read on
			if (rc < 0 && tab.empty()) {
				fail("offset " + std::to_string(raw_base + raw_pos + bad_at) + ": " + why + ": not a BGZF member inside a BGZF file (set GDIET_BGZF=0 to read the file through zlib)");
				return;
			}
			if (tab.empty()) {
				if (avail) fail("offset " + std::to_string(raw_base + raw_pos) + ": the file ends inside a BGZF member");
				else *eof_ = true;
				return;
			}
			taken = (size_t)(tab.back().in_off + tab.back().in_len + 8); // (behind a member that is not one, the members in front of it are still read)
			const size_t n = tab.size(), total = (size_t)(tab.back().out_off + tab.back().isize);
			std::vector<uint32_t> out_len(n, 0);
			std::vector<std::string> msg(n);
			std::vector<uint8_t> ok(n, 1);
			int64_t t0 = now_ns();
			if (use_dev) {
				const int drc = dev->inflate(r, taken, tab.data(), n, dst, total, out_len.data(), why);
				if (drc < 0) { io_dev_err = drc == -1; fail(why); return; }
				bz_ns[1] += now_ns() - t0, t0 = now_ns();
				bz_parallel(nt, n, [&](size_t k, size_t) { ok[k] = gd_bgzf_check(tab[k], k, dst + tab[k].out_off, out_len[k], &msg[k]); });
				bz_ns[2] += now_ns() - t0;
				bz_members_device += (int64_t)n;
			} else {
				std::deque<z_stream> &zs = bz_zs; // (one per thread, kept for the file: zlib's state is 40 KiB to set up)
				while (zs.size() < nt) { zs.emplace_back(); memset(&zs.back(), 0, sizeof(z_stream)); }
				bz_parallel(nt, n, [&](size_t k, size_t w) {
					ok[k] = gd_bgzf_inflate_host(&zs[w], r + tab[k].in_off, tab[k].in_len, dst + tab[k].out_off, tab[k].isize, &out_len[k], k, &msg[k]) &&
					        gd_bgzf_check(tab[k], k, dst + tab[k].out_off, out_len[k], &msg[k]);
				});
				bz_ns[1] += now_ns() - t0;
				bz_members_host += (int64_t)n;
			}
			for (size_t k = 0; k < n; ++k)
				if (!ok[k]) { fail("offset " + std::to_string(raw_base + raw_pos + tab[k].in_off) + ": " + msg[k]); return; }
			raw_pos += taken;
			bz_bytes_in += (int64_t)taken, bz_bytes_out += (int64_t)total;
			if (raw_eof && raw_pos == raw_fill) *eof_ = true;
			if (total || *eof_) { *got_ = total; return; } // (only empty members so far: read on)
		}
	}
	// bytes a block must have room for behind the place a read of `want` bytes starts at
	size_t room_for(size_t want) const { return want + (bgzf ? (size_t)GD_BGZF_MAX_ISIZE : 0); }
	// start reading the next `want` bytes into `other`, in front of which the tail bp[pos, fill) of the current block is placed
	void prefetch(size_t pos, size_t want)
	{
		const size_t t = fill - pos;
		io_tail = t, io_base = (t + 4095) & ~(size_t)4095;
		if (other.size() < io_base + room_for(want)) other.resize(io_base + room_for(want));
		if (t) memcpy(other.data() + io_base - t, bp + pos, t);
		if (file_end) { io_got = 0, io_eof = true, io_err = false, io_pending = true; return; } // nothing more to read: only the tail moves
		unsigned char *dst = other.data() + io_base;
		const bool use_dev = dev && !dev_error;
		io = std::thread([this, dst, want, use_dev] { io_read(dst, want, &io_got, &io_eof, &io_err, use_dev); });
		io_pending = true;
	}
	// make the prefetched stretch the current block
	void take_prefetched()
	{
		if (io.joinable()) io.join();
		io_pending = false;
		block.swap(other);
		bp = block.data() + io_base - io_tail;
		fill = io_tail + io_got;
		if (io_eof) file_end = true;
		if (io_err) io_error = true;
		if (io_dev_err) dev_error = true;
	}
	// Parse block[from, fill) sequentially into C, never starting a record at or after `stop` (the next parser's first record, or
	// `fill`).  Returns where the next record would start: exactly `stop` when the stretch ends on the seam (or the range is
	// exhausted); something else tells the caller that the seam was not a record boundary.  A record cut off by the end of the
	// block (more of the file to come) is not parsed: its start is returned.
	size_t parse_range(GdFastxChunk &C, size_t from, size_t stop, bool last_of_file) const
	{
		GdFastxParser P;
		P.b = bp, P.end = fill;
		size_t pos = from;
		P.arena.swap(C.arena);
		for (;;) {
			// the header scan of kseq_read: the next '>' or '@', wherever it stands
			size_t h = pos;
			while (h < fill && bp[h] != '>' && bp[h] != '@') ++h;
			if (h >= stop) { pos = h >= fill ? fill : h; break; } // (h == stop: the seam; h > stop: not a boundary, the caller sees it)
			P.begin = h, P.eof = false, P.last_char = 0;
			int64_t o[4];
			const long r = P.read_record(with_qual, with_comment, o);
			if (P.eof && !last_of_file) { pos = h; P.arena.resize(o[0] >= 0 && (size_t)o[0] <= P.arena.size() && r >= 0 ? (size_t)o[0] : P.arena.size()); break; } // cut off by the block end
			size_t e = P.begin;
			if (P.last_char) --e; // the next header character was consumed: hand it back
			if (r >= 0) C.off.insert(C.off.end(), o, o + 4), C.len.push_back((int32_t)r), C.err.push_back(0);
			else if (r < -1) { if (C.len.empty()) C.err_first = true; else C.err.back() = 1; }
			pos = e;
			if (r == -1 || e >= fill) { pos = std::min(e, fill); if (r == -1) pos = fill; break; }
		}
		P.arena.swap(C.arena);
		return pos;
	}
	// a position in (from, fill) that looks like the first byte of a four-line FASTQ record
	size_t find_seam(size_t from) const
	{
		const unsigned char *b = bp;
		for (size_t p = from; p < fill;) {
			const void *nl = memchr(b + p, '\n', fill - p);
			if (!nl) return fill;
			size_t q = (size_t)((const unsigned char *)nl - b) + 1; // start of a line
			if (q >= fill) return fill;
			if (b[q] == '@') {
				const void *e1 = memchr(b + q, '\n', fill - q);
				if (!e1) return fill;
				const size_t l2 = (size_t)((const unsigned char *)e1 - b) + 1;
				const void *e2 = l2 < fill ? memchr(b + l2, '\n', fill - l2) : nullptr;
				if (!e2) return fill;
				const size_t l3 = (size_t)((const unsigned char *)e2 - b) + 1;
				if (l3 < fill && b[l3] == '+') {
					const void *e3 = memchr(b + l3, '\n', fill - l3);
					if (!e3) return fill;
					const size_t l4 = (size_t)((const unsigned char *)e3 - b) + 1;
					const void *e4 = l4 < fill ? memchr(b + l4, '\n', fill - l4) : nullptr;
					if (e4 && (size_t)((const unsigned char *)e4 - b) - l4 == l3 - 1 - l2) return q;
				}
			}
			p = q;
		}
		return fill;
	}
	std::shared_ptr<GdFastxChunk> fresh_chunk()
	{
		std::shared_ptr<GdFastxChunk> c;
		{
			std::lock_guard<std::mutex> lk(pool_mu);
			if (!pool.empty()) c = std::move(pool.back()), pool.pop_back();
		}
		if (!c) c.reset(new GdFastxChunk());
		c->arena.clear(), c->off.clear(), c->len.clear(), c->err.clear(), c->err_first = false, c->next = 0, c->fail.clear();
		c->rec.clear(), c->dev.reset(), c->on_device = false, c->text = nullptr; // (buf keeps its memory for the next block it takes over)
		return c;
	}
	// Device mode: the strict prefix of the current block becomes a chunk that takes the block over; returns where the host parser starts
	size_t parse_on_device(std::vector<std::shared_ptr<GdFastxChunk>> &parts)
	{
		std::shared_ptr<GdFastxChunk> c = fresh_chunk();
		const long na = fill < ((size_t)1 << 31) ? dev->parse(bp, fill, c->rec, c->dev) : 0; // (the record table holds 32-bit offsets)
		if (na < 0) dev_error = true;
		if (na <= 0) {
			c->dev.reset();
			if (pool.size() < 64) pool.push_back(std::move(c));
			return 0;
		}
		unsigned char *w = const_cast<unsigned char *>(bp); // (the block is this reader's own buffer)
		c->off.resize(4 * (size_t)na), c->len.resize((size_t)na), c->err.assign((size_t)na, 0);
		for (long r = 0; r < na; ++r) {
			const GdxRec &R = c->rec[(size_t)r];
			int64_t *o = c->off.data() + 4 * r;
			o[0] = R.name_off, o[2] = R.seq_off;
			o[1] = with_comment && R.comment_off != GDX_NONE ? (int64_t)R.comment_off : -1;
			o[3] = with_qual ? (int64_t)R.qual_off : -1;
			c->len[(size_t)r] = (int32_t)R.seq_len;
			w[R.name_off + R.name_len] = 0;              // the delimiter behind the name, or the '\n' of the header line
			w[R.seq_off - 1] = 0;                        // the '\n' of the header line: the end of the comment
			w[R.seq_off + R.seq_len] = 0, w[R.qual_off + R.seq_len] = 0;
		}
		const GdxRec &L = c->rec[(size_t)na - 1];
		const size_t from = (size_t)L.qual_off + L.seq_len + 1;
		c->buf.swap(block); // (bp keeps pointing into it; `block` gets the buffer this chunk owned before, if any)
		c->home = bufpool;
		if (block.empty()) { // ... or one that a dead chunk sent back
			std::lock_guard<std::mutex> lk(bufpool->mu);
			if (!bufpool->bufs.empty()) block.swap(bufpool->bufs.back()), bufpool->bufs.pop_back();
		}
		c->text = (const char *)bp, c->on_device = true;
		n_rec_device += na;
		parts.push_back(std::move(c));
		return from;
	}
	// BAM: the records of the current block become one chunk; returns where the block's tail starts.  The walk is sequential and stays on
	// the host; the rows it yields are independent, so their text is written side by side: by the device (one D2H copy becomes the front
	// of the arena, and the device's copy stays with the chunk for the resident batch), or by n_threads host threads.  Names and comments
	// are the host's on both routes: they go behind the text.  The end of the file inside a record (or inside the header) is the
	// malformed record of the FASTQ grammar (GDIET_W_TRUNCATED); a record that contradicts itself ends the file with a read error.
	size_t parse_bam(std::vector<std::shared_ptr<GdFastxChunk>> &parts)
	{
		std::shared_ptr<GdFastxChunk> c = fresh_chunk();
		auto done = [&](size_t pos) {
			if (!c->fail.empty()) file_end = true, pos = fill; // nothing behind a malformed record is read
			parts.push_back(std::move(c));
			return pos;
		};
		if (fill >= ((size_t)1 << 31)) { c->fail = "BAM: a record, or the header, of 2 GiB or more"; return done(fill); } // (the tables hold 32-bit offsets)
		uint64_t from = 0;
		if (!bam_header_done) {
			const int h = gdi_header(bp, fill, &from, c->fail);
			if (h > 0) {
				if (file_end) c->err_first = true;
				return done(file_end ? fill : 0);
			}
			if (h < 0) return done(fill);
			bam_header_done = true;
		}
		GdiWalk W;
		gdi_walk(bp, (size_t)from, fill, with_qual, with_comment, bam_ordinal, bam_base, W);
		bam_ordinal += W.n_seen;
		const size_t n = W.rows.size(), nt = (size_t)std::max(1, n_threads);
		const bool on_dev = dev && !dev_error && n > 0 && W.text_len < ((uint64_t)1 << 32);
		if (n) {
			std::string &A = c->arena;
			A.resize((size_t)(W.text_len + W.names_len));
			if (on_dev) {
				std::string why;
				if (!gdi_rows_inside(W.rows.data(), n, fill, W.text_len)) why = "BAM: a table row outside its block";
				if (!why.empty() || dev->bam_unpack(bp, fill, W.rows.data(), n, W.text_len, &A[0], c->dev, why) < 0) {
					dev_error = true, io_msg = why, c->fail = why; // (nothing continues on the host for this file)
					c->dev.reset(), c->arena.clear();
					return done(fill);
				}
			}
			// ranges of rows for the threads: the text (host route), the names, and the comments, which each range collects for itself
			const size_t n_rng = std::min(n, nt * 4);
			std::vector<std::string> cm(with_comment ? n_rng : 0);
			std::vector<int64_t> cm_off(with_comment ? n : 0, -1);
			uint8_t *text = (uint8_t *)&A[0];
			bz_parallel(nt, n_rng, [&](size_t g, size_t) {
				for (size_t k = n * g / n_rng; k < n * (g + 1) / n_rng; ++k) {
					const GdiHostRow &H = W.host[k];
					if (!on_dev) gdi_unpack(W.rows[k], bp, text, 0, 1);
					memcpy(text + W.text_len + H.name_dst, bp + H.name_off, H.l_name);
					if (with_comment && H.aux_len) {
						cm_off[k] = (int64_t)cm[g].size();
						gdi_aux_text(bp + H.aux_off, H.aux_len, cm[g]);
						cm[g].push_back('\0');
					}
				}
			});
			c->off.resize(4 * n), c->len.resize(n), c->err.assign(n, 0);
			for (size_t g = 0; g < cm.size(); ++g) {
				for (size_t k = n * g / n_rng; k < n * (g + 1) / n_rng; ++k) if (cm_off[k] >= 0) cm_off[k] += (int64_t)A.size();
				A += cm[g];
			}
			for (size_t k = 0; k < n; ++k) {
				const GdiRow &R = W.rows[k];
				int64_t *o = c->off.data() + 4 * k;
				o[0] = (int64_t)(W.text_len + W.host[k].name_dst), o[1] = with_comment ? cm_off[k] : -1;
				o[2] = (int64_t)R.dst, o[3] = (R.flags & GDI_NOQUAL) ? -1 : (int64_t)(R.dst + R.l_seq + 1);
				c->len[k] = (int32_t)R.l_seq;
			}
			if (on_dev) c->text = A.data(), c->on_device = true, n_rec_device += (int64_t)n; // (the arena does not change any more)
			else n_rec_host += (int64_t)n;
		}
		if (W.bad) c->fail = W.msg;
		else if (file_end && W.pos < fill) { // the input ends inside a record
			if (n) c->err[n - 1] = 1; else c->err_first = true;
			W.pos = fill;
		}
		return done(W.pos);
	}
	// read and parse one more block; false when the input is exhausted
	bool parse_more()
	{
		// (device mode: the parser threads have nothing to do -- the device takes the strict prefix and the rest is parsed in sequence -- so a block is one thread's)
		size_t want = block_size * (size_t)(dev && !dev_error ? 1 : n_threads);
		for (;;) {
			if (!io_pending) { // the very first block: nothing was read ahead
				if (file_end) return false;
				if (block.size() < room_for(want)) block.resize(room_for(want));
				bool e, r;
				io_read(block.data(), want, &fill, &e, &r, dev && !dev_error);
				bp = block.data(), file_end = e, io_error = r;
				if (io_dev_err) dev_error = true;
			} else take_prefetched();
			if (fill == 0) return false;
			if (format < 0) { // the first bytes of the stream decide; fewer than four of them with more to come: read on
				const bool is_bam = fill >= 4 && !memcmp(bp, "BAM\1", 4);
				if (fill >= 4 || file_end || memcmp(bp, "BAM\1", fill)) format = is_bam ? 1 : 0;
			}
			std::vector<std::shared_ptr<GdFastxChunk>> parts;
			size_t pos = 0;
			if (format == 1) pos = parse_bam(parts);
			else if (format == 0) pos = parse_fastx(parts);
			++n_blocks;
			size_t n_rec = 0;
			for (auto &c : parts) if (c) {
				const bool any = !c->len.empty() || c->err_first || !c->fail.empty();
				n_rec += c->len.size() + (c->err_first ? 1 : 0) + (c->fail.empty() ? 0 : 1);
				if (any) ready.push_back(std::move(c)); else if (pool.size() < 64) pool.push_back(std::move(c));
			}
			// the unparsed tail (a record cut off by the block end) goes in front of the next stretch of the file, which is read while
			// the caller works on what was parsed
			if (file_end && pos >= fill) { fill = 0, io_pending = false; return n_rec > 0; }
			if (!n_rec && !file_end) want *= 2; // a record longer than the block: read on, in bigger steps
			if (!n_rec && file_end) { fill = 0, io_pending = false; return false; } // (only separators / a malformed rest were left)
			if (format == 1) bam_base += pos;
			prefetch(pos, want);
			if (n_rec) return true;
		}
	}
	// FASTA / FASTQ: the records of the current block as chunks in file order; returns where the block's tail starts
	size_t parse_fastx(std::vector<std::shared_ptr<GdFastxChunk>> &out)
	{
		// split points: record starts verified by look-ahead; whether they ARE boundaries of the sequential grammar is checked
		// afterwards (every stretch must end exactly where the next one began) -- if not, the rest is parsed again in sequence
		std::vector<size_t> cut(1, 0);
		std::vector<std::shared_ptr<GdFastxChunk>> dparts;
		if (dev && !dev_error) cut[0] = parse_on_device(dparts); // the rest goes through parse_range in sequence, as behind a wrong seam
		else if (n_threads > 1 && fill >= std::min<size_t>((size_t)1 << 20, block_size))
			for (int k = 1; k < n_threads; ++k) {
				const size_t c = find_seam(std::max(cut.back() + 1, fill / (size_t)n_threads * (size_t)k));
				if (c >= fill) break;
				cut.push_back(c);
			}
		const size_t nr = cut.size();
		std::vector<std::shared_ptr<GdFastxChunk>> parts(nr);
		std::vector<size_t> endpos(nr, 0);
		auto work = [&](size_t k) {
			parts[k] = fresh_chunk();
			endpos[k] = parse_range(*parts[k], cut[k], k + 1 < nr ? cut[k + 1] : fill, file_end);
		};
		if (nr > 1) {
			std::vector<std::thread> th;
			for (size_t k = 1; k < nr; ++k) th.emplace_back(work, k);
			work(0);
			for (auto &t : th) t.join();
		} else work(0);
		size_t good = 1; // stretches [0, good) are what a sequential parse would have produced
		while (good < nr && endpos[good - 1] == cut[good]) ++good;
		size_t pos = endpos[good - 1];
		if (getenv("GDIET_FASTX_TRACE")) fprintf(stderr, "[fastx] block %zu bytes, %zu stretches, %zu good, file_end %d\n", fill, nr, good, (int)file_end);
		if (good < nr) { // a seam was no boundary: everything after the last good stretch again, in sequence
			parts.resize(good + 1);
			parts[good] = fresh_chunk();
			pos = parse_range(*parts[good], endpos[good - 1], fill, file_end);
		}
		for (auto &c : parts) if (c) n_rec_host += (int64_t)c->len.size();
		if (!dparts.empty()) {
			for (auto &c : parts) if (c && (!c->len.empty() || c->err_first)) { ++n_blocks_handed; break; }
			parts.insert(parts.begin(), dparts.begin(), dparts.end());
		}
		out.swap(parts);
		return pos;
	}
	// U -> T in the host strings of the last batch's reads from device-parsed chunks (kseq2bseq, LR/bseq.c:71-73; read_record does it
	// for the host's own).  For a caller that takes no resident batch: the encode kernel flags the reads that need it otherwise.
	void u_to_t_on_host()
	{
		for (size_t i = 0; i < v_len.size() && n_rec_device; ++i)
			if (lent[(size_t)v_chunk[i]]->on_device) {
				char *q = const_cast<char *>(v_seq[i]);
				for (int32_t k = 0; k < v_len[i]; ++k) if (gdx_is_u((unsigned char)q[k])) --q[k];
			}
	}
	// mm_bseq_read3 (LR/bseq.c:80-121); returns the number of reads of the batch (0 at the end of the file), < 0 on a read error
	int read_batch(int64_t chunk_size, bool wq, bool wc, bool frag_mode, bool *parse_error)
	{
		if (!flags_set) with_qual = wq, with_comment = wc, flags_set = true; // (the flags of the first call hold for the whole file)
		for (auto &c : lent) if (c.use_count() == 1 && pool.size() < 64) pool.push_back(std::move(c)); // (not in `ready` any more, not detached)
		lent.clear();
		v_name.clear(), v_comment.clear(), v_seq.clear(), v_qual.clear(), v_len.clear(), v_chunk.clear(), v_rec.clear();
		if (parse_error) *parse_error = false;
		int64_t size = 0;
		bool closing = false; // the batch is full: only mates of its last read may still join (fragment mode)
		for (;;) {
			while (!ready.empty() && ready.front()->next >= ready.front()->len.size() && !ready.front()->err_first && ready.front()->fail.empty()) ready.pop_front();
			if (ready.empty() && !parse_more()) break;
			if (ready.empty()) continue;
			GdFastxChunk &C = *ready.front();
			if (C.err_first) { C.err_first = false; if (parse_error) *parse_error = true; break; } // the reference warns and returns what it has
			if (C.next >= C.len.size() && !C.fail.empty()) { // BAM: the malformed record is next: the reads in front of it go out first
				if (v_len.empty()) io_error = true, io_msg = C.fail;
				break;
			}
			if (C.next >= C.len.size()) continue;
			const size_t i = C.next;
			const char *const base = C.base();
			const char *nm = base + C.off[4 * i];
			if (closing) {
				const char *prev = v_name.back();
				const size_t l1 = qname_len(nm), l2 = qname_len(prev);
				if (!(l1 == l2 && strncmp(nm, prev, l1) == 0)) break;
			}
			if (lent.empty() || lent.back().get() != &C) lent.push_back(ready.front());
			v_name.push_back(nm);
			v_comment.push_back(C.off[4 * i + 1] < 0 ? nullptr : base + C.off[4 * i + 1]);
			v_seq.push_back(base + C.off[4 * i + 2]);
			v_qual.push_back(C.off[4 * i + 3] < 0 ? nullptr : base + C.off[4 * i + 3]);
			v_len.push_back(C.len[i]);
			v_chunk.push_back((int32_t)lent.size() - 1), v_rec.push_back((int32_t)i);
			size += C.len[i];
			++C.next;
			if (C.err[i]) { C.err[i] = 0; if (parse_error) *parse_error = true; break; }
			if (!closing && size >= chunk_size) {
				if (frag_mode && C.len[i] < 1000000) closing = true; // CHECK_PAIR_THRES
				else break;
			}
		}
		// (pointers into chunks still in `ready` stay valid: a chunk is only released from `lent`, at the next call)
		if (io_error || dev_error) return -1;
		return (int)v_len.size();
	}
};

// a batch taken out of the reader (several mini-batches in flight): owns the pointer arrays and keeps the chunks alive
struct GdFastxBatch {
	std::vector<std::shared_ptr<GdFastxChunk>> chunks;
	std::vector<const char *> v_name, v_comment, v_seq, v_qual;
	std::vector<int32_t> v_len;
};
static inline GdFastxBatch *gd_fastx_detach(GdFastx *fx)
{
	GdFastxBatch *b = new GdFastxBatch();
	b->chunks = fx->lent; // (shared: the reader may still hand out the rest of the last chunk)
	b->v_name.swap(fx->v_name), b->v_comment.swap(fx->v_comment), b->v_seq.swap(fx->v_seq), b->v_qual.swap(fx->v_qual), b->v_len.swap(fx->v_len);
	return b;
}

// WHEN A FILE TAKES THE BGZF ROUTE: it is a regular file, its first member is a BGZF member, its last 28 bytes are the BGZF end-of-file
// member, and GDIET_BGZF is not 0.  Everything else that starts with the gzip magic goes through gzread as before.
static inline bool gd_fastx_takes_bgzf_route(int fd)
{
	if (const char *e = getenv("GDIET_BGZF")) if (!strcmp(e, "0")) return false;
	struct stat st;
	if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < (off_t)(18 + GD_BGZF_EOF_LEN)) return false;
	unsigned char head[512], tail[GD_BGZF_EOF_LEN];
	const long nh = (long)::pread(fd, head, sizeof(head), 0);
	if (nh < 18 || !gd_bgzf_first_is_member(head, (size_t)nh)) return false;
	return ::pread(fd, tail, sizeof(tail), st.st_size - (off_t)GD_BGZF_EOF_LEN) == (long)sizeof(tail) && gd_bgzf_ends_with_marker(tail, sizeof(tail));
}

static inline GdFastx *gd_fastx_open(const char *path)
{
	GdFastx *fx = new GdFastx();
	if (const char *e = getenv("GDIET_FASTX_BLOCK")) fx->block_size = std::max<size_t>(256, (size_t)atol(e)); // (tests: many small blocks)
	if (path && strcmp(path, "-")) { // a plain file is read directly, anything that starts with the gzip magic through zlib
		const int fd = ::open(path, O_RDONLY);
		if (fd < 0) { delete fx; return nullptr; }
		unsigned char magic[2] = {0, 0};
		const long n = (long)::pread(fd, magic, 2, 0);
		if (n == 2 && magic[0] == 0x1f && magic[1] == 0x8b && gd_fastx_takes_bgzf_route(fd)) fx->fd = fd, fx->bgzf = true;
		else if (n == 2 && magic[0] == 0x1f && magic[1] == 0x8b) {
			::close(fd);
			fx->fp = gzopen(path, "r");
			if (!fx->fp) { delete fx; return nullptr; }
			gzbuffer(fx->fp, 1 << 20);
		} else fx->fd = fd;
	} else {
		fx->fp = gzdopen(0, "r"); // (LR/bseq.c:42)
		if (!fx->fp) { delete fx; return nullptr; }
	}
	return fx;
}

static inline void gd_fastx_close(GdFastx *fx)
{
	if (!fx) return;
	if (fx->io.joinable()) fx->io.join();
	if (fx->fp) gzclose(fx->fp);
	for (auto &z : fx->bz_zs) if (z.state) inflateEnd(&z);
	if (fx->fd >= 0) ::close(fx->fd);
	delete fx;
}
