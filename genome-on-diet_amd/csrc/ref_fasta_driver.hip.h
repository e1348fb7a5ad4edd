// Driver of the reference input (ref_fasta.hip.h); included by gdiet_hip.hip behind fastx_reader.h and map_pipeline.hip.h (needs
// gdiet_ctx, gdiet_index, GdFastx, gd_index_build_from_nt4, gd_index_upload).  Pieces:
//   GdRefDevice             GdRefExec on the device: a block of text -> its bases at d_nt4[base0 ..] and its header rows (classify, scan,
//                           count, scan, write); the bases the host grammar produced go to the same buffer
//   gd_ref_open_device      a file -> blocks as the reader reads them (inflated on its threads, the next one read while this one is parsed)
//                           -> d_nt4 and the sequence table -> ref_pack_kernel -> S -> gd_index_build_from_nt4
//   gd_ref_open_host        GDIET_INDEX_BUILD=host: the reader's records -> gd_index_build, all on the host
//   gdiet_hip_index_open / _index_info / _index_open_stats / _ref_block   the entry points (include/gdiet_hip.h, "Reference input")
// Everything runs on the context's stream, like gdiet_hip_index_build; the stream is synchronised before the host reads a table.
#pragma once
#include <hipcub/hipcub.hpp>
#include <sys/stat.h>
#include "ref_fasta.hip.h"

static double gd_ref_now()
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

struct GdRefDevice : GdRefExec {
	gdiet_ctx *ctx;
	hipStream_t s;
	uint8_t *d_blk = nullptr, *d_nt4 = nullptr, *d_tmp = nullptr;
	uint32_t *d_code = nullptr, *d_in = nullptr;
	GdrCnt *d_cnt = nullptr, *d_off = nullptr;
	GdrMeta *d_meta = nullptr;
	GdrHdr *d_rows = nullptr;
	size_t blk_cap = 0, tile_cap = 0, tmp_cap = 0, row_cap = 0;
	uint64_t nt4_cap = 0, nt4_used = 0; // nt4_used: bases placed so far (what a larger buffer must take over)
	uint64_t peak_bytes = 0, live_bytes = 0;
	explicit GdRefDevice(gdiet_ctx *c) : ctx(c), s(c->stream) {}
	GdRefDevice(const GdRefDevice &) = delete;
	GdRefDevice &operator=(const GdRefDevice &) = delete;
	~GdRefDevice()
	{
		(void)hipStreamSynchronize(s);
		void *p[] = {d_blk, d_nt4, d_tmp, d_code, d_in, d_cnt, d_off, d_meta, d_rows};
		for (void *q : p) if (q) (void)hipFree(q);
	}
	// p[0, cap) -> room for `need` items; the first `keep` items survive (allocation and copy on the stream, then the old buffer goes)
	template <class T, class N> hipError_t grow(T *&p, N &cap, uint64_t need, uint64_t keep, bool geometric)
	{
		if (need <= cap && p) return hipSuccess;
		uint64_t got = std::max<uint64_t>(std::max<uint64_t>(need, 1), geometric ? 2 * (uint64_t)cap : 0);
		T *q = nullptr;
		hipError_t e = hipMalloc((void **)&q, got * sizeof(T));
		if (e != hipSuccess && got > std::max<uint64_t>(need, 1)) { // no room to double: just enough
			(void)hipGetLastError();
			got = std::max<uint64_t>(need, 1), e = hipMalloc((void **)&q, got * sizeof(T));
		}
		if (e != hipSuccess) return e;
		live_bytes += got * sizeof(T), peak_bytes = std::max(peak_bytes, live_bytes);
		if (p && keep && (e = hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, s)) != hipSuccess) { (void)hipFree(q); return e; }
		if (p) {
			if ((e = hipStreamSynchronize(s)) != hipSuccess) { (void)hipFree(q); return e; }
			(void)hipFree(p), live_bytes -= (uint64_t)cap * sizeof(T);
		}
		p = q, cap = (N)got;
		return hipSuccess;
	}
	hipError_t room_for_bases(uint64_t upto) { return grow(d_nt4, nt4_cap, upto + 64, nt4_used, true); } // (+ 64: the pack pass reads whole words, the sketch a little past a contig)

	int fail(std::string &why, hipError_t e, const char *what)
	{
		(void)hipStreamSynchronize(s);
		(void)hipGetLastError();
		why = std::string("reference input: ") + what + ": " + hipGetErrorString(e);
		return -1;
	}
	int block(const uint8_t *text, uint32_t n, int state_in, uint64_t base0, GdrBlockOut &out, std::string &why) override
	{
		out = GdrBlockOut();
		out.state_out = state_in;
		if (n == 0) return 0;
		hipError_t e = hipSuccess;
		const uint32_t n_tiles = (n + GDX_TILE - 1) / GDX_TILE;
		if ((e = grow(d_blk, blk_cap, (uint64_t)n_tiles * GDX_TILE, 0, false)) != hipSuccess) return fail(why, e, "block");
		if (!d_meta) { size_t one = 0; if ((e = grow(d_meta, one, 1, 0, false)) != hipSuccess) return fail(why, e, "counts"); }
		if (tile_cap < (size_t)n_tiles + 1) {
			size_t c0 = d_code ? tile_cap : 0, c1 = c0, c2 = c0, c3 = c0;
			if ((e = grow(d_code, c0, (uint64_t)n_tiles + 1, 0, false)) != hipSuccess || (e = grow(d_in, c1, (uint64_t)n_tiles + 1, 0, false)) != hipSuccess ||
			    (e = grow(d_cnt, c2, (uint64_t)n_tiles + 1, 0, false)) != hipSuccess || (e = grow(d_off, c3, (uint64_t)n_tiles + 1, 0, false)) != hipSuccess)
				return fail(why, e, "counts");
			tile_cap = (size_t)n_tiles + 1;
		}
		size_t b1 = 0, b2 = 0;
		const uint32_t seed = state_in == GDR_HD ? (uint32_t)GDR_HD : (uint32_t)GDR_SQ; // (GDR_LS: byte 0 starts a line, the seed is never read)
		const GdrCnt zero = {0, 0, 0, 0};
		if ((e = hipcub::DeviceScan::ExclusiveScan(nullptr, b1, d_code, d_in, GdrTakeLast(), seed, (int)n_tiles, s)) != hipSuccess) return fail(why, e, "scan");
		if ((e = hipcub::DeviceScan::ExclusiveScan(nullptr, b2, d_cnt, d_off, GdrCntSum(), zero, (int)(n_tiles + 1), s)) != hipSuccess) return fail(why, e, "scan");
		if ((e = grow(d_tmp, tmp_cap, std::max(b1, b2) + 64, 0, true)) != hipSuccess) return fail(why, e, "scan buffer");
		if ((e = hipMemcpyAsync(d_blk, text, n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(why, e, "block copy");
		if ((e = hipMemsetAsync(&d_meta->bad, 0, sizeof(uint32_t), s)) != hipSuccess) return fail(why, e, "counts");
		if ((e = hipMemsetAsync(&d_meta->run_nl, 0xff, sizeof(uint32_t), s)) != hipSuccess) return fail(why, e, "counts");
		if ((e = hipMemsetAsync(d_cnt + n_tiles, 0, sizeof(GdrCnt), s)) != hipSuccess) return fail(why, e, "counts");
		hipLaunchKernelGGL(ref_classify_kernel, dim3(n_tiles), dim3(64), 0, s, (const uint8_t *)d_blk, n, state_in, d_code, d_meta);
		b1 = tmp_cap;
		if ((e = hipcub::DeviceScan::ExclusiveScan(d_tmp, b1, d_code, d_in, GdrTakeLast(), seed, (int)n_tiles, s)) != hipSuccess) return fail(why, e, "scan");
		hipLaunchKernelGGL(ref_count_kernel, dim3(n_tiles), dim3(64), 0, s, (const uint8_t *)d_blk, n, state_in, (const uint32_t *)d_in, d_cnt);
		b2 = tmp_cap;
		if ((e = hipcub::DeviceScan::ExclusiveScan(d_tmp, b2, d_cnt, d_off, GdrCntSum(), zero, (int)(n_tiles + 1), s)) != hipSuccess) return fail(why, e, "scan");
		GdrCnt tot = zero;
		GdrMeta meta = {1, GDX_NONE};
		if ((e = hipMemcpyAsync(&tot, d_off + n_tiles, sizeof(GdrCnt), hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(why, e, "counts");
		if ((e = hipMemcpyAsync(&meta, d_meta, sizeof(GdrMeta), hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(why, e, "counts");
		if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(why, e, "count pass");
		if ((e = hipGetLastError()) != hipSuccess) return fail(why, e, "kernels");
		if (meta.bad) return 0; // not claimed
		const uint32_t hd_in = state_in == GDR_HD ? 1u : 0u;
		if (tot.bases > n || tot.hstart > n || tot.hend > tot.hstart + hd_in) return fail(why, hipErrorInvalidValue, "counts that contradict the block");
		if ((e = room_for_bases(base0 + tot.bases)) != hipSuccess) return fail(why, e, "bases");
		if ((e = grow(d_rows, row_cap, tot.hstart, 0, true)) != hipSuccess) return fail(why, e, "header rows");
		if (tot.hstart && (e = hipMemsetAsync(d_rows, 0xff, sizeof(GdrHdr) * (size_t)tot.hstart, s)) != hipSuccess) return fail(why, e, "header rows");
		hipLaunchKernelGGL(ref_write_kernel, dim3(n_tiles), dim3(64), 0, s, (const uint8_t *)d_blk, n, state_in, (const uint32_t *)d_in, (const GdrCnt *)d_off, d_nt4, base0,
		                   (uint64_t)nt4_cap, d_rows, (uint32_t)std::min<size_t>(row_cap, 0xffffffffu), d_meta);
		out.rows.resize(tot.hstart);
		if (tot.hstart && (e = hipMemcpyAsync(out.rows.data(), d_rows, sizeof(GdrHdr) * (size_t)tot.hstart, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(why, e, "header rows");
		if ((e = hipMemcpyAsync(&meta, d_meta, sizeof(GdrMeta), hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(why, e, "header rows");
		if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(why, e, "write pass");
		if ((e = hipGetLastError()) != hipSuccess) return fail(why, e, "kernels");
		// every offset the host is going to use lies inside the block (the table came over a bus)
		for (size_t r = 0; r < out.rows.size(); ++r) {
			const GdrHdr &H = out.rows[r];
			const bool open = H.nl_off == GDX_NONE;
			if (H.gt_off >= n || text[H.gt_off] != '>' || H.base_rank > tot.bases || (!open && (H.nl_off <= H.gt_off || H.nl_off >= n)) || (open && r + 1 != out.rows.size()) ||
			    (r && (H.gt_off <= out.rows[r - 1].nl_off || H.base_rank < out.rows[r - 1].base_rank)))
				return fail(why, hipErrorInvalidValue, "a header row outside its block");
		}
		if (meta.run_nl != GDX_NONE && (!hd_in || meta.run_nl >= n)) return fail(why, hipErrorInvalidValue, "a header end outside its block");
		nt4_used = std::max(nt4_used, base0 + tot.bases);
		out.claimed = n, out.bases = tot.bases, out.run_nl = meta.run_nl;
		out.state_out = gdr_state_out(text, n, state_in, tot.hstart, tot.hend);
		return 0;
	}
	int store(uint64_t at, const uint8_t *nt4, size_t n, std::string &why) override
	{
		hipError_t e = hipSuccess;
		nt4_used = std::min(nt4_used, at); // (bases behind `at` were taken back)
		if ((e = room_for_bases(at + n)) != hipSuccess) return fail(why, e, "bases");
		if (n && (e = hipMemcpyAsync(d_nt4 + at, nt4, n, hipMemcpyHostToDevice, s)) != hipSuccess) return fail(why, e, "bases of the host grammar");
		if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(why, e, "bases of the host grammar");
		nt4_used = at + n;
		return 0;
	}
};

// names and lengths from the grammar's table; false with the text of the limit that was exceeded
static bool gd_ref_table(const GdRefGrammar &G, GdIndex &I, std::string &err)
{
	const size_t n = G.names.size();
	I.seq.resize(n);
	for (size_t i = 0; i < n; ++i) {
		const uint64_t len = (i + 1 < n ? G.start[i + 1] : G.rank) - G.start[i];
		if (len > 0xffffffffull) { err = "sequence " + G.names[i] + " is longer than 2^32 - 1 bases"; return false; }
		I.seq[i].name = G.names[i], I.seq[i].offset = G.start[i], I.seq[i].len = (uint32_t)len;
	}
	return true;
}

static int gd_ref_open_device(gdiet_ctx *ctx, gdiet_index *ix, GdFastx *fx, const char *path, int k, int w, const GdPattern &P, GdRefStats &S, uint64_t *peak)
{
	GdRefDevice X(ctx);
	GdRefGrammar G;
	std::string why;
	struct stat sb;
	const bool plain = fx->fd >= 0 && !fx->bgzf && fstat(fx->fd, &sb) == 0 && S_ISREG(sb.st_mode);
	if (plain && sb.st_size > 0) { // a plain file has at most one base per byte: one allocation
		const hipError_t e = X.room_for_bases((uint64_t)sb.st_size);
		if (e != hipSuccess) { (void)hipGetLastError(); ctx->err = std::string("reference input: bases: ") + hipGetErrorString(e); return GDIET_E_NOMEM; }
	}
	const size_t want = fx->block_size;
	std::vector<unsigned char> buf[2];
	buf[0].resize(fx->room_for(want)), buf[1].resize(fx->room_for(want));
	size_t got[2] = {0, 0};
	bool eof = false, err = false, first = true;
	double t_io = 0;
	auto read_into = [&](int b) { const double t0 = gd_ref_now(); fx->io_read(buf[b].data(), want, &got[b], &eof, &err, false); t_io += gd_ref_now() - t0; };
	read_into(0);
	for (int cur = 0; !err && got[cur] > 0; cur ^= 1) {
		std::thread io;
		const bool more = !eof;
		if (more) io = std::thread(read_into, cur ^ 1); // the next block is read (and inflated) while this one is parsed
		else got[cur ^ 1] = 0;
		int rc = gd_ref_one_block(G, X, S, buf[cur].data(), got[cur], first, gd_ref_now, why);
		if (rc == 0) { const double t0 = gd_ref_now(); rc = gd_ref_flush(G, X, why); S.s_host += gd_ref_now() - t0; }
		first = false;
		if (io.joinable()) io.join();
		if (rc < 0) { ctx->err = why; return GDIET_E_HIP; }
	}
	if (err) { ctx->err = std::string("read error on ") + path + (fx->io_msg.empty() ? "" : ": " + fx->io_msg); return GDIET_E_PARAM; }
	G.finish();
	// (seconds on the reading thread: a BGZF file reports its raw reads and its inflate apart; a gzip stream inflates inside its read)
	if (fx->bgzf) S.s_read = 1e-9 * (double)fx->bz_ns[0], S.s_inflate = 1e-9 * (double)(fx->bz_ns[1] + fx->bz_ns[2]);
	else if (fx->fp) S.s_inflate = t_io;
	else S.s_read = t_io;
	if (G.names.empty()) { ctx->err = std::string(path) + ": no sequence"; return GDIET_E_PARAM; }
	const double t0 = gd_ref_now();
	GdIndex &I = ix->h;
	if (!gd_ref_table(G, I, ctx->err)) return GDIET_E_PARAM;
	const uint64_t sum = G.rank, n_words = (sum + 7) / 8;
	hipError_t e = hipSuccess;
	hipStream_t s = ctx->stream;
	X.nt4_used = std::min(X.nt4_used, sum);
	if ((e = X.room_for_bases(8 * n_words)) != hipSuccess) { (void)hipGetLastError(); ctx->err = std::string("reference input: bases: ") + hipGetErrorString(e); return GDIET_E_NOMEM; }
	GD_HIP(hipMemsetAsync(X.d_nt4 + sum, 0, (size_t)(8 * n_words + 64 - sum), s)); // behind the last base: what idx_unpack_kernel leaves of an S word's unused nibbles
	GdDevTmp T;
	uint32_t *d_S = nullptr;
	if ((e = T.alloc(&d_S, n_words + 2)) != hipSuccess) { (void)hipGetLastError(); ctx->err = std::string("reference input: S: ") + hipGetErrorString(e); return GDIET_E_NOMEM; }
	if (n_words) hipLaunchKernelGGL(ref_pack_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, s, (const uint64_t *)X.d_nt4, d_S, n_words, sum);
	I.S.resize(n_words);
	if (n_words) GD_HIP(hipMemcpyAsync(I.S.data(), d_S, n_words * 4, hipMemcpyDeviceToHost, s));
	GD_HIP(hipStreamSynchronize(s));
	*peak = X.peak_bytes + (n_words + 2) * 4;
	if (!gd_index_build_from_nt4(ix, T, d_S, (const uint64_t *)X.d_nt4, k, w, P, s, ctx->err)) return GDIET_E_HIP;
	S.s_build = gd_ref_now() - t0;
	return GDIET_OK;
}

// GDIET_INDEX_BUILD=host: the reader's own records, the host builder, one upload
static int gd_ref_open_host(gdiet_ctx *ctx, gdiet_index *ix, GdFastx *fx, const char *path, int k, int w, const GdPattern &P, int nt, GdRefStats &S)
{
	std::vector<std::string> names, seqs;
	const double t0 = gd_ref_now();
	for (;;) {
		bool bad = false;
		const int n = fx->read_batch((int64_t)1 << 28, false, false, false, &bad);
		if (n < 0) { ctx->err = std::string("read error on ") + path + (fx->io_msg.empty() ? "" : ": " + fx->io_msg); return GDIET_E_PARAM; }
		for (int i = 0; i < n; ++i) names.emplace_back(fx->v_name[(size_t)i]), seqs.emplace_back(fx->v_seq[(size_t)i], (size_t)fx->v_len[(size_t)i]);
		if (n == 0 && !bad) break;
	}
	S.blocks = S.blocks_host = fx->n_blocks;
	for (const std::string &q : seqs) S.bases_host += (int64_t)q.size();
	S.s_host = gd_ref_now() - t0;
	if (fx->bgzf) S.s_read = 1e-9 * (double)fx->bz_ns[0], S.s_inflate = 1e-9 * (double)(fx->bz_ns[1] + fx->bz_ns[2]), S.text_bytes = fx->bz_bytes_out;
	if (names.empty()) { ctx->err = std::string(path) + ": no sequence"; return GDIET_E_PARAM; }
	const double t1 = gd_ref_now();
	std::vector<GdSeqSpan> sq(seqs.size());
	for (size_t i = 0; i < seqs.size(); ++i) sq[i].p = seqs[i].data(), sq[i].n = seqs[i].size();
	gd_index_build(ix->h, names, sq, k, w, P, nt, true);
	const int rc = gd_index_upload(ctx, ix);
	S.s_build = gd_ref_now() - t1;
	return rc;
}

extern "C" int gdiet_hip_index_open(gdiet_ctx *ctx, gdiet_index **out, const char *path, int k, int w, const char *pattern, int pattern_len, int n_threads)
{
	if (!ctx || !out || !path) return GDIET_E_PARAM;
	*out = nullptr;
	gd_err_clear();
	(void)hipSetDevice(ctx->device);
	GdPattern P;
	if (!gd_pattern_init(P, pattern, pattern_len)) { ctx->err = "bad pattern"; return GDIET_E_PARAM; }
	// an index file is known by its magic (mm_idx_is_idx, LR/index.c:573-593): a regular file of four bytes or more that starts with "MMI\2"
	bool is_mmi = false;
	struct stat sb;
	memset(&sb, 0, sizeof(sb));
	if (strcmp(path, "-")) {
		const int fd = ::open(path, O_RDONLY);
		if (fd < 0) { ctx->err = std::string("cannot open ") + path + ": " + strerror(errno); return GDIET_E_PARAM; }
		char magic[4];
		is_mmi = fstat(fd, &sb) == 0 && sb.st_size >= 4 && ::pread(fd, magic, 4, 0) == 4 && !memcmp(magic, "MMI\2", 4);
		::close(fd);
	}
	GdRefStats S;
	S.file_bytes = (int64_t)sb.st_size;
	uint64_t peak = 0;
	int rc = GDIET_OK;
	gdiet_index *ix = nullptr;
	if (is_mmi) { // k and w are the file's (the reference overrides the command line's with a warning, LR/main.c)
		const double t0 = gd_ref_now();
		if ((rc = gdiet_hip_index_load_mmi(ctx, &ix, path, pattern, pattern_len))) return rc;
		S.text_bytes = S.file_bytes, S.s_build = gd_ref_now() - t0;
	} else {
		if (w <= 0 || w > GDM_MAX_W || k <= 0 || k > 28) { ctx->err = "k must be in [1,28] and w in [1,64]"; return GDIET_E_PARAM; }
		GdFastx *fx = gd_fastx_open(path);
		if (!fx) { ctx->err = std::string("cannot open ") + path; return GDIET_E_PARAM; }
		const int nt = n_threads > 0 ? n_threads : gd_effective_cpus();
		fx->n_threads = std::min(nt, 64);
		ix = new gdiet_index();
		rc = ctx->index_on_device ? gd_ref_open_device(ctx, ix, fx, path, k, w, P, S, &peak) : gd_ref_open_host(ctx, ix, fx, path, k, w, P, nt, S);
		gd_fastx_close(fx);
		if (rc) { gdiet_hip_index_destroy(ctx, ix); return rc; }
	}
	const int64_t c[6] = {S.file_bytes, S.text_bytes, S.blocks, S.blocks_host, S.bases_device, S.bases_host};
	const double t[5] = {S.s_read, S.s_inflate, S.s_device, S.s_host, S.s_build};
	memcpy(ix->open_counts, c, sizeof(c)), memcpy(ix->open_seconds, t, sizeof(t)), ix->open_peak = peak;
	*out = ix;
	return GDIET_OK;
}

extern "C" int gdiet_hip_index_info(const gdiet_index *ix, int *k, int *w, int *n_seq, const char *const **names, const uint32_t **lens)
{
	if (!ix) return GDIET_E_PARAM;
	const GdIndex &h = ix->h;
	if (k) *k = h.k;
	if (w) *w = h.w;
	if (n_seq) *n_seq = (int)h.seq.size();
	if (names || lens) { // the arrays are made on first use and live with the index
		gdiet_index *m = const_cast<gdiet_index *>(ix);
		std::lock_guard<std::mutex> lk(m->seq_mu);
		if (m->info_lens.size() != h.seq.size() || m->info_names.size() != h.seq.size()) {
			m->info_names.resize(h.seq.size()), m->info_lens.resize(h.seq.size());
			for (size_t i = 0; i < h.seq.size(); ++i) m->info_names[i] = h.seq[i].name.c_str(), m->info_lens[i] = h.seq[i].len;
		}
		if (names) *names = m->info_names.data();
		if (lens) *lens = m->info_lens.data();
	}
	return GDIET_OK;
}

extern "C" int gdiet_hip_index_open_stats(const gdiet_index *ix, int64_t *counts6, double *seconds5, uint64_t *device_peak_bytes)
{
	if (!ix) return GDIET_E_PARAM;
	if (counts6) memcpy(counts6, ix->open_counts, sizeof(ix->open_counts));
	if (seconds5) memcpy(seconds5, ix->open_seconds, sizeof(ix->open_seconds));
	if (device_peak_bytes) *device_peak_bytes = ix->open_peak;
	return GDIET_OK;
}

extern "C" int gdiet_hip_ref_block(gdiet_ctx *ctx, const char *text, size_t n, int state_in, uint8_t *nt4, size_t nt4_cap, size_t *n_bases, uint32_t *rows, size_t row_cap, size_t *n_rows,
                                   size_t *claimed, int *state_out, uint32_t *run_nl)
{
	if (!ctx || (!text && n) || state_in < GDR_LS || state_in > GDR_SQ || n >= ((size_t)1 << 31)) return GDIET_E_PARAM;
	gd_err_clear();
	(void)hipSetDevice(ctx->device);
	GdRefDevice X(ctx);
	GdrBlockOut O;
	std::string why;
	if (X.block((const uint8_t *)text, (uint32_t)n, state_in, 0, O, why) < 0) { ctx->err = why; return GDIET_E_HIP; }
	if (claimed) *claimed = O.claimed;
	if (state_out) *state_out = O.claimed == n ? O.state_out : -1;
	if (run_nl) *run_nl = O.run_nl;
	if (n_bases) *n_bases = O.bases;
	if (n_rows) *n_rows = O.rows.size();
	if (nt4 && O.bases) {
		if (nt4_cap < O.bases) { ctx->err = "gdiet_hip_ref_block: room for " + std::to_string(O.bases) + " bases is needed"; return GDIET_E_PARAM; }
		GD_HIP(hipMemcpy(nt4, X.d_nt4, O.bases, hipMemcpyDeviceToHost));
	}
	if (rows && !O.rows.empty()) {
		if (row_cap < O.rows.size()) { ctx->err = "gdiet_hip_ref_block: room for " + std::to_string(O.rows.size()) + " header rows is needed"; return GDIET_E_PARAM; }
		memcpy(rows, O.rows.data(), sizeof(GdrHdr) * O.rows.size());
	}
	return GDIET_OK;
}
