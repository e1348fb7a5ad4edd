// CPU emulator of the reference input's device stage (csrc/ref_fasta.h: the statements of the kernels in csrc/ref_fasta.hip.h as host
// loops), built with -fsanitize=address,undefined by tests/test_ref_fasta.py.
//
//     ref_fasta_emul files FILE...        every file at block sizes 256, 1024, 4096 and one block for the whole file
//     ref_fasta_emul blocks CASES         the kernel-level boundary: CASES holds {u32 n, u32 state_in, n bytes} back to back
//     ref_fasta_emul mmi FILE K W Z OUT   the host route on the CPU: the reader's records -> gd_index_build -> the .mmi file (bucket bits 14)
//
// The executor runs the three passes of a block as loops over the tiles and, inside a tile, over the lanes -- 0..63 and again 63..0:
// the results must not depend on the order -- with the block in whole tiles whose bytes past the end are hostile, and the bases and the
// header rows in buffers of exactly the counted size.  `files` reads each file through the library's reader (gd_fastx_open, io_read: plain,
// gzip, BGZF) and runs the driver's own loop (gd_ref_one_block) on its blocks.  Checked, per file and block size:
//   * after every block, the grammar that took the device's results stands exactly where a second grammar stands that read every byte
//     itself (state, bases, records, the name so far): the claimed prefix and the end state fit the next block's start;
//   * at the end, names, lengths and the concatenated bases are those of read_record (fastx_reader.h) on the whole text;
//   * S packed by the pack pass's statement equals gd_index_pack_S of the same sequences.
// Prints one line per file and block size: "ok FILE block B blocks N handed H device D host K seqs S"; any difference ends the program
// with status 1.  `blocks` prints one line per case: "claimed C state S run_nl R bases <hex> rows <gt:nl:rank,...>".
#include "fastx_reader.h"
#include "map_index.h"
#include "ref_fasta.h"
#include <stdio.h>

static void die(const char *what, const char *file, size_t block, size_t at)
{
	printf("MISMATCH %s (%s, block size %zu, at %zu)\n", what, file, block, at);
	exit(1);
}

struct EmulExec : GdRefExec {
	std::vector<uint8_t> nt4; // every base placed so far
	const char *file = "";
	size_t block_size = 0;

	struct Pass { bool bad; GdrCnt tot; GdrMeta meta; std::vector<uint8_t> bases; std::vector<GdrHdr> rows; };
	Pass run(const uint8_t *text, uint32_t n, int state_in, bool reverse)
	{
		const uint32_t n_tiles = (n + GDX_TILE - 1) / GDX_TILE;
		std::vector<uint8_t> blk((size_t)n_tiles * GDX_TILE);
		for (size_t i = 0; i < blk.size(); ++i) blk[i] = (uint8_t)"\n>\r+@"[i % 5]; // what the allocation holds behind the block: hostile
		memcpy(blk.data(), text, n);
		auto lane_at = [&](uint32_t t, uint32_t l) { return t * GDX_TILE + l * GDX_LANE_BYTES; };
		auto load = [&](uint32_t at, uint32_t w[4], uint32_t &valid) {
			memcpy(w, blk.data() + at, 16);
			valid = gdx_valid16(at, n);
			return gdr_lane_masks(w, valid, gdr_prev_nl(blk.data(), at, n, state_in));
		};
		Pass P;
		P.bad = false, P.meta.bad = 0, P.meta.run_nl = GDX_NONE;
		// classify
		std::vector<uint32_t> code(n_tiles), tin(n_tiles);
		std::vector<uint64_t> has(n_tiles, 0), ishdr(n_tiles, 0);
		for (uint32_t t = 0; t < n_tiles; ++t) {
			for (uint32_t q = 0; q < 64; ++q) {
				const uint32_t l = reverse ? 63 - q : q;
				uint32_t w[4], valid;
				const GdrLane L = load(lane_at(t, l), w, valid);
				const uint32_t c = gdr_lane_code(L);
				if (c) has[t] |= 1ull << l;
				if (c == GDR_HD) ishdr[t] |= 1ull << l;
				if (L.bad) P.bad = true;
			}
			code[t] = gdr_tile_code(has[t], ishdr[t]);
		}
		uint32_t run = state_in == GDR_HD ? (uint32_t)GDR_HD : (uint32_t)GDR_SQ;
		for (uint32_t t = 0; t < n_tiles; ++t) tin[t] = run, run = gdr_take_last(run, code[t]);
		P.tot = GdrCnt{0, 0, 0, 0};
		if (P.bad) return P;
		// count
		std::vector<GdrCnt> cnt(n_tiles), off(n_tiles + 1);
		for (uint32_t t = 0; t < n_tiles; ++t) {
			cnt[t] = GdrCnt{0, 0, 0, 0};
			for (uint32_t q = 0; q < 64; ++q) {
				const uint32_t l = reverse ? 63 - q : q;
				uint32_t w[4], valid, bases, hend;
				const GdrLane L = load(lane_at(t, l), w, valid);
				gdr_lane_split(L, valid, gdr_class_in(has[t], ishdr[t], l, tin[t]), bases, hend);
				cnt[t].bases += (uint32_t)__builtin_popcount(bases), cnt[t].hstart += (uint32_t)__builtin_popcount(L.hdr), cnt[t].hend += (uint32_t)__builtin_popcount(hend);
			}
		}
		off[0] = GdrCnt{0, 0, 0, 0};
		for (uint32_t t = 0; t < n_tiles; ++t) off[t + 1] = GdrCnt{off[t].bases + cnt[t].bases, off[t].hstart + cnt[t].hstart, off[t].hend + cnt[t].hend, 0};
		P.tot = off[n_tiles];
		// write: buffers of exactly the counted size
		P.bases.assign(P.tot.bases, 0xee);
		P.rows.assign(P.tot.hstart, GdrHdr{GDX_NONE, GDX_NONE, GDX_NONE});
		const uint32_t hd_in = state_in == GDR_HD ? 1u : 0u;
		for (uint32_t t = 0; t < n_tiles; ++t) {
			uint32_t lb[64], ls[64], le[64], msk_b[64], msk_e[64];
			GdrLane LL[64];
			uint32_t ww[64][4];
			for (uint32_t l = 0; l < 64; ++l) {
				uint32_t valid;
				LL[l] = load(lane_at(t, l), ww[l], valid);
				gdr_lane_split(LL[l], valid, gdr_class_in(has[t], ishdr[t], l, tin[t]), msk_b[l], msk_e[l]);
				lb[l] = (uint32_t)__builtin_popcount(msk_b[l]), ls[l] = (uint32_t)__builtin_popcount(LL[l].hdr), le[l] = (uint32_t)__builtin_popcount(msk_e[l]);
			}
			uint32_t xb[64], xs[64], xe[64], a = 0, b = 0, c = 0; // the lanes' exclusive scan
			for (uint32_t l = 0; l < 64; ++l) xb[l] = a, xs[l] = b, xe[l] = c, a += lb[l], b += ls[l], c += le[l];
			for (uint32_t q = 0; q < 64; ++q) {
				const uint32_t l = reverse ? 63 - q : q;
				gdr_lane_write(LL[l], msk_b[l], msk_e[l], ww[l], lane_at(t, l), off[t].bases + xb[l], off[t].hstart + xs[l], off[t].hend + xe[l], hd_in, P.bases.data(), 0,
				               P.bases.size(), P.rows.data(), (uint32_t)P.rows.size(), &P.meta);
			}
		}
		return P;
	}
	int block(const uint8_t *text, uint32_t n, int state_in, uint64_t base0, GdrBlockOut &out, std::string &) override
	{
		out = GdrBlockOut();
		out.state_out = state_in;
		if (n == 0) return 0;
		Pass A = run(text, n, state_in, false), B = run(text, n, state_in, true);
		if (A.bad != B.bad || A.bases != B.bases || A.rows.size() != B.rows.size() || A.meta.run_nl != B.meta.run_nl ||
		    (A.rows.size() && memcmp(A.rows.data(), B.rows.data(), sizeof(GdrHdr) * A.rows.size())))
			die("the order of the lanes changes the result", file, block_size, (size_t)base0);
		if (A.bad) return 0;
		for (uint8_t c : A.bases) if (c > 4) die("a base nobody wrote", file, block_size, (size_t)base0);
		if (nt4.size() < base0) die("bases placed behind a gap", file, block_size, (size_t)base0);
		nt4.resize((size_t)base0);
		nt4.insert(nt4.end(), A.bases.begin(), A.bases.end());
		out.claimed = n, out.bases = A.tot.bases, out.run_nl = A.meta.run_nl, out.rows = A.rows;
		out.state_out = gdr_state_out(text, n, state_in, A.tot.hstart, A.tot.hend);
		return 0;
	}
	int store(uint64_t at, const uint8_t *p, size_t n, std::string &) override
	{
		if (nt4.size() < at) die("host bases placed behind a gap", file, block_size, (size_t)at);
		nt4.resize((size_t)at);
		nt4.insert(nt4.end(), p, p + n);
		return 0;
	}
};

static double no_clock() { return 0; }

static bool same_place(const GdRefGrammar &A, const GdRefGrammar &B)
{
	if (A.st != B.st || A.rank != B.rank || A.names != B.names || A.start != B.start) return false;
	if (A.st == GdRefGrammar::NAME && (A.hdr_bytes == 0) != (B.hdr_bytes == 0)) return false;
	return true;
}

static void one_file(const char *path, size_t block)
{
	GdFastx *fx = gd_fastx_open(path);
	if (!fx) die("cannot open", path, block, 0);
	fx->n_threads = 2;
	EmulExec X;
	X.file = path, X.block_size = block;
	GdRefGrammar G, H; // H reads every byte itself
	GdRefStats S;
	std::string whole, why;
	std::vector<unsigned char> buf(fx->room_for(block));
	bool eof = false, err = false, first = true;
	for (;;) {
		size_t got = 0;
		fx->io_read(buf.data(), block, &got, &eof, &err, false);
		if (err) die("read error", path, block, whole.size());
		if (got) {
			std::vector<unsigned char> exact(buf.begin(), buf.begin() + got); // (the block in a buffer of its own size: a read past it is an error)
			whole.append((const char *)exact.data(), got);
			if (gd_ref_one_block(G, X, S, exact.data(), got, first, no_clock, why) < 0 || gd_ref_flush(G, X, why) < 0) die("executor failed", path, block, whole.size());
			H.feed(exact.data(), got), H.hb.clear();
			if (!same_place(G, H)) die("the device's block leaves the grammar somewhere else than its own bytes do", path, block, whole.size());
			first = false;
		}
		if (eof || !got) break;
	}
	gd_fastx_close(fx);
	G.finish(), H.finish();
	if (!same_place(G, H)) die("the end of the file", path, block, whole.size());
	// the sequential grammar on the whole text
	GdFastxParser P;
	P.b = (const unsigned char *)whole.data(), P.begin = 0, P.end = whole.size();
	std::vector<std::string> names, seqs;
	for (;;) {
		int64_t o[4];
		const long r = P.read_record(false, false, o);
		if (r == -1) break;
		if (r < 0) continue; // a malformed record is not returned; the scan goes on behind it
		names.emplace_back(P.arena.data() + o[0]), seqs.emplace_back(P.arena.data() + o[2], (size_t)r);
	}
	if (names != G.names) die("names", path, block, names.size());
	uint64_t at = 0;
	for (size_t i = 0; i < seqs.size(); ++i) {
		if (G.start[i] != at) die("contig start", path, block, i);
		if (X.nt4.size() < at + seqs[i].size()) die("bases missing", path, block, i);
		for (size_t j = 0; j < seqs[i].size(); ++j)
			if (X.nt4[(size_t)at + j] != gd_nt4((unsigned char)seqs[i][j])) die("base", path, block, (size_t)at + j);
		at += seqs[i].size();
	}
	if (G.rank != at) die("total bases", path, block, (size_t)at);
	// S
	GdIndex I;
	std::vector<GdSeqSpan> sp(seqs.size());
	for (size_t i = 0; i < seqs.size(); ++i) sp[i].p = seqs[i].data(), sp[i].n = seqs[i].size();
	gd_index_pack_S(I, names, sp, 2);
	const uint64_t n_words = (at + 7) / 8;
	std::vector<uint8_t> padded(X.nt4.begin(), X.nt4.begin() + (size_t)at);
	padded.resize((size_t)(8 * n_words), 0xab); // (what lies behind the last base must not matter)
	if (I.S.size() != n_words) die("S size", path, block, 0);
	for (uint64_t i = 0; i < n_words; ++i) {
		uint64_t b8;
		memcpy(&b8, padded.data() + 8 * i, 8);
		if (gdr_pack_word(b8, i, at) != I.S[(size_t)i]) die("S word", path, block, (size_t)i);
	}
	printf("ok %s block %zu blocks %lld handed %lld device %lld host %lld seqs %zu\n", path, block, (long long)S.blocks, (long long)S.blocks_host, (long long)S.bases_device,
	       (long long)S.bases_host, names.size());
}

static int run_blocks(const char *path)
{
	FILE *fp = fopen(path, "rb");
	if (!fp) return 2;
	uint32_t h[2];
	while (fread(h, 4, 2, fp) == 2) {
		std::vector<uint8_t> text(h[0]);
		if (h[0] && fread(text.data(), 1, h[0], fp) != h[0]) return 2;
		EmulExec X;
		GdrBlockOut O;
		std::string why;
		X.block(text.data(), h[0], (int)h[1], 0, O, why);
		printf("claimed %u state %d run_nl %u bases ", O.claimed, O.claimed == h[0] ? O.state_out : -1, O.run_nl);
		for (uint32_t i = 0; i < O.bases; ++i) printf("%x", X.nt4[i]);
		printf(" rows ");
		for (size_t r = 0; r < O.rows.size(); ++r) printf("%s%u:%u:%u", r ? "," : "", O.rows[r].gt_off, O.rows[r].nl_off, O.rows[r].base_rank);
		printf("\n");
	}
	fclose(fp);
	return 0;
}

// what gd_ref_open_host does (ref_fasta_driver.hip.h), without a device: for the digests of tests/golden/reffile
static int run_mmi(const char *path, int k, int w, const char *Z, const char *out)
{
	GdFastx *fx = gd_fastx_open(path);
	if (!fx) return 2;
	std::vector<std::string> names, seqs;
	for (;;) {
		bool bad = false;
		const int n = fx->read_batch((int64_t)1 << 28, false, false, false, &bad);
		if (n < 0) return 2;
		for (int i = 0; i < n; ++i) names.emplace_back(fx->v_name[(size_t)i]), seqs.emplace_back(fx->v_seq[(size_t)i], (size_t)fx->v_len[(size_t)i]);
		if (n == 0 && !bad) break;
	}
	gd_fastx_close(fx);
	GdPattern P;
	if (!gd_pattern_init(P, Z, (int)strlen(Z))) return 2;
	std::vector<GdSeqSpan> sp(seqs.size());
	for (size_t i = 0; i < seqs.size(); ++i) sp[i].p = seqs[i].data(), sp[i].n = seqs[i].size();
	GdIndex I;
	gd_index_build(I, names, sp, k, w, P, 4, true);
	std::string err;
	if (!gd_index_write_mmi(I, out, 14, err)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 7 && !strcmp(argv[1], "mmi")) return run_mmi(argv[2], atoi(argv[3]), atoi(argv[4]), argv[5], argv[6]);
	if (argc >= 3 && !strcmp(argv[1], "blocks")) return run_blocks(argv[2]);
	if (argc < 3 || strcmp(argv[1], "files")) { fprintf(stderr, "usage: ref_fasta_emul files FILE... | blocks CASES\n"); return 2; }
	const size_t blocks[4] = {256, 1024, 4096, (size_t)64 << 20};
	for (int i = 2; i < argc; ++i)
		for (size_t b : blocks) one_file(argv[i], b);
	return 0;
}
