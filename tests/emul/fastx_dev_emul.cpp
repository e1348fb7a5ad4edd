// CPU emulator of the reader's device mode (csrc/fastx_dev.h, the statements of the kernels in csrc/fastx_dev.hip.h as host loops),
// built with -fsanitize=address,undefined by tests/test_fastx_device.py.
//
//     fastx_dev_emul FILE BLOCK_BYTES CHUNK_BASES
//
// An executor that runs the device's passes on the host -- newline / '\r' masks per 16-byte lane of every 1 KiB tile, the tile counts,
// their exclusive scan, the offsets written from the scanned positions, the record predicate and header split per group of four
// lines, first_bad as a minimum, the nt4 map over every accepted sequence -- is installed in a real GdFastx, so blocks, tails and
// batches are the reader's own.  Inside every block each accepted record is compared with what GdFastxParser returns from the same
// position (name, comment, sequence, quality, length, where the next record starts), and the hand-over position with where that
// parser stands.  Then the attached reader's batches are compared with those of an unattached one.
// Prints "ok device D host H total T early E blocks B handed K"; any difference ends the program with status 1.
#include "fastx_reader.h"
#include "nt4_encode.h"
#include <stdio.h>

static void die(const char *what, size_t block_at, long r)
{
	printf("MISMATCH %s (block of %zu bytes, record %ld)\n", what, block_at, r);
	exit(1);
}

struct EmulDevice : GdFastxDevice {
	long parse(const unsigned char *b, size_t n, std::vector<GdxRec> &rec, std::shared_ptr<void> &dev) override
	{
		rec.clear(), dev.reset();
		const uint32_t n32 = (uint32_t)n, n_tiles = (n32 + GDX_TILE - 1) / GDX_TILE;
		// the device's copy: whole tiles, the bytes past the end are whatever the allocation holds (made hostile here)
		std::vector<unsigned char> blk((size_t)n_tiles * GDX_TILE, (unsigned char)'\n');
		memcpy(blk.data(), b, n);
		auto lane_words = [&](uint32_t at, uint32_t w[4]) { memcpy(w, blk.data() + at, 16); };
		// count pass
		std::vector<uint32_t> counts(n_tiles + 1, 0), tile_off(n_tiles + 1, 0);
		uint32_t first_cr = GDX_NONE;
		for (uint32_t t = 0; t < n_tiles; ++t)
			for (uint32_t lane = 0; lane < 64; ++lane) {
				const uint32_t at = t * GDX_TILE + lane * GDX_LANE_BYTES, valid = gdx_valid16(at, n32);
				uint32_t w[4];
				lane_words(at, w);
				const uint32_t m = gdx_eq_mask16(w, '\n', valid), crm = gdx_eq_mask16(w, '\r', valid);
				for (uint32_t j = 0; j < 16; ++j) { // the mask against the bytes themselves
					const bool in = at + j < n32;
					if (((m >> j) & 1u) != (uint32_t)(in && b[at + j] == '\n') || ((crm >> j) & 1u) != (uint32_t)(in && b[at + j] == '\r')) die("lane mask", n, (long)at);
				}
				counts[t] += (uint32_t)__builtin_popcount(m);
				if (crm) first_cr = std::min(first_cr, at + (uint32_t)__builtin_ctz(crm));
			}
		// scan
		for (uint32_t t = 0; t < n_tiles; ++t) tile_off[t + 1] = tile_off[t] + counts[t];
		const uint32_t n_lines = tile_off[n_tiles], n_cand = n_lines / 4;
		if (n_cand == 0) return 0;
		// write pass: every lane stores at the scanned position of its tile plus the set bits of the lanes below it
		const uint32_t cap = n_lines;
		std::vector<uint32_t> nl(cap, GDX_NONE);
		for (uint32_t t = 0; t < n_tiles; ++t) {
			uint32_t below = 0;
			for (uint32_t lane = 0; lane < 64; ++lane) {
				const uint32_t at = t * GDX_TILE + lane * GDX_LANE_BYTES;
				uint32_t w[4];
				lane_words(at, w);
				uint32_t m = gdx_eq_mask16(w, '\n', gdx_valid16(at, n32)), o = tile_off[t] + below;
				below += (uint32_t)__builtin_popcount(m);
				while (m) {
					if (o >= cap) die("offset table overflow", n, (long)o);
					nl[o] = at + (uint32_t)__builtin_ctz(m);
					m &= m - 1, ++o;
				}
			}
		}
		for (uint32_t k = 0; k < n_lines; ++k)
			if (nl[k] >= n32 || b[nl[k]] != '\n' || (k && nl[k] <= nl[k - 1])) die("newline offsets", n, (long)k);
		// record pass
		std::vector<GdxRec> all(n_cand);
		uint32_t first_bad = GDX_NONE;
		for (uint32_t r = 0; r < n_cand; ++r)
			if (!gdx_record(blk.data(), nl.data(), r, first_cr, all[r])) first_bad = std::min(first_bad, r);
		const uint32_t n_acc = std::min(first_bad, n_cand);
		// what the sequential grammar returns from the same positions
		GdFastxParser P;
		P.b = b, P.begin = 0, P.end = n;
		size_t pos = 0;
		for (uint32_t r = 0; r < n_acc; ++r) {
			const GdxRec &R = all[r];
			int64_t o[4];
			const size_t a0 = P.arena.size();
			const long l = P.read_record(true, true, o);
			if (l < 0 || P.eof || P.last_char != 0) die("the parser does not return this record", n, r);
			if ((size_t)l != R.seq_len) die("length", n, r);
			if (strlen(P.arena.data() + o[0]) != R.name_len || memcmp(P.arena.data() + o[0], b + R.name_off, R.name_len)) die("name", n, r);
			if ((o[1] < 0) != (R.comment_off == GDX_NONE)) die("comment presence", n, r);
			if (o[1] >= 0 && (strlen(P.arena.data() + o[1]) != R.comment_len || memcmp(P.arena.data() + o[1], b + R.comment_off, R.comment_len))) die("comment", n, r);
			if (o[3] < 0 || memcmp(P.arena.data() + o[3], b + R.qual_off, R.seq_len) || P.arena[(size_t)o[3] + R.seq_len] != 0) die("quality", n, r);
			// the sequence: the host string is the line with U -> T, the resident batch its nt4 codes, the flag says whether a U was there
			bool flag = false, has_u = false;
			std::vector<uint8_t> enc(R.seq_len), want(R.seq_len);
			for (uint32_t k = 0; k < R.seq_len; ++k) {
				const unsigned char c = b[R.seq_off + k];
				enc[k] = (uint8_t)gdx_nt4(c), flag |= gdx_is_u(c);
				has_u |= c == 'U' || c == 'u';
				const char host = (char)(gdx_is_u(c) ? c - 1 : c);
				if (P.arena[(size_t)o[2] + k] != host) die("sequence", n, r);
			}
			gd_nt4_encode(P.arena.data() + o[2], want.data(), R.seq_len); // what gdiet_hip_batch_upload makes of the host string
			if (enc != want || flag != has_u) die("nt4 codes", n, r);
			pos = P.begin;
			if (pos != (size_t)R.qual_off + R.seq_len + 1) die("where the next record starts", n, r);
			P.arena.resize(a0);
		}
		(void)pos;
		rec.assign(all.begin(), all.begin() + n_acc);
		return (long)n_acc;
	}
};

static std::string digest(const char *path, bool attach, size_t block, int64_t chunk, long *n_out, int *early, int64_t st[4])
{
	GdFastx *fx = gd_fastx_open(path);
	if (!fx) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
	fx->block_size = block;
	if (attach) fx->dev = std::make_shared<EmulDevice>();
	std::string d;
	long n = 0;
	*early = 0;
	for (;;) {
		bool bad = false;
		const int k = fx->read_batch(chunk, true, true, false, &bad);
		if (k < 0) { printf("MISMATCH read error\n"); exit(1); }
		if (k == 0 && !bad) break;
		fx->u_to_t_on_host();
		for (int i = 0; i < k; ++i) {
			if ((int32_t)strlen(fx->v_seq[i]) != fx->v_len[i]) die("string length", block, n + i);
			d += fx->v_name[i], d += '\t', d += fx->v_comment[i] ? fx->v_comment[i] : "-", d += '\t', d += fx->v_seq[i], d += '\t';
			d += fx->v_qual[i] ? fx->v_qual[i] : "-", d += '\n';
		}
		d += bad ? "==bad==\n" : "==\n";
		*early += bad;
		n += k;
	}
	st[0] = fx->n_rec_device, st[1] = fx->n_rec_host, st[2] = fx->n_blocks, st[3] = fx->n_blocks_handed;
	gd_fastx_close(fx);
	*n_out = n;
	return d;
}

int main(int argc, char **argv)
{
	if (argc < 4) return 2;
	for (unsigned c = 0; c < 256; ++c)
		if (gdx_nt4(c) != gd_nt4_byte((unsigned char)c) || gdx_is_u(c) != (c == 'U' || c == 'u')) { printf("MISMATCH nt4 of byte %u\n", c); return 1; }
	const size_t block = (size_t)atol(argv[2]);
	const int64_t chunk = atol(argv[3]);
	long n0 = 0, n1 = 0;
	int e0 = 0, e1 = 0;
	int64_t s0[4], s1[4];
	const std::string want = digest(argv[1], false, block, chunk, &n0, &e0, s0);
	const std::string got = digest(argv[1], true, block, chunk, &n1, &e1, s1);
	if (want != got) { printf("MISMATCH attached and unattached reader differ (%ld vs %ld records)\n", n1, n0); return 1; }
	if (s1[0] + s1[1] != n1 || s0[0] != 0 || s0[1] != n0) { printf("MISMATCH statistics\n"); return 1; }
	printf("ok device %lld host %lld total %ld early %d blocks %lld handed %lld\n", (long long)s1[0], (long long)s1[1], n1, e1, (long long)s1[2], (long long)s1[3]);
	return 0;
}
