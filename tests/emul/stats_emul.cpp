// Stand-alone host run of the statistics accumulator, meant to be built with -fsanitize=address,undefined: the statements of
// stats_scatter_kernel (stats.h, which uses pile.h and cov.h) as loops over blocks, their four wavefronts and 64 lanes, on exact-size
// copies of every buffer, so that a read or an add outside them is a sanitizer report.  Local memory is a plain uint32 array per block,
// flushed as the kernel flushes it; an add that would carry out of a uint32 cell ends the run.
//
//   stats_emul <in.records> <ref.codes> <excl_flags> <min_mapq> <cycles> <max_len> <max_indel> <bound> <blocks> <n_ref> <len 0> ...
//       ref.codes holds one byte 0..4 per reference base, the contigs back to back.  bound 0: the default; blocks 0: the driver's choice.
//       Everything is run twice, with the lanes 0..63 and 63..0, and must agree.  Prints
//         BAD <index of the call's first bad record> <reason code> <reason text>      (only if there is one)
//         SUMMARY <the 26 counters>
//         TABLE <which> <its counters>                                                 per table, in the order of GDIET_STATS_*
// Exit status 0; 2 usage / file errors; 3 the input ends inside a record; 7 the two lane orders differ; 8 a uint32 cell would overflow.
#include <stdlib.h>
#include <memory>
#include "record_emul.h"
#include "stats.h"

struct Tables {
	uint32_t n_ref = 0;
	uint64_t bound = 0, blocks = 0;
	GdtOpt opt;
	GdtLayout Y;
	std::unique_ptr<uint32_t[]> clen, S;
	std::unique_ptr<uint64_t[]> seq_off;
};
struct Result {
	std::unique_ptr<uint64_t[]> cells;
	uint64_t first_bad = ~(uint64_t)0;
};

struct Host {
	uint32_t *lds;
	uint64_t *cells;
	uint32_t n_lds, n_all, direct;
	void add(uint32_t cell, uint64_t v) const
	{
		if (cell >= n_all || v == 0) return;
		if (cell < n_lds && !direct) {
			if ((uint64_t)lds[cell] + v > 0xffffffffull) exit(8);
			lds[cell] += (uint32_t)v;
		} else cells[cell] += v;
	}
	void add_hot(uint32_t cell) const { add(cell, 1); }
};

static void flush(uint32_t *lds, uint64_t *cells, uint32_t n_lds)
{
	for (uint32_t i = 0; i < n_lds; ++i) cells[i] += lds[i], lds[i] = 0;
}

// the statements of one wavefront behind the step's barrier, on its record
static void passes(Host &W, const uint8_t *rec, const GdcHead &H, uint32_t is_read, uint32_t is_aln, const Tables &T, uint64_t *summary, bool down)
{
	uint32_t lead, trail;
	gdt_hard_ends(rec, H, &lead, &trail);
	GdtRecord R;
	gdt_record_clear(&R);
	if (is_read) {
		GdtReadLane A[64], S;
		gdt_read_lane_clear(&S);
		for (uint32_t i = 0; i < 64; ++i) {
			const uint32_t lane = down ? 63 - i : i;
			gdt_read_lane_clear(&A[lane]);
			gdt_read_share(W, T.Y, rec, H, lead, trail, T.opt.cycles, lane, &A[lane]);
		}
		for (uint32_t l = 0; l < 64; ++l) { // the wave sums
			S.a += A[l].a, S.g += A[l].g, S.tqn += A[l].tqn, S.tqs += A[l].tqs;
			for (int c = 0; c < 5; ++c) S.tb[c] += A[l].tb[c];
		}
		gdt_read_close(W, T.Y, H, T.opt, S);
		R.v[GDT_S_READS - GDT_S_READS] = 1, R.v[GDT_S_READ_BASES - GDT_S_READS] = H.l_seq;
	}
	if (is_aln) {
		GdtAlnLane A[64];
		for (uint32_t l = 0; l < 64; ++l) gdt_aln_lane_clear(&A[l]);
		const uint64_t seq_base = T.seq_off[H.refID];
		const uint32_t clen = T.clen[H.refID];
		uint32_t carry_r = (uint32_t)H.pos, carry_q = 0;
		for (uint32_t b0 = 0; b0 < H.n_ops; b0 += 64) {
			uint32_t L[64], rl[64], ql[64], kind[64], r[64], q[64], s[64], n[64], run[64], tot_r = 0, tot_q = 0;
			for (uint32_t l = 0; l < 64; ++l) kind[l] = gdp_op(rec, H, b0 + l, &L[l], &rl[l], &ql[l]);
			for (uint32_t l = 0; l < 64; ++l) r[l] = carry_r + tot_r, q[l] = carry_q + tot_q, tot_r += rl[l], tot_q += ql[l]; // the two exclusive scans
			for (uint32_t i = 0; i < 64; ++i) {
				const uint32_t l = down ? 63 - i : i;
				gdt_op_share(W, T.Y, rec, H, T.opt.max_indel, b0 + l, kind[l], L[l], &A[l]);
				run[l] = kind[l] == GDP_K_BASES && H.l_seq > 0 && gdp_run_of(kind[l], r[l], (uint32_t)H.pos, L[l], &s[l], &n[l]);
			}
			for (uint32_t jn = 0; jn < 64; ++jn) { // one run after another, every lane on each
				if (!run[jn]) continue;
				for (uint32_t i = 0; i < 64; ++i) {
					const uint32_t lane = down ? 63 - i : i;
					gdt_run_share(W, T.Y, rec, H, T.S.get(), seq_base, clen, lead, trail, T.opt.cycles, s[jn], n[jn], q[jn], lane, &A[lane]);
				}
			}
			carry_r += tot_r, carry_q += tot_q;
		}
		uint64_t m = 0, x = 0, o = 0, tcn = 0, tcx = 0, ie = 0, de = 0, db = 0, ib = 0, sc = 0, hc = 0;
		for (uint32_t l = 0; l < 64; ++l)
			m += A[l].m, x += A[l].x, o += A[l].o, tcn += A[l].tcn, tcx += A[l].tcx, ie += A[l].ie, de += A[l].de, db += A[l].db, ib += A[l].ib, sc += A[l].sc, hc += A[l].hc;
		gdt_aln_close(W, T.Y, H, T.opt, m, x, tcn, tcx, ie, de);
		gdt_aln_record(H, m, x, o, ie, ib, de, db, sc, hc, &R);
	}
	for (int i = 0; i < GDT_N_SUMMARY - GDT_S_READS; ++i) summary[GDT_S_READS + i] += R.v[i];
}

static void run(const std::string &data, const std::vector<uint64_t> &start, const Tables &T, bool down, Result &R)
{
	R.cells.reset(new uint64_t[T.Y.n_all]());
	std::unique_ptr<uint8_t[]> buf(new uint8_t[data.size()]);
	if (!data.empty()) memcpy(buf.get(), data.data(), data.size());
	const uint64_t n_rec = start.size();
	uint64_t blocks = T.blocks ? T.blocks : (n_rec + 3) / 4;
	if (blocks > GDT_MAX_BLOCKS) blocks = GDT_MAX_BLOCKS;
	uint64_t *summary = R.cells.get() + T.Y.off[GDT_T_SUMMARY];
	for (uint64_t block = 0; block < blocks; ++block) {
		std::unique_ptr<uint32_t[]> lds(new uint32_t[T.Y.n_lds]());
		uint64_t held = 0;
		for (uint64_t j0 = block * 4; j0 < n_rec; j0 += blocks * 4) {
			GdcHead H[4];
			uint32_t is_read[4] = {}, is_aln[4] = {}, direct[4] = {};
			uint64_t all = 0;
			for (uint32_t wave = 0; wave < 4; ++wave) {
				const uint64_t j = j0 + wave;
				if (j >= n_rec) continue;
				const uint32_t reason = record_pass1(buf.get(), data.size(), start[j], T.n_ref, T.clen.get(), down, &H[wave]);
				const uint32_t bits = gdt_classes(H[wave], reason, T.opt.excl_flags, T.opt.min_mapq, &is_read[wave], &is_aln[wave]);
				for (uint32_t l = 0; l < GDT_S_READS; ++l) summary[l] += bits >> l & 1u;
				note_bad(&R.first_bad, j, reason);
				const uint64_t weight = gdt_weight(H[wave], is_read[wave], is_aln[wave]);
				direct[wave] = weight > T.bound / 4;
				if (!direct[wave]) all += weight;
			}
			if (held + all > T.bound) flush(lds.get(), R.cells.get(), T.Y.n_lds), held = 0;
			held += all;
			for (uint32_t i = 0; i < 4; ++i) {
				const uint32_t wave = down ? 3 - i : i;
				if (j0 + wave >= n_rec || (!is_read[wave] && !is_aln[wave])) continue;
				Host W = {lds.get(), R.cells.get(), T.Y.n_lds, T.Y.n_all, direct[wave]};
				passes(W, buf.get() + start[j0 + wave], H[wave], is_read[wave], is_aln[wave], T, summary, down);
			}
		}
		flush(lds.get(), R.cells.get(), T.Y.n_lds);
	}
}

int main(int argc, char **argv)
{
	const int fixed = 11;
	if (argc < fixed || argc != fixed + atoi(argv[10])) {
		fprintf(stderr, "usage: stats_emul <in.records> <ref.codes> <excl_flags> <min_mapq> <cycles> <max_len> <max_indel> <bound> <blocks> <n_ref> <len> ...\n");
		return 2;
	}
	std::string data, codes;
	if (!slurp(argv[1], data) || !slurp(argv[2], codes)) return 2;
	Tables T;
	T.opt.excl_flags = (uint32_t)strtoul(argv[3], nullptr, 0), T.opt.min_mapq = (uint32_t)strtoul(argv[4], nullptr, 0), T.opt.cycles = (uint32_t)strtoul(argv[5], nullptr, 0);
	T.opt.max_len = (uint32_t)strtoul(argv[6], nullptr, 0), T.opt.max_indel = (uint32_t)strtoul(argv[7], nullptr, 0);
	T.bound = strtoull(argv[8], nullptr, 0), T.blocks = strtoull(argv[9], nullptr, 0), T.n_ref = (uint32_t)strtoul(argv[10], nullptr, 0);
	if (!T.bound) T.bound = GDT_DEFAULT_BOUND;
	if (!T.n_ref || T.bound > GDT_DEFAULT_BOUND || T.opt.cycles < 1 || T.opt.cycles > GDT_MAX_CYCLES || T.opt.max_len < 1 || T.opt.max_len > GDT_MAX_LEN || T.opt.max_indel < 1 ||
	    T.opt.max_indel > GDT_MAX_INDEL)
		return 2;
	T.Y = gdt_layout(T.opt.cycles, T.opt.max_len, T.opt.max_indel);
	T.clen.reset(new uint32_t[T.n_ref]), T.seq_off.reset(new uint64_t[T.n_ref]);
	uint64_t bases = 0;
	for (uint32_t r = 0; r < T.n_ref; ++r) T.clen[r] = (uint32_t)strtoul(argv[fixed + r], nullptr, 0), T.seq_off[r] = bases, bases += T.clen[r];
	if (codes.size() != bases) { fprintf(stderr, "ref.codes holds %zu bases, the contigs %llu\n", codes.size(), (unsigned long long)bases); return 2; }
	T.S.reset(new uint32_t[(bases + 7) / 8]());
	for (uint64_t u = 0; u < bases; ++u) T.S[u >> 3] |= ((uint32_t)codes[u] & 15u) << ((u & 7) << 2);
	std::vector<uint64_t> start;
	if (record_starts(data, start)) return 3;
	Result up, dn;
	run(data, start, T, false, up), run(data, start, T, true, dn);
	if (memcmp(up.cells.get(), dn.cells.get(), 8 * (size_t)T.Y.n_all) || up.first_bad != dn.first_bad) return 7;
	print_bad(up.first_bad);
	printf("SUMMARY");
	for (int i = 0; i < GDT_N_SUMMARY; ++i) printf(" %llu", (unsigned long long)up.cells[T.Y.off[GDT_T_SUMMARY] + i]);
	printf("\n");
	for (int t = 0; t < GDT_T_SUMMARY; ++t) {
		printf("TABLE %d", t);
		for (uint32_t k = 0; k < T.Y.len[t]; ++k) printf(" %llu", (unsigned long long)up.cells[T.Y.off[t] + k]);
		printf("\n");
	}
	return 0;
}
