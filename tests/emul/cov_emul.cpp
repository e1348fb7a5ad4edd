// Stand-alone host run of the coverage accumulator, meant to be built with -fsanitize=address,undefined: the statements of
// cov_scatter_kernel, of the chunked inclusive sum and of cov_window_kernel (cov.h) as loops over records and over 64 lanes, on exact-size
// copies of every buffer, so that a read or an add outside them is a sanitizer report.  A running sum stands for hipCUB's scan.
//
//   cov_emul <in.records> <excl_flags> <min_mapq> <window> <chunk> <n_ref> <len 0> ... <len n_ref-1>
//       Everything is run twice, with the lanes 0..63 and 63..0, and must agree.  Prints
//         BAD <index of the call's first bad record> <reason code> <reason text>      (only if there is one)
//         SUMMARY <the ten counters>
//         CONTIG <rid> <n_reads cov_bases sum_depth sum_mapq sum_baseq n_baseq>       per contig
//         WIN <rid> <n> <cov_bases sum_depth> x n                                     per contig, if window > 0
//         DEPTH <rid> <depth of every position>                                       per contig
// Exit status 0; 2 usage / file errors; 3 the input ends inside a record; 7 the two lane orders differ or the array's last slot is not 0.
#include <stdlib.h>
#include <memory>
#include "record_emul.h"

struct Tables {
	uint32_t n_ref = 0, excl = 0, min_mapq = 0, window = 0, win_eff = 65536;
	uint64_t chunk = 0;
	std::unique_ptr<uint32_t[]> clen;
	std::unique_ptr<uint64_t[]> base, wbase; // n_ref + 1
};
struct Result {
	std::unique_ptr<int32_t[]> diff; // total + 1
	std::unique_ptr<uint64_t[]> contig, summary;
	std::vector<uint32_t> win_cov;
	std::vector<uint64_t> win_sum;
	uint64_t first_bad = ~(uint64_t)0;
};

struct PlainAdd {
	void operator()(int32_t *p, int v) const { *p += v; }
};

// the statements of one wavefront of cov_scatter_kernel on record j
static void record(const uint8_t *buf, uint64_t len, uint64_t at, uint64_t j, const Tables &T, Result &R, bool down)
{
	GdcHead H;
	const uint32_t reason = record_pass1(buf, len, at, T.n_ref, T.clen.get(), down, &H);
	const uint8_t *rec = buf + at;
	uint32_t counted;
	const uint32_t bits = gdc_summary_bits(H, reason, T.excl, T.min_mapq, &counted);
	for (uint32_t l = 0; l < GDC_N_SUMMARY; ++l) R.summary[l] += bits >> l & 1u;
	note_bad(&R.first_bad, j, reason);
	if (!counted) return;
	const uint64_t base = T.base[H.refID];
	const uint32_t clen = T.clen[H.refID];
	uint32_t carry_r = (uint32_t)H.pos, carry_q = 0;
	uint64_t depth = 0, sumq = 0;
	for (uint32_t b0 = 0; b0 < H.n_ops; b0 += 64) {
		uint32_t L[64], rl[64], ql[64], m[64], r[64], q[64], unused = 0, tot_r = 0, tot_q = 0;
		for (uint32_t l = 0; l < 64; ++l) m[l] = gdc_op(rec, H, b0 + l, &L[l], &rl[l], &ql[l], &unused);
		for (uint32_t l = 0; l < 64; ++l) r[l] = carry_r + tot_r, q[l] = carry_q + tot_q, tot_r += rl[l], tot_q += ql[l]; // the two exclusive scans
		for (uint32_t i = 0; i < 64; ++i) {
			const uint32_t lane = down ? 63 - i : i;
			if (m[lane]) gdc_scatter(PlainAdd(), R.diff.get(), base, clen, r[lane], L[lane]), depth += L[lane];
		}
		if (H.has_qual)
			for (uint32_t jn = 0; jn < 64; ++jn) // one run after another, every lane on each
				if (m[jn] && L[jn])
					for (uint32_t i = 0; i < 64; ++i) sumq += gdc_qual_share(rec, H, q[jn], L[jn], down ? 63 - i : i);
		carry_r += tot_r, carry_q += tot_q;
	}
	uint64_t *c = R.contig.get() + (uint64_t)H.refID * GDC_N_CONTIG;
	c[GDC_C_READS] += 1, c[GDC_C_DEPTH] += depth, c[GDC_C_MAPQ] += H.mapq, c[GDC_C_BASEQ] += sumq, c[GDC_C_NBASEQ] += H.has_qual ? depth : 0;
}

static int run(const std::string &data, const std::vector<uint64_t> &start, const Tables &T, bool down, Result &R)
{
	const uint64_t total = T.base[T.n_ref];
	R.diff.reset(new int32_t[total + 1]()), R.contig.reset(new uint64_t[(size_t)GDC_N_CONTIG * T.n_ref]()), R.summary.reset(new uint64_t[GDC_N_SUMMARY]());
	std::unique_ptr<uint8_t[]> buf(new uint8_t[data.size()]);
	if (!data.empty()) memcpy(buf.get(), data.data(), data.size());
	for (size_t j = 0; j < start.size(); ++j) record(buf.get(), data.size(), start[j], j, T, R, down);
	// the inclusive sum in chunks: the previous chunk's last depth goes onto a chunk's first slot first
	const uint64_t slots = total + 1, chunk = T.chunk && T.chunk < slots ? T.chunk : slots;
	for (uint64_t c0 = 0; c0 < slots; c0 += chunk) {
		if (c0) R.diff[c0] += R.diff[c0 - 1];
		for (uint64_t k = c0 + 1; k < c0 + chunk && k < slots; ++k) R.diff[k] += R.diff[k - 1];
	}
	if (R.diff[total] != 0) return 7;
	const uint64_t n_win = T.wbase[T.n_ref];
	R.win_cov.assign(n_win, 0), R.win_sum.assign(n_win, 0);
	for (uint64_t w = 0; w < n_win; ++w) {
		uint64_t beg, end;
		const uint32_t rid = gdc_window_range(T.base.get(), T.wbase.get(), T.n_ref, T.win_eff, w, &beg, &end);
		for (uint32_t i = 0; i < 64; ++i) {
			uint32_t c;
			uint64_t s;
			gdc_window_share((const uint32_t *)R.diff.get(), beg, end, down ? 63 - i : i, &c, &s);
			R.win_cov[w] += c, R.win_sum[w] += s;
		}
		R.contig[(size_t)GDC_N_CONTIG * rid + GDC_C_COV] += R.win_cov[w];
	}
	return 0;
}

int main(int argc, char **argv)
{
	if (argc < 8 || argc != 7 + atoi(argv[6])) {
		fprintf(stderr, "usage: cov_emul <in.records> <excl_flags> <min_mapq> <window> <chunk> <n_ref> <len> ...\n");
		return 2;
	}
	std::string data;
	if (!slurp(argv[1], data)) return 2;
	Tables T;
	T.excl = (uint32_t)strtoul(argv[2], nullptr, 0), T.min_mapq = (uint32_t)strtoul(argv[3], nullptr, 0), T.window = (uint32_t)strtoul(argv[4], nullptr, 0);
	T.chunk = strtoull(argv[5], nullptr, 0), T.n_ref = (uint32_t)strtoul(argv[6], nullptr, 0);
	T.win_eff = T.window ? T.window : 65536;
	T.clen.reset(new uint32_t[T.n_ref]), T.base.reset(new uint64_t[T.n_ref + 1]()), T.wbase.reset(new uint64_t[T.n_ref + 1]());
	for (uint32_t r = 0; r < T.n_ref; ++r) {
		T.clen[r] = (uint32_t)strtoul(argv[7 + r], nullptr, 0);
		T.base[r + 1] = T.base[r] + T.clen[r], T.wbase[r + 1] = T.wbase[r] + ((uint64_t)T.clen[r] + T.win_eff - 1) / T.win_eff;
	}
	std::vector<uint64_t> start;
	if (record_starts(data, start)) return 3;
	Result up, dn;
	if (run(data, start, T, false, up) || run(data, start, T, true, dn)) return 7;
	const uint64_t total = T.base[T.n_ref];
	if (memcmp(up.diff.get(), dn.diff.get(), 4 * (total + 1)) || memcmp(up.contig.get(), dn.contig.get(), 8 * (size_t)GDC_N_CONTIG * T.n_ref) ||
	    memcmp(up.summary.get(), dn.summary.get(), 8 * GDC_N_SUMMARY) || up.first_bad != dn.first_bad || up.win_cov != dn.win_cov || up.win_sum != dn.win_sum)
		return 7;
	print_bad(up.first_bad);
	printf("SUMMARY");
	for (int i = 0; i < GDC_N_SUMMARY; ++i) printf(" %llu", (unsigned long long)up.summary[i]);
	printf("\n");
	for (uint32_t r = 0; r < T.n_ref; ++r) {
		printf("CONTIG %u", r);
		for (int i = 0; i < GDC_N_CONTIG; ++i) printf(" %llu", (unsigned long long)up.contig[(size_t)GDC_N_CONTIG * r + i]);
		printf("\n");
	}
	for (uint32_t r = 0; r < T.n_ref && T.window; ++r) {
		printf("WIN %u %llu", r, (unsigned long long)(T.wbase[r + 1] - T.wbase[r]));
		for (uint64_t w = T.wbase[r]; w < T.wbase[r + 1]; ++w) printf(" %u %llu", up.win_cov[w], (unsigned long long)up.win_sum[w]);
		printf("\n");
	}
	for (uint32_t r = 0; r < T.n_ref; ++r) {
		printf("DEPTH %u", r);
		for (uint64_t k = T.base[r]; k < T.base[r + 1]; ++k) printf(" %u", (unsigned)up.diff[k]);
		printf("\n");
	}
	return 0;
}
