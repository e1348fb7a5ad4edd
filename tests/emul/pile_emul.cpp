// Stand-alone host run of the pileup accumulator, meant to be built with -fsanitize=address,undefined: the statements of
// pile_scatter_kernel, pile_call_kernel, the chunked exclusive sum and pile_site_kernel (pile.h, which uses cov.h) as loops over records and
// over 64 lanes, on exact-size copies of every buffer, so that a read or an add outside them is a sanitizer report.  A running sum stands
// for hipCUB's scan.
//
//   pile_emul <in.records> <ref.codes> <excl_flags> <min_mapq> <min_baseq> <chunk> <min_depth> <min_alt> <num> <den>
//             <n_ref> <len 0> ... <n_reg> <rid beg end> ...
//       ref.codes holds one byte 0..4 per reference base, the contigs back to back.  Everything is run twice, with the lanes 0..63 and
//       63..0, and must agree.  Prints
//         BAD <index of the call's first bad record> <reason code> <reason text>      (only if there is one)
//         SUMMARY <the twelve counters>
//         COUNTS <region> <eight counters of every position>                          per region
//         CONS <region> <consensus bytes>                                             per region
//         SITE <rid pos ref alt depth> <eight counters>                               per site, in order
// Exit status 0; 2 usage / file errors; 3 the input ends inside a record; 7 the two lane orders differ.
#include <stdlib.h>
#include <memory>
#include "record_emul.h"
#include "pile.h"

struct Tables {
	uint32_t n_ref = 0, n_reg = 0, excl = 0, min_mapq = 0, min_baseq = 0;
	uint64_t chunk = 0, total = 0;
	GdpCallOpt opt;
	std::unique_ptr<uint32_t[]> clen, S;
	std::unique_ptr<uint64_t[]> seq_off;
	std::unique_ptr<GdpRegion[]> regs;
};
struct Result {
	std::unique_ptr<uint32_t[]> cnt; // 8 x total
	std::unique_ptr<uint64_t[]> summary;
	std::vector<std::string> cons;
	std::vector<uint32_t> rows; // 13 a site
	uint64_t first_bad = ~(uint64_t)0;
};

struct Host {
	uint32_t uni(uint32_t v) const { return v; }
	uint64_t uni64(uint64_t v) const { return v; }
	void add(uint32_t *p) const { *p += 1; }
};

// the statements of one wavefront of pile_scatter_kernel on record j
static void record(const uint8_t *buf, uint64_t len, uint64_t at, uint64_t j, const Tables &T, Result &R, bool down)
{
	Host W;
	GdcHead H;
	const uint32_t reason = record_pass1(buf, len, at, T.n_ref, T.clen.get(), down, &H);
	const uint8_t *rec = buf + at;
	uint32_t counted;
	const uint32_t bits = gdp_summary_bits(H, reason, T.excl, T.min_mapq, &counted);
	for (uint32_t l = 0; l < GDP_S_SKIPPED_BASEQ; ++l) R.summary[l] += bits >> l & 1u;
	note_bad(&R.first_bad, j, reason);
	if (!counted) return;
	uint32_t carry_r = (uint32_t)H.pos, carry_q = 0;
	for (uint32_t b0 = 0; b0 < H.n_ops; b0 += 64) {
		uint32_t L[64], rl[64], ql[64], kind[64], r[64], q[64], s[64], n[64], run[64], tot_r = 0, tot_q = 0;
		for (uint32_t l = 0; l < 64; ++l) kind[l] = gdp_op(rec, H, b0 + l, &L[l], &rl[l], &ql[l]);
		for (uint32_t l = 0; l < 64; ++l) r[l] = carry_r + tot_r, q[l] = carry_q + tot_q, tot_r += rl[l], tot_q += ql[l]; // the two exclusive scans
		for (uint32_t l = 0; l < 64; ++l) run[l] = gdp_run_of(kind[l], r[l], (uint32_t)H.pos, L[l], &s[l], &n[l]);
		for (uint32_t jn = 0; jn < 64; ++jn) { // one run after another, every lane on each
			if (!run[jn]) continue;
			const uint32_t i0 = gdp_region_lower(W, T.regs.get(), T.n_reg, (uint32_t)H.refID, s[jn]);
			for (uint32_t i = 0; i < 64; ++i)
				R.summary[GDP_S_SKIPPED_BASEQ] += gdp_run_share(W, R.cnt.get(), T.regs.get(), T.n_reg, i0, rec, H, kind[jn], s[jn], n[jn], q[jn], T.min_baseq, down ? 63 - i : i);
		}
		carry_r += tot_r, carry_q += tot_q;
	}
}

// one thread of pile_call_kernel / pile_site_kernel on position t
static uint32_t call_position(const Tables &T, const Result &R, uint64_t t, uint32_t *row, uint8_t *cons)
{
	const uint32_t i = gdp_region_of(T.regs.get(), T.n_reg, t);
	const GdpRegion &G = T.regs[i];
	const uint32_t *c = R.cnt.get() + t * GDP_N_CNT;
	row[0] = G.rid, row[1] = G.beg + (uint32_t)(t - G.off);
	row[2] = gdp_ref_base(T.S.get(), T.seq_off[G.rid] + row[1]);
	for (int k = 0; k < GDP_N_CNT; ++k) row[5 + k] = c[k];
	return gdp_call(c, row[2], T.opt, cons, &row[4], &row[3]);
}

static void run(const std::string &data, const std::vector<uint64_t> &start, const Tables &T, bool down, Result &R)
{
	R.cnt.reset(new uint32_t[(size_t)GDP_N_CNT * T.total]()), R.summary.reset(new uint64_t[GDP_N_SUMMARY]());
	std::unique_ptr<uint8_t[]> buf(new uint8_t[data.size()]);
	if (!data.empty()) memcpy(buf.get(), data.data(), data.size());
	for (size_t j = 0; j < start.size(); ++j) record(buf.get(), data.size(), start[j], j, T, R, down);
	for (uint32_t g = 0; g < T.n_reg; ++g) { // the consensus of every region
		const uint64_t n = T.regs[g].end - T.regs[g].beg;
		std::unique_ptr<uint8_t[]> cons(new uint8_t[n]);
		uint32_t row[13];
		for (uint64_t k = 0; k < n; ++k) (void)call_position(T, R, T.regs[g].off + (down ? n - 1 - k : k), row, &cons[down ? n - 1 - k : k]);
		R.cons.push_back(std::string((const char *)cons.get(), n));
	}
	// the sites: per chunk the flags, their exclusive sum, the rows at the offsets; the chunk's count is the carry
	const uint64_t chunk = T.chunk && T.chunk < T.total ? T.chunk : T.total;
	for (uint64_t c0 = 0; c0 < T.total; c0 += chunk) {
		const uint64_t m = chunk < T.total - c0 ? chunk : T.total - c0;
		std::unique_ptr<uint32_t[]> flag(new uint32_t[m]), offs(new uint32_t[m]);
		uint32_t row[13], sum = 0;
		uint8_t cb;
		for (uint64_t k = 0; k < m; ++k) flag[k] = call_position(T, R, c0 + k, row, &cb);
		for (uint64_t k = 0; k < m; ++k) offs[k] = sum, sum += flag[k];
		const uint32_t n_c = offs[m - 1] + flag[m - 1];
		std::unique_ptr<uint32_t[]> rows(new uint32_t[13 * (size_t)n_c]);
		for (uint64_t i = 0; i < m; ++i) {
			const uint64_t k = down ? m - 1 - i : i;
			if (call_position(T, R, c0 + k, row, &cb) && offs[k] < n_c) memcpy(rows.get() + 13 * (size_t)offs[k], row, sizeof row);
		}
		R.rows.insert(R.rows.end(), rows.get(), rows.get() + 13 * (size_t)n_c);
	}
}

int main(int argc, char **argv)
{
	const int fixed = 12;
	if (argc < fixed || argc < fixed + atoi(argv[11]) + 1 || argc != fixed + atoi(argv[11]) + 1 + 3 * atoi(argv[fixed + atoi(argv[11])])) {
		fprintf(stderr, "usage: pile_emul <in.records> <ref.codes> <excl_flags> <min_mapq> <min_baseq> <chunk> <min_depth> <min_alt> <num> <den> <n_ref> <len> ... <n_reg> <rid beg end> ...\n");
		return 2;
	}
	std::string data, codes;
	if (!slurp(argv[1], data) || !slurp(argv[2], codes)) return 2;
	Tables T;
	T.excl = (uint32_t)strtoul(argv[3], nullptr, 0), T.min_mapq = (uint32_t)strtoul(argv[4], nullptr, 0), T.min_baseq = (uint32_t)strtoul(argv[5], nullptr, 0);
	T.chunk = strtoull(argv[6], nullptr, 0);
	T.opt.min_depth = (uint32_t)strtoul(argv[7], nullptr, 0), T.opt.min_alt = (uint32_t)strtoul(argv[8], nullptr, 0);
	T.opt.num = (uint32_t)strtoul(argv[9], nullptr, 0), T.opt.den = (uint32_t)strtoul(argv[10], nullptr, 0);
	T.n_ref = (uint32_t)strtoul(argv[11], nullptr, 0);
	if (!T.n_ref || !T.opt.den) return 2;
	T.clen.reset(new uint32_t[T.n_ref]), T.seq_off.reset(new uint64_t[T.n_ref]);
	uint64_t bases = 0;
	for (uint32_t r = 0; r < T.n_ref; ++r) T.clen[r] = (uint32_t)strtoul(argv[fixed + r], nullptr, 0), T.seq_off[r] = bases, bases += T.clen[r];
	if (codes.size() != bases) { fprintf(stderr, "ref.codes holds %zu bases, the contigs %llu\n", codes.size(), (unsigned long long)bases); return 2; }
	T.S.reset(new uint32_t[(bases + 7) / 8]());
	for (uint64_t u = 0; u < bases; ++u) T.S[u >> 3] |= ((uint32_t)codes[u] & 15u) << ((u & 7) << 2);
	const int ra = fixed + (int)T.n_ref;
	T.n_reg = (uint32_t)strtoul(argv[ra], nullptr, 0);
	if (!T.n_reg) return 2;
	T.regs.reset(new GdpRegion[T.n_reg]);
	for (uint32_t g = 0; g < T.n_reg; ++g) {
		GdpRegion &G = T.regs[g];
		G.off = T.total, G.rid = (uint32_t)strtoul(argv[ra + 1 + 3 * g], nullptr, 0), G.beg = (uint32_t)strtoul(argv[ra + 2 + 3 * g], nullptr, 0), G.end = (uint32_t)strtoul(argv[ra + 3 + 3 * g], nullptr, 0), G.pad = 0;
		if (G.rid >= T.n_ref || G.beg >= G.end || G.end > T.clen[G.rid]) return 2;
		T.total += G.end - G.beg;
	}
	std::vector<uint64_t> start;
	if (record_starts(data, start)) return 3;
	Result up, dn;
	run(data, start, T, false, up), run(data, start, T, true, dn);
	if (memcmp(up.cnt.get(), dn.cnt.get(), 4 * (size_t)GDP_N_CNT * T.total) || memcmp(up.summary.get(), dn.summary.get(), 8 * GDP_N_SUMMARY) || up.first_bad != dn.first_bad ||
	    up.cons != dn.cons || up.rows != dn.rows)
		return 7;
	print_bad(up.first_bad);
	printf("SUMMARY");
	for (int i = 0; i < GDP_N_SUMMARY; ++i) printf(" %llu", (unsigned long long)up.summary[i]);
	printf("\n");
	for (uint32_t g = 0; g < T.n_reg; ++g) {
		printf("COUNTS %u", g);
		for (uint64_t k = T.regs[g].off * GDP_N_CNT; k < (T.regs[g].off + (T.regs[g].end - T.regs[g].beg)) * GDP_N_CNT; ++k) printf(" %u", up.cnt[k]);
		printf("\nCONS %u %s\n", g, up.cons[g].c_str());
	}
	for (size_t k = 0; k < up.rows.size(); k += 13) {
		printf("SITE");
		for (int i = 0; i < 13; ++i) printf(" %u", up.rows[k + i]);
		printf("\n");
	}
	return 0;
}
