// CPU check of the position-parallel sketch (map_tile_sketch.h): gd_tile_sketch() run on 64 emulated lock-step lanes must give the
// emission list of the sequential automaton gd_sketch_core(), element for element: every (x, y) in order, the count, the cut at a
// cap and the real location of the cap-th minimizer (tmp_extracted_len).
//   tile_sketch_test [seed]
// Sequences are made in sparsified space (what the automaton sees) and spread over the pattern's 1-positions, so that N runs, tile
// boundaries and lengths are exact.  Patterns 10 / 1 / 110 / 0001 / 40 ones, every shift < W, k in {11, 15, 19, 21, 28},
// w in {1, 8, 10, 19, 33, 64}; the lengths, generators and caps rotate through every setting.  How often the rare paths fire is counted
// from the automaton alone: gd_sketch_slice over single steps of the sequences of up to 800 positions gives the emissions of every
// step (two or more: a tie enumeration, at l == w+k-1 the first-full-window one; one on an N: the flush), a capped gd_sketch_core that
// returns `cap` minimizers is a cap cut; the caps "on a tile's last emission" come from gd_sketch_slice over whole tiles.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include <string>
#include <vector>
#define __host__
#define __device__
#include "map_tile_sketch.h"

struct EmitV {
	std::vector<GdMini> *v;
	size_t cap;
	bool operator()(const GdMini &m) { v->push_back(m); return v->size() == cap; }
};

static std::mt19937 g;
static GdTileLds L;
static long runs = 0, bad = 0, overflow_checks = 0, tie_leave = 0, tie_first = 0, n_flush = 0, cap_cut = 0;

static unsigned real_of(const GdPattern &P, unsigned i, unsigned shift) { return (i / P.ones) * P.W + P.ones_loc[i % P.ones] + shift; }

// one comparison at one cap (0: none)
static void check(const std::vector<uint8_t> &s, unsigned len, unsigned dl, const GdPattern &P, unsigned shift, int k, int w, uint32_t cap, bool final_ge,
                  unsigned dst_cap, const char *what)
{
	std::vector<GdMini> ref;
	EmitV e = {&ref, cap ? (size_t)cap : (size_t)-1};
	gd_sketch_core(s.data(), dl, w, k, 0, shift, P, final_ge, e);
	const uint32_t tel_ref = cap && ref.size() == cap ? (uint32_t)(ref.back().y >> 1) : len;
	std::vector<GdMini> out(dst_cap ? dst_cap : 1);
	const unsigned n = gd_tile_sketch(s.data(), dl, w, k, 0, shift, P, final_ge, out.data(), dst_cap, cap, &L);
	++runs;
	if (cap && ref.size() == cap) ++cap_cut;
	bool ok;
	if (ref.size() > dst_cap) ok = n == ~0u, ++overflow_checks;
	else {
		ok = n == ref.size();
		for (size_t i = 0; ok && i < ref.size(); ++i) ok = ref[i].x == out[i].x && ref[i].y == out[i].y;
		const uint32_t tel = cap && n == cap ? (uint32_t)(out[n - 1].y >> 1) : len;
		ok = ok && tel == tel_ref;
	}
	if (!ok && ++bad <= 8)
		fprintf(stderr, "MISMATCH %s dl=%u k=%d w=%d pat=%s shift=%u cap=%u final_ge=%d dst_cap=%u ref=%zu got=%u\n", what, dl, k, w, P.Z, shift, cap, (int)final_ge,
		        dst_cap, ref.size(), n);
}

// all caps of one sequence
static void check_all(const std::vector<uint8_t> &sp, const GdPattern &P, unsigned shift, int k, int w, const char *what)
{
	const unsigned dl = (unsigned)sp.size();
	const unsigned len = dl ? real_of(P, dl - 1, shift) + 1 : shift;
	std::vector<uint8_t> s(len + 8);
	for (auto &c : s) c = g() % 5; // the bases the pattern skips are never read
	for (unsigned i = 0; i < dl; ++i) s[real_of(P, i, shift)] = sp[i];
	if (gd_diet_len(P, len, shift) != dl) { fprintf(stderr, "generator: diet_len\n"); exit(2); }
	std::vector<GdMini> all, t1;
	EmitV e = {&all, (size_t)-1};
	gd_sketch_core(s.data(), dl, w, k, 0, shift, P, true, e);
	const unsigned total = (unsigned)all.size();
	check(s, len, dl, P, shift, k, w, 0, true, total + 1, what);
	check(s, len, dl, P, shift, k, w, 0, false, total + 1, what);
	if (dl <= 800) { // what fires at every step, by the automaton alone
		int l = 0;
		for (unsigned i = 0; i < dl; ++i) {
			t1.clear();
			EmitV e1 = {&t1, (size_t)-1};
			gd_sketch_slice(s.data(), dl, i, i + 1, w, k, 0, shift, P, true, e1);
			if (sp[i] >= 4) { if (!t1.empty()) ++n_flush; l = 0; continue; }
			++l;
			if (i + 1 < dl && t1.size() >= 2) ++(l == w + k - 1 ? tie_first : tie_leave); // (the last step's slice holds the final flush as well)
		}
	}
	if (total == 0) return;
	// emissions of the steps of the first one / two tiles, by the automaton
	unsigned on_tile[2] = {0, 0};
	for (int t = 0; t < 2; ++t) {
		if (64u * (t + 1) >= dl) break;
		t1.clear();
		EmitV e1 = {&t1, (size_t)-1};
		gd_sketch_slice(s.data(), dl, 0, 64u * (t + 1), w, k, 0, shift, P, true, e1);
		on_tile[t] = (unsigned)t1.size();
	}
	const uint32_t caps[] = {1, on_tile[0], on_tile[1], on_tile[0] + 1, total / 2, total - 1, total, total + 5};
	for (uint32_t cap : caps)
		if (cap) check(s, len, dl, P, shift, k, w, cap, (cap & 1) != 0, cap < total ? cap : total, what);
	check(s, len, dl, P, shift, k, w, total / 2 + 1, true, total + 1, what);
	if (total > 1) check(s, len, dl, P, shift, k, w, 0, true, total - 1, what); // a list that does not fit: reported, nothing written past it
}

static void fill_random(std::vector<uint8_t> &v) { for (auto &c : v) c = g() & 3; }

static void put_n(std::vector<uint8_t> &v, long at, long n)
{
	for (long i = at; i < at + n; ++i)
		if (i >= 0 && i < (long)v.size()) v[i] = 4;
}

int main(int argc, char **argv)
{
	g.seed(argc > 1 ? atoi(argv[1]) : 1);
	const std::string p40 = std::string(20, '1') + "0" + std::string(20, '1') + "00";
	const char *pats[] = {"10", "1", "110", "0001", p40.c_str()};
	const int ks[] = {11, 15, 19, 21, 28}, ws[] = {1, 8, 10, 19, 33, 64};
	unsigned rot = 0;
	for (const char *pz : pats) {
		GdPattern P;
		if (!gd_pattern_init(P, pz, (int)strlen(pz))) return 2;
		for (unsigned shift = 0; shift < (unsigned)P.W; ++shift)
			for (int k : ks)
				for (int w : ws) {
					const int f = w + k - 1;
					const unsigned lens[] = {0, 1, (unsigned)k - 1, (unsigned)k, (unsigned)f - 1, (unsigned)f, (unsigned)f + 1, (unsigned)f + 2, 63, 64, 65, 127, 128, 129,
					                         (unsigned)(2000 + g() % 3000), (unsigned)(300 + g() % 500)};
					const int nruns = P.W > 8 ? 3 : 8; // (the 40-ones pattern has 43 shifts)
					for (int r = 0; r < nruns; ++r, ++rot) {
						std::vector<uint8_t> v(lens[rot % 16]);
						const long n = (long)v.size();
						const int gen = (rot / 16 + rot) % 11;
						const long nrun[] = {1, k - 1, k, f - 1, f, f + 1};
						const long nr = nrun[(rot / 7) % 6];
						fill_random(v);
						const char *what = "random";
						switch (gen) {
						case 1: { const uint8_t b = g() & 3; for (auto &c : v) c = b; what = "homopolymer"; break; }
						case 2: { const uint8_t a = g() & 3, b = g() & 3; for (auto &c : v) c = g() & 1 ? a : b; what = "two letters"; break; }
						case 3: case 4: { // tandem repeat: equal hashes in one window
							const long u = 1 + g() % 40;
							for (long i = u; i < n; ++i) v[i] = v[i - u];
							if (gen == 4 && n > 200) for (long i = n / 3; i < n / 2; ++i) v[i] = g() & 3; // ... with a unique stretch inside
							what = "tandem";
							break;
						}
						case 5: { // reverse-palindromic: the second half is the reverse complement of the first (palindromic k-mers for even k)
							for (long i = 0; i < n / 2; ++i) v[n - 1 - i] = 3 - v[i];
							if (n > 300) for (long i = 0; i + 28 <= n; i += 97) for (int j = 0; j < 14; ++j) v[i + 27 - j] = 3 - v[i + j];
							what = "palindromes";
							break;
						}
						case 6: put_n(v, 0, nr), put_n(v, n - nr, nr), what = "N at both ends"; break;
						case 7: put_n(v, 64 - nr / 2, nr), put_n(v, 128 - 1, nr), what = "N over a tile boundary"; break;
						case 8: { // the only non-N stretch is exactly w+k-1 long, at a varying place (also across a boundary)
							const long at = n > f ? (long)(g() % (n - f + 1)) : 0;
							std::vector<uint8_t> o(v);
							put_n(v, 0, n);
							for (long i = at; i < at + f && i < n; ++i) v[i] = o[i];
							if (g() & 1) { const long u = 1 + g() % 5; for (long i = at + u; i < at + f && i < n; ++i) v[i] = v[i - u]; }
							what = "one full window";
							break;
						}
						case 10: { // random stretches and short-period repeats in turn: a minimum of a random stretch leaves the window inside a repeat,
							// where the new minimum has copies (the tie enumeration on leaving the window)
							for (long at = f + (long)(g() % 20); at < n; at += 3 * w + k + 10) {
								const long u = 1 + g() % 3;
								for (long i = at + u; i < at + 2 * w + k && i < n; ++i) v[i] = v[i - u];
							}
							what = "repeats in turn";
							break;
						}
						case 9: { // scattered N runs of the critical lengths in a repeat
							const long u = 1 + g() % 12;
							for (long i = u; i < n; ++i) v[i] = v[i - u];
							for (long at = g() % 90; at < n; at += f + 1 + g() % 150) put_n(v, at, nrun[g() % 6]);
							what = "N runs in a repeat";
							break;
						}
						}
						check_all(v, P, shift, k, w, what);
					}
				}
	}
	printf("tile_sketch_test runs=%ld mismatches=%ld tie_leave=%ld tie_first=%ld n_flush=%ld cap_cut=%ld overflow_checks=%ld\n", runs, bad, tie_leave, tie_first, n_flush,
	       cap_cut, overflow_checks);
	return bad != 0;
}
