// The winnowing automaton of map_stages.h (gd_sketch_range) in position-parallel form: a wavefront works through the sparsified
// positions of a read 64 at a time, one position per lane, in read order.  gd_sketch_range stays the definition -- this form must
// produce its emission list element for element (tests/emul/tile_sketch_test.cpp runs these statements on 64 emulated lock-step
// lanes against gd_sketch_core) -- but nothing here is sequential per base:
//   * a position's k-mer and hash do not depend on the automaton: the tile's bases are two 64-bit ballots (one per bit of the 2-bit
//     code), a lane's k-mer is the k bits of each that end at its position (the previous tile's ballots carried along);
//   * l, the run length of non-N bases, is the distance to the last set bit of the N ballot at or below the lane;
//   * the automaton's running minimum after step i is always the rightmost smallest entry of the last w -- M(i) -- found for all 64
//     positions at once by doubling (windows of 1, 2, 4, ... entries) plus one overlapping combine; the order "smaller x, then the
//     later position" is total and min is idempotent, so overlapping windows are exact;
//   * every emission of step i follows from M(i-1), M(i), l and the new entry (see "emissions" below), and a tile's emissions are
//     compacted in read order with a ballot and a prefix count, straight to the destination list.
// A capped pass stops at the tile that reaches the cap; the warm-up of w + k steps happens once per pass, not once per lane.
// ONE WAVEFRONT PER BLOCK is assumed (the kernel's __launch_bounds__(64)): GDT_SYNC orders a phase's LDS writes before the next phase's
// reads, but the reads of ring slots a LATER tile overwrites (level 0's y words of the previous tile, read by the compaction and the
// final flush) are kept ahead of those writes only by a wavefront issuing its LDS operations in order.
// Lanes exchange values through a small LDS record (GdTileLds: rings of 128 entries, the current and the previous tile); on the host
// the record is plain memory and every phase between two exchanges is a loop over the 64 lanes.
#pragma once
#include "map_stages.h"

#define GDT_LEVELS 7 // windows of 1, 2, ..., 64 entries (w <= GDM_MAX_W = 64)
#define GDT_RING 128

struct GdTileLds {
	uint64_t lx[GDT_LEVELS][GDT_RING]; // level p: smallest x of the 2^p entries that end at position i (level 0: the entries themselves)
	uint32_t lo[GDT_LEVELS][GDT_RING]; // level 0: low word of the entry's y; above: distance from i back to the rightmost | leftmost << 8 of the smallest
	uint64_t mx[GDT_RING];             // M(i): the window minimum after step i ...
	uint32_t mo[GDT_RING];             // ... and its distances, as in lo
	uint32_t cnt[64];                  // emissions per lane (tiles with tie emissions only)
	int32_t ones_loc[GDM_MAX_ONES];
};

#if defined(__HIP_DEVICE_COMPILE__)
#define GDT_NL 1
#define GDT_EACH_LANE for (unsigned lane = threadIdx.x & 63, gdt_once_ = 1; gdt_once_; gdt_once_ = 0)
#define GDT_LI 0
#define GDT_SYNC() __syncthreads()
#define GDT_BALLOT(dst_, arr_) dst_ = __ballot(arr_[0])
#define GDT_NOUNROLL _Pragma("unroll 1") // (the loops stay loops: unrolled, the tie path's count loop alone keeps 64 loads in flight and the kernel reports 143 registers, not 64)
#else
#define GDT_NL 64
#define GDT_EACH_LANE for (unsigned lane = 0; lane < 64; ++lane)
#define GDT_LI lane
#define GDT_SYNC() ((void)0)
#define GDT_NOUNROLL
#define GDT_BALLOT(dst_, arr_) do { dst_ = 0; for (unsigned q_ = 0; q_ < 64; ++q_) dst_ |= (uint64_t)(arr_[q_] != 0) << q_; } while (0)
#endif
#define GDT_V(a_) a_[GDT_LI]

GDM_HD uint64_t gdt_brev64(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __brevll(v);
#else
	v = (v >> 1 & 0x5555555555555555ull) | (v & 0x5555555555555555ull) << 1;
	v = (v >> 2 & 0x3333333333333333ull) | (v & 0x3333333333333333ull) << 2;
	v = (v >> 4 & 0x0f0f0f0f0f0f0f0full) | (v & 0x0f0f0f0f0f0f0f0full) << 4;
	return __builtin_bswap64(v);
#endif
}

GDM_HD uint32_t gdt_spread16(uint32_t a) // bit j of the low half -> bit 2j
{
	a = (a | a << 8) & 0x00ff00ffu;
	a = (a | a << 4) & 0x0f0f0f0fu;
	a = (a | a << 2) & 0x33333333u;
	return (a | a << 1) & 0x55555555u;
}

GDM_HD int gdt_popc64(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __popcll(v);
#else
	return __builtin_popcountll(v);
#endif
}

// Sketch of dl sparsified positions.  The first min(total, cap) minimizers go to dst[0..) in the automaton's order (cap == 0: no
// cap).  Returns (wave-uniform) their number, or ~0u when one of them did not fit into dst_cap entries.
GDM_HDI unsigned gd_tile_sketch(const uint8_t *str, unsigned dl, int w, int k, uint32_t rid, unsigned shift, const GdPattern &P, bool final_ge,
                                GdMini *dst, unsigned dst_cap, uint32_t cap, GdTileLds *L)
{
	const uint64_t mask = (1ULL << 2 * k) - 1, yhi = (uint64_t)rid << 32;
	const uint32_t kmask = (1u << k) - 1;
	const unsigned ones = (unsigned)P.ones, W = (unsigned)P.W, loc0 = (unsigned)P.ones_loc[0];
	const bool one_1 = ones == 1;
	const int full = w + k - 1; // l of the first full window
	int ptop = 0;
	while ((2 << ptop) <= w) ++ptop;
	const unsigned rest = (unsigned)w - (1u << ptop); // the window is 2^ptop entries plus `rest` more
	const uint32_t lim = cap ? cap : UINT32_MAX;
	GDT_EACH_LANE {
		GDT_NOUNROLL
		for (int p = 0; p <= ptop; ++p) {
			L->lx[p][lane] = L->lx[p][lane + 64] = UINT64_MAX;
			L->lo[p][lane] = L->lo[p][lane + 64] = 0;
		}
		L->mx[lane] = L->mx[lane + 64] = UINT64_MAX;
		L->mo[lane] = L->mo[lane + 64] = 0;
		if (!one_1)
			GDT_NOUNROLL
			for (unsigned j = 0; j < ones; ++j) L->ones_loc[j] = P.ones_loc[j];
	}
	GDT_SYNC();
	uint64_t pb0 = 0, pb1 = 0; // the previous tile's bases
	unsigned lc = 0, have = 0; // l after the previous tile's last position; minimizers written so far
	uint8_t fbad[GDT_NL];
	GDT_EACH_LANE GDT_V(fbad) = 0;
	GDT_NOUNROLL
	for (unsigned t0 = 0; t0 < dl; t0 += 64) {
		uint8_t c[GDT_NL], f0[GDT_NL], f1[GDT_NL], fn[GDT_NL];
		uint32_t ylo[GDT_NL];
		// ---- the base of every position
		GDT_EACH_LANE {
			const unsigned i = t0 + lane;
			unsigned real;
			if (one_1) real = i * W + loc0 + shift;
			else {
				const unsigned iq = i / ones;
				real = iq * W + (unsigned)L->ones_loc[i - iq * ones] + shift;
			}
			uint8_t b = 4;
			if (i < dl) { b = str[real]; if (b > 4) b = 4; }
			GDT_V(c) = b, GDT_V(ylo) = real << 1;
			GDT_V(f0) = b & 1, GDT_V(f1) = (b >> 1) & 1, GDT_V(fn) = b >> 2;
		}
		uint64_t b0, b1, bN;
		GDT_BALLOT(b0, f0);
		GDT_BALLOT(b1, f1);
		GDT_BALLOT(bN, fn);
		// ---- l, the k-mer pair, the entry (info.x / info.y of the automaton); level 0 of the rings
		int l[GDT_NL], lp[GDT_NL];
		uint64_t x[GDT_NL], cx[GDT_NL];
		uint32_t co[GDT_NL];
		GDT_EACH_LANE {
			const uint64_t le = lane == 63 ? ~0ull : (2ull << lane) - 1; // lanes <= this one
			const uint64_t m = bN & le, mp = bN & (le >> 1);
			GDT_V(l) = m ? (int)lane - (63 - __builtin_clzll(m)) : (int)(lc + lane + 1);
			GDT_V(lp) = mp ? (int)lane - 1 - (63 - __builtin_clzll(mp)) : (int)(lc + lane);
			// bit 63 - j of v0 / v1: bit 0 / 1 of the base j positions back
			const uint64_t v0 = b0 << (63 - lane) | (pb0 >> lane) >> 1, v1 = b1 << (63 - lane) | (pb1 >> lane) >> 1;
			const uint32_t r0 = (uint32_t)gdt_brev64(v0) & kmask, r1 = (uint32_t)gdt_brev64(v1) & kmask;
			// forward k-mer: the newest base in the lowest two bits
			const uint64_t fw = (uint64_t)(gdt_spread16(r0 >> 16) | gdt_spread16(r1 >> 16) << 1) << 32 | (gdt_spread16(r0 & 0xffff) | gdt_spread16(r1 & 0xffff) << 1);
			// reverse complement: the 2-bit groups of fw in reverse order, complemented
			uint64_t rv = gdt_brev64(fw);
			rv = (rv >> 1 & 0x5555555555555555ull) | (rv & 0x5555555555555555ull) << 1;
			rv = ~(rv >> (64 - 2 * k)) & mask;
			uint64_t xi = UINT64_MAX;
			uint32_t z = 0;
			if (GDT_V(c) < 4 && GDT_V(l) >= k && fw != rv) {
				z = fw < rv ? 0 : 1;
				xi = gd_hash64(z ? rv : fw, mask) << 8 | (uint64_t)k; // span = min(l, k) = k here
			}
			GDT_V(ylo) |= z;
			GDT_V(x) = GDT_V(cx) = xi, GDT_V(co) = 0;
			const unsigned slot = (t0 + lane) & (GDT_RING - 1);
			L->lx[0][slot] = xi, L->lo[0][slot] = GDT_V(ylo);
		}
		GDT_SYNC();
		// ---- M(i) by doubling: the window of 2^p entries that ends at i = the one that ends at i - 2^(p-1) followed by the one at i
		GDT_NOUNROLL
		for (int p = 1; p <= ptop; ++p) {
			const unsigned d = 1u << (p - 1);
			GDT_EACH_LANE {
				const unsigned j = (t0 + lane - d) & (GDT_RING - 1), slot = (t0 + lane) & (GDT_RING - 1);
				const uint64_t xb = L->lx[p - 1][j];
				const uint32_t ob = (p == 1 ? 0u : L->lo[p - 1][j]) + d * 0x101u;
				const uint32_t oa = GDT_V(co);
				GDT_V(co) = ((xb < GDT_V(cx) ? ob : oa) & 0xffu) | ((xb <= GDT_V(cx) ? ob : oa) & 0xff00u);
				if (xb < GDT_V(cx)) GDT_V(cx) = xb;
				if (p < ptop || rest) L->lx[p][slot] = GDT_V(cx), L->lo[p][slot] = GDT_V(co);
			}
			GDT_SYNC();
		}
		uint64_t px[GDT_NL];
		uint32_t po[GDT_NL];
		GDT_EACH_LANE {
			const unsigned slot = (t0 + lane) & (GDT_RING - 1);
			if (rest) { // ... and the overlapping combine for a w that is no power of two
				const unsigned j = (t0 + lane - rest) & (GDT_RING - 1);
				const uint64_t xb = L->lx[ptop][j];
				const uint32_t ob = L->lo[ptop][j] + rest * 0x101u, oa = GDT_V(co);
				GDT_V(co) = ((xb < GDT_V(cx) ? ob : oa) & 0xffu) | ((xb <= GDT_V(cx) ? ob : oa) & 0xff00u);
				if (xb < GDT_V(cx)) GDT_V(cx) = xb;
			}
			L->mx[slot] = GDT_V(cx), L->mo[slot] = GDT_V(co);
		}
		GDT_SYNC();
		// ---- emissions of step i, in the automaton's order: M(i-1) on the N flush (l(i-1) >= w+k-1), on replacement by the new entry
		// (l >= w+k) or on leaving the window (l >= w+k-1); then, on leaving, the entries equal to the new minimum in window order except
		// the minimum itself; at l == w+k-1 the same over the window without the new entry.  Ties exist iff the leftmost smallest entry is
		// not the rightmost one.
		uint8_t ep[GDT_NL], et[GDT_NL];
		GDT_EACH_LANE {
			const unsigned j = (t0 + lane - 1) & (GDT_RING - 1);
			GDT_V(px) = L->mx[j], GDT_V(po) = L->mo[j];
			const bool vp = GDT_V(px) != UINT64_MAX, vc = GDT_V(cx) != UINT64_MAX;
			const bool left = vp && !(GDT_V(x) <= GDT_V(px)) && (GDT_V(po) & 0xffu) == (unsigned)(w - 1);
			bool e;
			if (GDT_V(c) >= 4) e = GDT_V(lp) >= full;
			else if (GDT_V(x) <= GDT_V(px)) e = GDT_V(l) >= full + 1;
			else e = left && GDT_V(l) >= full;
			GDT_V(ep) = vp && e && t0 + lane < dl;
			const bool t3 = left && GDT_V(l) >= full && vc, t4 = GDT_V(l) == full && vc;
			GDT_V(et) = (t3 || t4) && (GDT_V(co) & 0xffu) != (GDT_V(co) >> 8) && t0 + lane < dl;
		}
		uint64_t be, bt;
		GDT_BALLOT(be, ep);
		GDT_BALLOT(bt, et);
		unsigned total;
		if (bt == 0) { // (almost every tile) at most one emission per lane
			GDT_EACH_LANE {
				if (GDT_V(ep)) {
					const unsigned p = have + (unsigned)gdt_popc64(be & ((1ull << lane) - 1));
					if (p < lim) {
						if (p < dst_cap) {
							const unsigned a = (t0 + lane - 1 - (GDT_V(po) & 0xffu)) & (GDT_RING - 1);
							dst[p].x = GDT_V(px), dst[p].y = yhi | L->lo[0][a];
						} else GDT_V(fbad) = 1;
					}
				}
			}
			total = (unsigned)gdt_popc64(be);
		} else { // tie emissions: the lanes that have some read their window's entries back from level 0
			GDT_EACH_LANE {
				unsigned n = GDT_V(ep);
				if (GDT_V(et)) {
					const int i = (int)(t0 + lane), ac = i - (int)(GDT_V(co) & 0xffu); // (positions fit an int: a read has fewer than 2^31 bases)
					const int j1 = GDT_V(l) == full ? i - 1 : i; // (the first full window: without the new entry)
					GDT_NOUNROLL
					for (int j = i - w + 1; j <= j1; ++j)
						if (j >= 0 && j != ac && L->lx[0][j & (GDT_RING - 1)] == GDT_V(cx)) ++n;
				}
				L->cnt[lane] = n;
			}
			GDT_SYNC();
			total = 0;
			GDT_NOUNROLL
			for (unsigned q = 0; q < 64; ++q) total += L->cnt[q];
			GDT_EACH_LANE {
				unsigned p = have;
				GDT_NOUNROLL
				for (unsigned q = 0; q < lane; ++q) p += L->cnt[q];
				if (GDT_V(ep)) {
					if (p < lim) {
						if (p < dst_cap) {
							const unsigned a = (t0 + lane - 1 - (GDT_V(po) & 0xffu)) & (GDT_RING - 1);
							dst[p].x = GDT_V(px), dst[p].y = yhi | L->lo[0][a];
						} else GDT_V(fbad) = 1;
					}
					++p;
				}
				if (GDT_V(et)) {
					const int i = (int)(t0 + lane), ac = i - (int)(GDT_V(co) & 0xffu); // (positions fit an int: a read has fewer than 2^31 bases)
					const int j1 = GDT_V(l) == full ? i - 1 : i;
					GDT_NOUNROLL
					for (int j = i - w + 1; j <= j1; ++j)
						if (j >= 0 && j != ac && L->lx[0][j & (GDT_RING - 1)] == GDT_V(cx)) {
							if (p < lim) {
								if (p < dst_cap) dst[p].x = GDT_V(cx), dst[p].y = yhi | L->lo[0][j & (GDT_RING - 1)];
								else GDT_V(fbad) = 1;
							}
							++p;
						}
				}
			}
			GDT_SYNC();
		}
		have += total;
		if (have >= lim) { // the cap-th minimizer: the automaton returns from inside its loop
			have = lim;
			break;
		}
		if (t0 + 64 >= dl) { // the final flush, by the lane of the last position
			uint8_t ff[GDT_NL];
			GDT_EACH_LANE GDT_V(ff) = t0 + lane == dl - 1 && (final_ge ? GDT_V(l) >= full : GDT_V(l) > full) && GDT_V(cx) != UINT64_MAX;
			uint64_t bf;
			GDT_BALLOT(bf, ff);
			GDT_EACH_LANE {
				if (GDT_V(ff)) {
					if (have < dst_cap) {
						const unsigned a = (t0 + lane - (GDT_V(co) & 0xffu)) & (GDT_RING - 1);
						dst[have].x = GDT_V(cx), dst[have].y = yhi | L->lo[0][a];
					} else GDT_V(fbad) = 1;
				}
			}
			if (bf) ++have;
		}
		pb0 = b0, pb1 = b1;
		lc = bN ? (unsigned)__builtin_clzll(bN) : lc + 64;
	}
	uint64_t bb;
	GDT_BALLOT(bb, fbad);
	return bb ? ~0u : have;
}
