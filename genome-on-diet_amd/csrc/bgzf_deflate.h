// A DEFLATE (RFC 1951) encoder that writes one complete BGZF member per wavefront: the statements, written once for the kernel
// (bgzf_deflate.hip.h) and for the host emulator that runs them as loops over 64 lanes (tests/emul/bgzf_deflate_emul.cpp).  No HIP in
// here.  The decoder's twin is bgzf_inflate.h; the member layout is that of bgzf.h.
//
// HOW THE WORK IS SPLIT.  The member's input (at most 65280 bytes) is staged in local memory.  It is then walked 64 positions at a time:
//   * MATCH SEARCH, 64 positions side by side: lane l hashes the three bytes at p = base + l, reads the hash table's candidate (the latest
//     earlier position with that hash, of an EARLIER group of 64: the probes of a group all come before its insertions), verifies it and
//     extends it byte by byte to at most 258, and leaves (length, distance) of its position in local memory; then every lane inserts its
//     position, and where lanes of one group share a hash the highest position wins (GDD_ATOMIC_MAX);
//   * a wave-uniform GREEDY PASS walks the group (the cursor is kept uniform, GDD_UNI): a match of length >= 3 is taken where the cursor
//     stands and skipped over, anything else is a literal.  Tokens go into a buffer of GDD_TOK tokens in local memory;
//   * when the buffer is full, or the input ends, the tokens become ONE DEFLATE BLOCK: the lanes count symbol frequencies (atomic adds),
//     gdd_build_lengths makes length-limited code lengths (the sort is a rank sort over the lanes, the Huffman pass and the repair of
//     the Kraft sum are a few hundred serial steps on lane 0), the exact sizes of a dynamic and of a fixed block are computed from the
//     frequencies, and the smaller one is written: 64 tokens at a time, every lane shifts its token's bits to the place a prefix sum of
//     the bit counts gives it and ORs them into a small staging area (GDD_ATOMIC_OR: lanes share words), whose whole words then go to
//     global memory;
//   * the CRC32 (zlib's polynomial) is computed by the same wavefront from the staged input: every lane takes a slice bit by bit, moves
//     its remainder to the end of the member by a multiplication with x^(8 * bytes behind the slice) mod P, and the 64 terms are XORed.
//
// TOKENS OF A WHOLE MEMBER do not fit beside the input, so a member is SEVERAL DEFLATE BLOCKS, each with codes of its own, over one
// shared window (the staged input: a match of a later block may reach into an earlier one).  The header of a dynamic block uses the
// zero-run codes 17 and 18 and a code-length code built by gdd_build_lengths with the limit 7; code 16 is not used.
// FALLBACKS: a block is written fixed (BTYPE 1) when that is smaller than dynamic; the whole member is written as one stored block
// (BTYPE 0) as soon as the stream would not be smaller than 5 + in_len bytes, so a member is at most 18 + 5 + 65280 + 8 = 65311 bytes.
// The output is never read back from global memory: the first five words (they hold BSIZE, known last) wait in local memory, and a
// stored rewrite starts again at word 0 behind a release fence.
//
// DETERMINISM: a member's bytes are a function of its input bytes alone.  Wherever two lanes can meet in one local-memory word in one
// statement the operation commutes (max for the hash table, add for the frequencies, or for the bits), no lane-loop body reads what
// another lane writes in the same statement (GDD_WAVE_FENCE stands between the statements), and everything else is wave-uniform.  The
// emulator is built with the lane loops running 0..63 and 63..0 (GDD_LANES_DOWN) and must print the same members.
//
// RULES THAT KEEP IT SAFE (the emulator runs the same statements under ASan / UBSan on exact-size copies of input and output):
//   W1 no input byte at or behind in_len is read: a position is hashed only if p + 3 <= in_len, a match is extended while p + l < in_len
//      (its source lies below p), staging reads whole 16-byte pieces only where they lie inside the input;
//   W2 every store to the output is checked against the slot (GDD_SLOT bytes), every store to the staging area against its size, and the
//      stream is bounded before it is written: a block whose exact size would take the stream to 5 + in_len bytes or more is not written,
//      the member is rewritten as a stored block instead -- never an overrun;
//   W3 a match has length 3..258 and distance 1..32768, and its source starts at or behind the member's first byte (candidates are
//      positions of this member);
//   W4 every iteration of the greedy loop consumes at least one input byte, every other loop counts up to a bound known before it starts.
//
// LOCAL MEMORY: GddLds is 65296 (input) + 16384 (hash table, 4096 words) + 16384 (4096 tokens) + about 6.5 KiB (frequencies, codes,
// code lengths, the builder's arrays, the per-lane arrays and the 512-byte staging area) = 104656 bytes per wavefront: ONE wavefront
// per CU of 160 KiB, 256 on the device.  Two per CU would need the hash table and the token buffer together below 14 KiB beside the
// staged input; a mini-batch of SAM text is about 1600 members, so the device is full either way.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define GDD_HD __host__ __device__ __forceinline__
#else
#define GDD_HD static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define GDD_LANES(lane) for (uint32_t lane = threadIdx.x, once_ = 1; once_; once_ = 0)
#define GDD_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#define GDD_WAVE_FENCE() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront")
#define GDD_STORE_FENCE() __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent")
#define GDD_ROLLED _Pragma("clang loop unroll(disable) vectorize(disable) interleave(disable)")
#define GDD_ATOMIC_MAX(x, v) ((void)__hip_atomic_fetch_max(&(x), (uint32_t)(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
#define GDD_ATOMIC_ADD(x, v) ((void)__hip_atomic_fetch_add(&(x), (uint32_t)(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
#define GDD_ATOMIC_OR(x, v) ((void)__hip_atomic_fetch_or(&(x), (uint32_t)(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
#else
#define GDD_ROLLED
#if defined(GDD_LANES_DOWN) // (the emulator's second build: a result that depends on the order of the lanes shows)
#define GDD_LANES(lane) for (uint32_t lane = 63; lane < 64; --lane)
#else
#define GDD_LANES(lane) for (uint32_t lane = 0; lane < 64; ++lane)
#endif
#define GDD_UNI(x) ((uint32_t)(x))
#define GDD_WAVE_FENCE() ((void)0)
#define GDD_STORE_FENCE() ((void)0)
#define GDD_ATOMIC_MAX(x, v) ((void)((x) = (x) > (uint32_t)(v) ? (x) : (uint32_t)(v)))
#define GDD_ATOMIC_ADD(x, v) ((void)((x) += (uint32_t)(v)))
#define GDD_ATOMIC_OR(x, v) ((void)((x) |= (uint32_t)(v)))
#endif

enum { GDD_OK = 0, GDD_E_LEN = 1 };
enum {
	GDD_MAX_IN = 65280,  // bgzip's block size
	GDD_SLOT = 65536,    // a member's place in global memory; the largest member is 65311 bytes
	GDD_HEAD = 18,       // gzip header with the BC subfield
	GDD_HASH_BITS = 12,
	GDD_TOK = 4096,      // tokens of one DEFLATE block
	GDD_MIN_MATCH = 3, GDD_MAX_MATCH = 258, GDD_MAX_DIST = 32768,
	GDD_FAR = 4096,      // a match of length 3 further back than this costs more than its literals (zlib's TOO_FAR)
	GDD_NLIT = 286, GDD_NDIST = 30, GDD_NCL = 19,
	GDD_LITS = 288,      // where the distance lengths start in GddLds::lens
	GDD_OBUF = 128,      // words of the staging area: 31 bits left over + 64 x 48 bits of a chunk
	GDD_KEEP = 5         // the member's first words stay in local memory until BSIZE is known
};

struct alignas(16) GddV16 { uint32_t w[4]; };
struct GddBuild { // gdd_build_lengths' arrays
	uint32_t a[GDD_LITS];  // frequencies in ascending order, then parents, then depths
	uint16_t order[GDD_LITS]; // the symbols in that order
	uint32_t cnt[16];      // codes by length
};
struct GddLds {
	alignas(16) uint8_t in[GDD_MAX_IN + 16];
	uint32_t head[1 << GDD_HASH_BITS]; // position + 1 of the latest insertion, 0: none
	uint32_t tok[GDD_TOK];             // literal: the byte; match: 1 << 31 | (length - 3) << 15 | (distance - 1)
	uint32_t freq[GDD_LITS + 32], clfreq[GDD_NCL];
	uint16_t code[GDD_LITS + 32], clcode[GDD_NCL]; // first bit of the code in bit 0
	uint8_t lens[GDD_LITS + 32], cllens[GDD_NCL];
	uint16_t clsym[GDD_LITS + 32]; // the code lengths of a dynamic header as symbols of the code-length code: symbol | extra bits << 8
	GddBuild build;
	uint32_t mlen[64], mdist[64]; // per lane: the match at base + lane
	uint32_t eb_lo[64], eb_hi[64], nb[64]; // per lane: the bits of one token (first bit in bit 0) and how many
	uint32_t acc[4];               // sums over the lanes: extra bits, dynamic bits, fixed bits
	uint32_t ncl;                  // symbols in clsym
	uint32_t obuf[GDD_OBUF];       // the staging area
	uint32_t keep[GDD_KEEP + 1];
};

struct GddOut { // all of it wave-uniform
	uint32_t *dst;  // the member's slot (16-byte aligned)
	uint32_t bits;  // bits in the staging area
	uint32_t words; // words that have left it
};

// ---- code lengths ------------------------------------------------------------------------------------------------------------------
// Length-limited prefix code lengths for the frequencies freq[0, n) (n <= 288, max_bits <= 15, n <= 2^max_bits): lens[s] is 0 exactly
// where freq[s] is; with two or more symbols the code is complete (Kraft sum 1), a lone symbol gets length 1.  A plain Huffman build
// (the in-place two-queue pass over the sorted frequencies of Moffat and Katajainen), then the lengths above the limit are cut to it and
// the Kraft sum is repaired on the histogram of lengths, one unit at a time: the deepest code below the limit moves one level down and
// makes room for two at its new depth.  The lengths are handed out again in the order of the frequencies, so a rarer symbol never gets
// a shorter code.  Every lane of the wavefront calls it with the same arguments; freq and lens are local memory (or the emulator's heap).
// cut (the emulator's; the kernel passes none): counted up when the plain Huffman code was deeper than the limit, so that lengths were cut.
GDD_HD void gdd_build_lengths(const uint32_t *freq, uint32_t n, uint32_t max_bits, uint8_t *lens, GddBuild &B, uint32_t *cut = nullptr)
{
	GDD_WAVE_FENCE();
	// rank sort by (frequency, symbol) over the symbols that occur: every symbol has a rank of its own
	GDD_LANES(lane) GDD_ROLLED for (uint32_t s = lane; s < n; s += 64) {
		const uint32_t f = freq[s];
		lens[s] = 0;
		if (!f) continue;
		uint32_t r = 0;
		GDD_ROLLED for (uint32_t t = 0; t < n; ++t) {
			const uint32_t g = freq[t];
			r += g && (g < f || (g == f && t < s));
		}
		B.a[r] = f, B.order[r] = (uint16_t)s;
	}
	uint32_t m = 0;
	GDD_ROLLED for (uint32_t s = 0; s < n; ++s) m += GDD_UNI(freq[s]) != 0;
	GDD_WAVE_FENCE();
	if (m == 0) return;
	GDD_LANES(lane) if (lane == 0) {
		if (m == 1) lens[B.order[0]] = 1;
		else {
			uint32_t *A = B.a;
			A[0] += A[1];
			uint32_t root = 0, leaf = 2;
			GDD_ROLLED for (uint32_t next = 1; next + 1 < m; ++next) {
				if (leaf >= m || A[root] < A[leaf]) A[next] = A[root], A[root++] = next;
				else A[next] = A[leaf++];
				if (leaf >= m || (root < next && A[root] < A[leaf])) A[next] += A[root], A[root++] = next;
				else A[next] += A[leaf++];
			}
			A[m - 2] = 0;
			GDD_ROLLED for (uint32_t next = m - 2; next-- > 0;) A[next] = A[A[next]] + 1;
			// depths of the internal nodes -> histogram of the leaves' depths, cut at the limit
			GDD_ROLLED for (uint32_t l = 0; l < 16; ++l) B.cnt[l] = 0;
			int32_t avail = 1, used = 0, r = (int32_t)m - 2, left = (int32_t)m;
			GDD_ROLLED for (uint32_t depth = 0; avail > 0 && left > 0 && depth < GDD_LITS; ++depth) {
				GDD_ROLLED while (r >= 0 && A[r] == depth) ++used, --r;
				if (cut && avail > used && left > 0 && depth > max_bits) ++*cut, cut = nullptr;
				GDD_ROLLED while (avail > used && left > 0) B.cnt[depth < max_bits ? depth : max_bits]++, --avail, --left;
				avail = 2 * used, used = 0;
			}
			uint32_t total = 0;
			GDD_ROLLED for (uint32_t l = 1; l <= max_bits; ++l) total += B.cnt[l] << (max_bits - l);
			GDD_ROLLED for (uint32_t it = 0; total > (1u << max_bits) && it < GDD_LITS; ++it) { // (each turn takes one unit off: at most m turns)
				uint32_t l = max_bits - 1;
				GDD_ROLLED while (l > 0 && !B.cnt[l]) --l;
				if (l == 0) break;
				B.cnt[max_bits]--, B.cnt[l]--, B.cnt[l + 1] += 2, --total;
			}
			uint32_t i = 0;
			GDD_ROLLED for (uint32_t l = max_bits; l >= 1; --l)
				GDD_ROLLED for (uint32_t k = B.cnt[l]; k > 0 && i < m; --k) lens[B.order[i++]] = (uint8_t)l;
		}
	}
	GDD_WAVE_FENCE();
}

// the canonical codes of lens[0, n), bit-reversed (DEFLATE sends a code's first bit first, the stream fills its bytes from bit 0)
GDD_HD void gdd_make_codes(const uint8_t *lens, uint32_t n, uint16_t *code, GddBuild &B)
{
	GDD_WAVE_FENCE();
	GDD_LANES(lane) if (lane == 0) {
		uint32_t *next = B.a; // (the builder is done with its arrays)
		GDD_ROLLED for (uint32_t l = 0; l < 16; ++l) B.cnt[l] = 0;
		GDD_ROLLED for (uint32_t s = 0; s < n; ++s) B.cnt[lens[s] & 15u]++;
		B.cnt[0] = 0;
		uint32_t c = 0;
		next[0] = 0;
		GDD_ROLLED for (uint32_t l = 1; l < 16; ++l) c = (c + B.cnt[l - 1]) << 1, next[l] = c;
		GDD_ROLLED for (uint32_t s = 0; s < n; ++s) {
			const uint32_t l = lens[s] & 15u;
			uint32_t v = 0, r = 0;
			if (l) v = next[l]++;
			GDD_ROLLED for (uint32_t k = 0; k < l; ++k) r = r << 1 | (v & 1u), v >>= 1;
			code[s] = (uint16_t)r;
		}
	}
	GDD_WAVE_FENCE();
}

// ---- symbols -----------------------------------------------------------------------------------------------------------------------
GDD_HD uint32_t gdd_len_sym(uint32_t l3, uint32_t *extra, uint32_t *val) // l3 = length - 3, 0 .. 255; the symbol is 257 + the result
{
	if (l3 < 8) { *extra = 0, *val = 0; return l3; }
	if (l3 == 255) { *extra = 0, *val = 0; return 28; }
	const uint32_t e = (31u - (uint32_t)__builtin_clz(l3)) - 2u;
	*extra = e, *val = l3 & ((1u << e) - 1u);
	return 4u * e + 4u + ((l3 >> e) & 3u);
}
GDD_HD uint32_t gdd_dist_sym(uint32_t d1, uint32_t *extra, uint32_t *val) // d1 = distance - 1, 0 .. 32767
{
	if (d1 < 4) { *extra = 0, *val = 0; return d1; }
	const uint32_t nb = 31u - (uint32_t)__builtin_clz(d1), e = nb - 1u;
	*extra = e, *val = d1 & ((1u << e) - 1u);
	return 2u * nb + ((d1 >> e) & 1u);
}
GDD_HD uint32_t gdd_fixed_len(uint32_t s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u; }

// ---- the bit stream ----------------------------------------------------------------------------------------------------------------
// the staging area's whole words (all: its last, partly filled word too) to the member's slot; what is left moves to the front
GDD_HD void gdd_flush(GddLds &L, GddOut &O, bool all)
{
	const uint32_t nw = all ? (O.bits + 31u) >> 5 : O.bits >> 5;
	if (nw == 0) return;
	GDD_WAVE_FENCE();
	GDD_LANES(lane) GDD_ROLLED for (uint32_t w = lane; w < nw && w < GDD_OBUF; w += 64) {
		const uint32_t idx = O.words + w, v = L.obuf[w];
		if (idx < GDD_KEEP) L.keep[idx] = v;
		else if (idx < GDD_SLOT / 4) O.dst[idx] = v; // (W2)
	}
	GDD_WAVE_FENCE();
	GDD_LANES(lane) if (lane == 0) L.obuf[0] = !all && nw < GDD_OBUF ? L.obuf[nw] : 0u;
	GDD_WAVE_FENCE();
	GDD_LANES(lane) GDD_ROLLED for (uint32_t w = lane + 1; w <= nw && w < GDD_OBUF; w += 64) L.obuf[w] = 0;
	GDD_WAVE_FENCE();
	O.words += nw, O.bits = all ? 0u : O.bits & 31u;
}
// n <= 32 bits of v (nothing above them set), the same in every lane
GDD_HD void gdd_put(GddLds &L, GddOut &O, uint32_t v, uint32_t n)
{
	GDD_WAVE_FENCE();
	GDD_LANES(lane) if (lane == 0) {
		const uint32_t w = O.bits >> 5;
		const uint64_t t = (uint64_t)v << (O.bits & 31u);
		if (w < GDD_OBUF) L.obuf[w] |= (uint32_t)t;
		if (w + 1 < GDD_OBUF) L.obuf[w + 1] |= (uint32_t)(t >> 32);
	}
	GDD_WAVE_FENCE();
	O.bits += n; // (no flush: between two chunks, which flush, a member's header, a block's header and the trailer are below 400 bits)
}
// 64 pieces side by side: lane l has left nb[l] <= 48 bits in eb_lo / eb_hi[l]; they follow one another in lane order
GDD_HD void gdd_emit_chunk(GddLds &L, GddOut &O)
{
	if (O.bits >= 32) gdd_flush(L, O, false);
	GDD_WAVE_FENCE();
	uint32_t tot = 0;
	GDD_LANES(lane) {
		uint32_t off = 0, t = 0;
		GDD_ROLLED for (uint32_t j = 0; j < 64; ++j) {
			const uint32_t x = L.nb[j];
			t += x, off += j < lane ? x : 0u;
		}
		tot = t;
		if (L.nb[lane]) {
			const uint32_t b = O.bits + off, w = b >> 5, sh = b & 31u;
			const uint64_t lo = (uint64_t)L.eb_lo[lane] << sh, hi = (uint64_t)L.eb_hi[lane] << sh;
			const uint32_t w0 = (uint32_t)lo, w1 = (uint32_t)(lo >> 32) | (uint32_t)hi, w2 = (uint32_t)(hi >> 32);
			if (w0 && w < GDD_OBUF) GDD_ATOMIC_OR(L.obuf[w], w0);
			if (w1 && w + 1 < GDD_OBUF) GDD_ATOMIC_OR(L.obuf[w + 1], w1);
			if (w2 && w + 2 < GDD_OBUF) GDD_ATOMIC_OR(L.obuf[w + 2], w2);
		}
	}
	O.bits += GDD_UNI(tot);
	gdd_flush(L, O, false);
}
GDD_HD void gdd_put_head(GddLds &L, GddOut &O) // 1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 2 0, BSIZE (filled in at the end)
{
	gdd_put(L, O, 0x04088b1fu, 32), gdd_put(L, O, 0u, 32), gdd_put(L, O, 0x0006ff00u, 32), gdd_put(L, O, 0x00024342u, 32), gdd_put(L, O, 0u, 16);
}

// ---- CRC32 -------------------------------------------------------------------------------------------------------------------------
// a * b mod P in zlib's reflected representation (bit 31 is x^0, P = 0xedb88320): 32 steps whatever the operands
GDD_HD uint32_t gdd_mulmod(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	GDD_ROLLED for (uint32_t i = 0; i < 32; ++i) {
		p ^= (a >> (31u - i)) & 1u ? b : 0u;
		b = (b >> 1) ^ (0xedb88320u & (0u - (b & 1u)));
	}
	return p;
}
GDD_HD uint32_t gdd_xpow8(uint32_t k) // x^(8k) mod P, k < 2^17
{
	uint32_t r = 0x80000000u, base = 0x00800000u;
	GDD_ROLLED for (uint32_t i = 0; i < 17; ++i) {
		if (k >> i & 1u) r = gdd_mulmod(r, base);
		base = gdd_mulmod(base, base);
	}
	return r;
}
// zlib's crc32 of the staged input: register after n bytes = init * x^(8n) + sum over the slices of (remainder of the slice from
// register 0) * x^(8 * bytes behind it), all mod P; the result is its complement
GDD_HD uint32_t gdd_crc32(GddLds &L, uint32_t n)
{
	const uint32_t S = (n + 63u) / 64u;
	GDD_WAVE_FENCE();
	GDD_LANES(lane) {
		const uint32_t s0 = lane * S < n ? lane * S : n, s1 = s0 + S < n ? s0 + S : n;
		uint32_t r = 0;
		GDD_ROLLED for (uint32_t i = s0; i < s1; ++i) {
			r ^= L.in[i];
			GDD_ROLLED for (uint32_t k = 0; k < 8; ++k) r = (r >> 1) ^ (0xedb88320u & (0u - (r & 1u)));
		}
		L.nb[lane] = s1 > s0 ? gdd_mulmod(r, gdd_xpow8(n - s1)) : 0u;
	}
	GDD_WAVE_FENCE();
	uint32_t c = gdd_mulmod(0xffffffffu, gdd_xpow8(n));
	GDD_ROLLED for (uint32_t j = 0; j < 64; ++j) c ^= GDD_UNI(L.nb[j]);
	GDD_WAVE_FENCE();
	return ~c;
}

// ---- one block ---------------------------------------------------------------------------------------------------------------------
// The tokens tok[0, ntok) as one block, dynamic or fixed, whichever is smaller.  Returns false, with nothing written, if the stream
// would then not be smaller than a stored member's 5 + in_len bytes (W2).  cuts (the emulator's; the kernel passes none): three counters
// of gdd_build_lengths, for the literal/length code, the distance code and the code-length code.
GDD_HD bool gdd_block(GddLds &L, GddOut &O, uint32_t ntok, bool last, uint32_t in_len, uint32_t *cuts = nullptr)
{
	GDD_WAVE_FENCE();
	GDD_LANES(lane) {
		GDD_ROLLED for (uint32_t s = lane; s < GDD_LITS + 32; s += 64) L.freq[s] = 0;
		if (lane < GDD_NCL) L.clfreq[lane] = 0;
		if (lane < 4) L.acc[lane] = 0;
	}
	GDD_WAVE_FENCE();
	GDD_LANES(lane) {
		GDD_ROLLED for (uint32_t i = lane; i < ntok; i += 64) {
			const uint32_t t = L.tok[i];
			if (!(t >> 31)) { GDD_ATOMIC_ADD(L.freq[t & 255u], 1u); continue; }
			uint32_t e0, e1, v;
			const uint32_t ls = gdd_len_sym((t >> 15) & 255u, &e0, &v), ds = gdd_dist_sym(t & 32767u, &e1, &v);
			GDD_ATOMIC_ADD(L.freq[257u + ls], 1u), GDD_ATOMIC_ADD(L.freq[GDD_LITS + ds], 1u), GDD_ATOMIC_ADD(L.acc[0], e0 + e1);
		}
		if (lane == 0) GDD_ATOMIC_ADD(L.freq[256], 1u); // the end-of-block code
	}
	gdd_build_lengths(L.freq, GDD_NLIT, 15, L.lens, L.build, cuts);
	gdd_build_lengths(L.freq + GDD_LITS, GDD_NDIST, 15, L.lens + GDD_LITS, L.build, cuts ? cuts + 1 : nullptr);
	uint32_t hlit = GDD_NLIT, hdist = GDD_NDIST;
	GDD_ROLLED while (hlit > 257 && GDD_UNI(L.lens[hlit - 1]) == 0) --hlit;
	GDD_ROLLED while (hdist > 1 && GDD_UNI(L.lens[GDD_LITS + hdist - 1]) == 0) --hdist;
	// the code lengths of both codes as one sequence of symbols of the code-length code: runs of zeros become 17 (3..10) and 18 (11..138)
	GDD_LANES(lane) if (lane == 0) {
		const uint32_t n = hlit + hdist;
		uint32_t k = 0;
		GDD_ROLLED for (uint32_t i = 0; i < n;) {
			const uint32_t v = L.lens[i < hlit ? i : GDD_LITS + (i - hlit)];
			uint32_t run = 1;
			if (v == 0) GDD_ROLLED while (i + run < n && run < 138 && L.lens[i + run < hlit ? i + run : GDD_LITS + (i + run - hlit)] == 0) ++run;
			if (run >= 11) L.clsym[k++] = (uint16_t)(18u | (run - 11u) << 8), L.clfreq[18]++;
			else if (run >= 3) L.clsym[k++] = (uint16_t)(17u | (run - 3u) << 8), L.clfreq[17]++;
			else run = 1, L.clsym[k++] = (uint16_t)v, L.clfreq[v]++;
			i += run;
		}
		L.ncl = k;
		// zlib wants the code-length code complete: a second symbol beside a lone one (its one bit is counted below, and never sent)
		uint32_t nz = 0;
		GDD_ROLLED for (uint32_t s = 0; s < GDD_NCL; ++s) nz += L.clfreq[s] != 0;
		if (nz < 2) L.clfreq[L.clfreq[0] ? 1 : 0] = 1;
	}
	gdd_build_lengths(L.clfreq, GDD_NCL, 7, L.cllens, L.build, cuts ? cuts + 2 : nullptr);
	gdd_make_codes(L.cllens, GDD_NCL, L.clcode, L.build);
	const char *const order = "\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f"; // RFC 1951, 3.2.7
	uint32_t hclen = GDD_NCL;
	GDD_ROLLED while (hclen > 4 && GDD_UNI(L.cllens[(uint32_t)order[hclen - 1]]) == 0) --hclen;
	// the exact sizes (the dynamic one may count the one bit of the note above too much: an upper bound is what W2 needs)
	GDD_LANES(lane) {
		uint32_t dyn = 0, fix = 0;
		GDD_ROLLED for (uint32_t s = lane; s < GDD_LITS + 32; s += 64) {
			const uint32_t f = L.freq[s];
			dyn += f * L.lens[s], fix += f * (s < GDD_LITS ? gdd_fixed_len(s) : 5u);
		}
		if (lane < GDD_NCL) dyn += L.clfreq[lane] * (L.cllens[lane] + (lane == 17 ? 3u : lane == 18 ? 7u : 0u));
		GDD_ATOMIC_ADD(L.acc[1], dyn), GDD_ATOMIC_ADD(L.acc[2], fix);
	}
	GDD_WAVE_FENCE();
	const uint32_t xbits = GDD_UNI(L.acc[0]), dyn = 3u + 14u + 3u * hclen + GDD_UNI(L.acc[1]) + xbits, fix = 3u + GDD_UNI(L.acc[2]) + xbits;
	const bool fixed = fix <= dyn;
	const uint32_t ncl = GDD_UNI(L.ncl), so_far = O.words * 32u + O.bits - 8u * GDD_HEAD;
	if ((so_far + (fixed ? fix : dyn) + 7u) / 8u >= 5u + in_len) return false;
	if (fixed) {
		GDD_LANES(lane) GDD_ROLLED for (uint32_t s = lane; s < GDD_LITS + 32; s += 64) L.lens[s] = (uint8_t)(s < GDD_LITS ? gdd_fixed_len(s) : 5u);
	}
	gdd_make_codes(L.lens, fixed ? GDD_LITS : GDD_NLIT, L.code, L.build); // (the fixed code numbers 288 and 32 symbols)
	gdd_make_codes(L.lens + GDD_LITS, fixed ? 32 : GDD_NDIST, L.code + GDD_LITS, L.build);
	gdd_put(L, O, last ? 1u : 0u, 1), gdd_put(L, O, fixed ? 1u : 2u, 2);
	if (!fixed) {
		gdd_put(L, O, hlit - 257u, 5), gdd_put(L, O, hdist - 1u, 5), gdd_put(L, O, hclen - 4u, 4);
		GDD_ROLLED for (uint32_t i = 0; i < hclen; ++i) gdd_put(L, O, GDD_UNI(L.cllens[(uint32_t)order[i]]), 3);
		GDD_ROLLED for (uint32_t base = 0; base < ncl; base += 64) {
			GDD_WAVE_FENCE();
			GDD_LANES(lane) {
				uint32_t bits = 0, nb = 0;
				if (base + lane < ncl) {
					const uint32_t c = L.clsym[base + lane], s = c & 255u, l = L.cllens[s];
					bits = (uint32_t)L.clcode[s] | (c >> 8) << l, nb = l + (s == 17 ? 3u : s == 18 ? 7u : 0u);
				}
				L.eb_lo[lane] = bits, L.eb_hi[lane] = 0, L.nb[lane] = nb;
			}
			gdd_emit_chunk(L, O);
		}
	}
	GDD_ROLLED for (uint32_t base = 0; base < ntok; base += 64) {
		GDD_WAVE_FENCE();
		GDD_LANES(lane) {
			uint64_t bits = 0;
			uint32_t nb = 0;
			if (base + lane < ntok) {
				const uint32_t t = L.tok[base + lane];
				if (!(t >> 31)) bits = L.code[t & 255u], nb = L.lens[t & 255u];
				else {
					uint32_t e0, v0, e1, v1;
					const uint32_t ls = 257u + gdd_len_sym((t >> 15) & 255u, &e0, &v0), ds = GDD_LITS + gdd_dist_sym(t & 32767u, &e1, &v1);
					bits = L.code[ls], nb = L.lens[ls];
					bits |= (uint64_t)v0 << nb, nb += e0;
					bits |= (uint64_t)L.code[ds] << nb, nb += L.lens[ds];
					bits |= (uint64_t)v1 << nb, nb += e1;
				}
			}
			L.eb_lo[lane] = (uint32_t)bits, L.eb_hi[lane] = (uint32_t)(bits >> 32), L.nb[lane] = nb;
		}
		gdd_emit_chunk(L, O);
	}
	gdd_put(L, O, GDD_UNI(L.code[256]), GDD_UNI(L.lens[256]));
	return true;
}

// ---- one member --------------------------------------------------------------------------------------------------------------------
GDD_HD void gdd_start(GddLds &L, GddOut &O)
{
	GDD_WAVE_FENCE();
	GDD_LANES(lane) GDD_ROLLED for (uint32_t w = lane; w < GDD_OBUF; w += 64) L.obuf[w] = 0;
	GDD_WAVE_FENCE();
	O.bits = 0, O.words = 0;
	gdd_put_head(L, O);
}

// in[0, in_len) -> the complete BGZF member at slot[0, *member_len) (slot: GDD_SLOT bytes, 16-byte aligned; the bytes of its last word
// behind the member are zero).  Returns GDD_OK, or GDD_E_LEN for in_len above 65280 (nothing is written then).  Every lane of the
// wavefront calls it with the same arguments.  cuts: see gdd_block.
GDD_HD uint32_t gdd_deflate(GddLds &L, const uint8_t *in, uint32_t in_len, uint8_t *slot, uint32_t *member_len, uint32_t *cuts = nullptr)
{
	*member_len = 0;
	if (in_len > GDD_MAX_IN) return GDD_E_LEN;
	GddOut O = {(uint32_t *)(void *)slot, 0, 0};
	// the input to local memory, 16 bytes per lane where they lie inside it (W1), and an empty hash table
	GDD_WAVE_FENCE();
	GDD_LANES(lane) {
		GDD_ROLLED for (uint32_t at = lane * 16; at < in_len; at += 1024) {
			if (at + 16 <= in_len) { GddV16 v; memcpy(&v, in + at, 16); *(GddV16 *)(void *)(L.in + at) = v; }
			else GDD_ROLLED for (uint32_t j = at; j < in_len; ++j) L.in[j] = in[j];
		}
		GDD_ROLLED for (uint32_t h = lane; h < (1u << GDD_HASH_BITS); h += 64) L.head[h] = 0;
	}
	GDD_WAVE_FENCE();
	const uint32_t crc = gdd_crc32(L, in_len);
	gdd_start(L, O);
	uint32_t cur = 0, ntok = 0;
	bool stored = false, ended = false;
	// (an empty input takes one turn too: its block holds the end-of-block code alone)
	for (uint32_t base = 0; (base < in_len || in_len == 0) && !stored && !ended; base += 64) {
		const bool search = cur < base + 64; // (a group that a match has covered is only inserted)
		GDD_WAVE_FENCE();
		GDD_LANES(lane) {
			const uint32_t p = base + lane;
			uint32_t len = 0, dist = 0;
			if (search && p >= cur && p + GDD_MIN_MATCH <= in_len) { // (W1)
				const uint32_t h = (((uint32_t)L.in[p] | (uint32_t)L.in[p + 1] << 8 | (uint32_t)L.in[p + 2] << 16) * 0x9e3779b1u) >> (32 - GDD_HASH_BITS);
				const uint32_t c = L.head[h];
				if (c && p - (c - 1) <= GDD_MAX_DIST) { // (W3: c - 1 is a position of this member, in front of this group)
					const uint32_t q = c - 1, maxl = in_len - p < GDD_MAX_MATCH ? in_len - p : (uint32_t)GDD_MAX_MATCH;
					uint32_t l = 0;
					GDD_ROLLED while (l < maxl && L.in[q + l] == L.in[p + l]) ++l;
					if (l > GDD_MIN_MATCH || (l == GDD_MIN_MATCH && p - q <= GDD_FAR)) len = l, dist = p - q;
				}
			}
			L.mlen[lane] = len, L.mdist[lane] = dist;
		}
		GDD_WAVE_FENCE();
		GDD_LANES(lane) {
			const uint32_t p = base + lane;
			if (p + GDD_MIN_MATCH <= in_len) {
				const uint32_t h = (((uint32_t)L.in[p] | (uint32_t)L.in[p + 1] << 8 | (uint32_t)L.in[p + 2] << 16) * 0x9e3779b1u) >> (32 - GDD_HASH_BITS);
				GDD_ATOMIC_MAX(L.head[h], p + 1);
			}
		}
		GDD_WAVE_FENCE();
		const uint32_t end = base + 64 < in_len ? base + 64 : in_len;
		for (;;) { // (W4: every turn that does not end the loop moves cur on by at least one)
			if (ntok == GDD_TOK || cur >= in_len) {
				ended = cur >= in_len;
				stored = !gdd_block(L, O, ntok, ended, in_len, cuts);
				ntok = 0;
			}
			if (cur >= end || stored) break;
			const uint32_t len = GDD_UNI(L.mlen[cur - base]);
			const uint32_t t = len ? 0x80000000u | (len - 3u) << 15 | (GDD_UNI(L.mdist[cur - base]) - 1u) : (uint32_t)GDD_UNI(L.in[cur]);
			GDD_LANES(lane) if (lane == 0) L.tok[ntok] = t;
			cur += len ? len : 1u, ++ntok;
		}
	}
	if (!stored) {
		gdd_put(L, O, 0u, (0u - O.bits) & 7u);
		stored = (O.words * 32u + O.bits) / 8u - GDD_HEAD >= 5u + in_len;
	}
	if (stored) { // one stored block: everything written so far is written again, behind what is on its way
		GDD_STORE_FENCE();
		gdd_start(L, O);
		gdd_put(L, O, 1u, 8), gdd_put(L, O, in_len, 16), gdd_put(L, O, in_len ^ 0xffffu, 16);
		GDD_ROLLED for (uint32_t base = 0; base < in_len; base += 256) {
			GDD_WAVE_FENCE();
			GDD_LANES(lane) {
				const uint32_t at = base + lane * 4;
				uint32_t v = 0, k = 0;
				GDD_ROLLED for (; k < 4 && at + k < in_len; ++k) v |= (uint32_t)L.in[at + k] << (8 * k);
				L.eb_lo[lane] = v, L.eb_hi[lane] = 0, L.nb[lane] = 8 * k;
			}
			gdd_emit_chunk(L, O);
		}
	}
	gdd_put(L, O, crc, 32), gdd_put(L, O, in_len, 32);
	const uint32_t total = (O.words * 32u + O.bits) / 8u;
	gdd_flush(L, O, true);
	GDD_LANES(lane) if (lane == 0) L.keep[4] |= total - 1u; // BSIZE, bytes 16 and 17
	GDD_WAVE_FENCE();
	GDD_LANES(lane) if (lane < GDD_KEEP) O.dst[lane] = L.keep[lane];
	*member_len = total;
	return GDD_OK;
}
