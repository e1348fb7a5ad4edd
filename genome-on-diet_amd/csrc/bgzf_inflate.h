// A DEFLATE (RFC 1951) decoder for one BGZF member per wavefront: the statements, written once for the kernel (bgzf_inflate.hip.h) and
// for the host emulator that runs them as loops over 64 lanes (tests/emul/bgzf_emul.cpp).  No HIP in here.
//
// HOW THE WORK IS SPLIT.  The symbol loop is a serial chain (the position of a code depends on the length of the one before it), so it runs
// under wave-uniform control: bit buffer, positions and the symbol are kept uniform (GDZ_UNI: readfirstlane on the device, so that the
// chain lives in scalar registers), and all 64 lanes follow the same path.  The lanes work together where there is something to share out:
//   * the input is fetched 1 KiB at a time, 16 bytes per lane, into a two-slot ring in local memory, and the bit buffer is refilled from there;
//   * the decode tables of a block are built together: lane l counts and places the codes of length l, and every lane fills 1/64 of each
//     lookup table by decoding the table's own index with the canonical by-length walk -- the same walk that is the slow path for codes
//     longer than the table's index (10 bits literal/length, 8 bits distance, 7 bits code-length code);
//   * a match is copied by all lanes: lane k writes out[pos + k] = out[pos - dist + k % dist] for k < len in steps of 64;
//   * the finished member is copied to global memory in aligned 16-byte pieces.
//
// THE OUTPUT IS STAGED IN LOCAL MEMORY, all of it (a member inflates to at most 64 KiB), and that settles the hazard of a copy reading
// what another lane of the wavefront stored one symbol earlier: literals and copies are local-memory instructions of ONE wavefront, which
// the LDS unit executes in the order they were issued, and a copy never reads a byte that the same instruction writes (lane k reads below
// pos, since k % dist < dist, and writes at or above pos).  What is left is to keep the compiler from moving one lane's load above another
// lane's store, which it cannot see as a dependence: GDZ_WAVE_FENCE, a wavefront-scope fence (no instruction; it only orders) in front of
// every copy and every phase of a table build.  Global memory is written once, at the end, and never read back.
//
// RULES THAT KEEP IT SAFE ON ANY INPUT BYTES (the emulator runs the same statements under ASan / UBSan on mutated and truncated members):
//   R1 every read of the input is checked against in_len: whole 16-byte pieces only where they lie inside it, single bytes otherwise, and
//      the bit buffer never takes a byte at or behind in_len; a code that needs more bits than are left is GDZ_E_INPUT;
//   R2 every write is checked against [0, isize) of the member's output (GDZ_E_OUTPUT in the symbol loop; the final copy writes exactly
//      out[0, pos) with pos <= isize);
//   R3 a distance that reaches in front of the member's first byte is GDZ_E_DIST;
//   R4 every iteration of every loop consumes at least one input bit or produces at least one output byte: a block header is 3 bits, a code
//      is at least 1 bit, a repeat of code lengths advances by at least 3 -- and both are bounded, so the decoder ends on garbage;
//   R5 a set of code lengths is refused (GDZ_E_LENS) when it is over-subscribed, or incomplete and not a single code of length 1 (zlib's
//      rule, inflate_table), or has no end-of-block code, so the by-length walk never indexes past the symbols it was given.
//
// LOCAL MEMORY: GdzLds is 65552 (output) + 2048 (input ring) + 2816 (lookup tables) + 1920 (by-length tables) + 320 (code lengths) bytes
// = 72656 bytes per wavefront: two wavefronts per CU of 160 KiB, 512 on the device.  A read of 8 MiB is about 130 members, so the
// footprint does not limit anything: the device is short of members, not of room.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define GDZ_HD __host__ __device__ __forceinline__
#else
#define GDZ_HD static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define GDZ_LANES(lane) for (uint32_t lane = threadIdx.x, once_ = 1; once_; once_ = 0)
#define GDZ_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#define GDZ_WAVE_FENCE() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront")
#define GDZ_ROLLED _Pragma("clang loop unroll(disable) vectorize(disable) interleave(disable)")
#else
#define GDZ_ROLLED
#define GDZ_LANES(lane) for (uint32_t lane = 0; lane < 64; ++lane)
#define GDZ_UNI(x) ((uint32_t)(x))
#define GDZ_WAVE_FENCE() ((void)0)
#endif

enum { GDZ_OK = 0, GDZ_E_INPUT = 1, GDZ_E_BTYPE = 2, GDZ_E_STORED = 3, GDZ_E_LENS = 4, GDZ_E_CODE = 5, GDZ_E_DIST = 6, GDZ_E_OUTPUT = 7, GDZ_E_ISIZE = 8 };
static inline const char *gdz_strerror(uint32_t rc)
{
	static const char *const t[] = {"ok", "the deflate stream ends before its last block does", "invalid block type", "stored block lengths do not match",
	                                "invalid set of code lengths", "invalid code", "distance too far back", "output longer than ISIZE", "ISIZE above 65536"};
	return rc < sizeof(t) / sizeof(t[0]) ? t[rc] : "unknown error";
}

enum { GDZ_WIN = 65536, GDZ_RING = 2048, GDZ_CHUNK = 1024, GDZ_LIT_BITS = 10, GDZ_DIST_BITS = 8, GDZ_CLEN_BITS = 7, GDZ_MAX_LIT = 288, GDZ_MAX_DIST = 32 };

struct alignas(16) GdzV16 { uint32_t w[4]; };
struct GdzTab { // canonical code by length: count[l] codes of length l, their symbols in sym[offs[l] ..) in symbol order
	uint16_t count[16], offs[16];
	uint16_t sym[GDZ_MAX_LIT];
};
struct GdzLds {
	alignas(16) uint8_t win[GDZ_WIN + 16]; // the member's output, shifted by (address of out) & 15 so that 16-byte pieces line up
	alignas(16) uint32_t ring[GDZ_RING / 4]; // input bytes [c * 1024, (c + 1) * 1024) in slot c & 1
	uint16_t lit[1 << GDZ_LIT_BITS], dist[1 << GDZ_DIST_BITS], clen[1 << GDZ_CLEN_BITS]; // (symbol << 4) | length; 0: not in this table
	GdzTab tl, td, tc;
	uint8_t lens[GDZ_MAX_LIT + GDZ_MAX_DIST];
};

// the canonical by-length walk over the low `maxb` bits of v (first bit of the code in bit 0): (symbol << 4) | length, or 0 if no code of
// at most maxb bits starts v.  index + code - first stays below the number of symbols of T because T's counts are not over-subscribed (R5).
GDZ_HD uint32_t gdz_walk(const GdzTab &T, uint32_t v, uint32_t maxb)
{
	int32_t code = 0, first = 0, index = 0;
	GDZ_ROLLED for (uint32_t len = 1; len <= maxb; ++len) {
		code |= (int32_t)(v & 1u), v >>= 1;
		const int32_t count = T.count[len];
		if (code - count < first) return (uint32_t)T.sym[index + (code - first)] << 4 | len;
		index += count, first += count, first <<= 1, code <<= 1;
	}
	return 0;
}

// Tables of the code whose lengths are lens[0, n) (n <= 288): T, and the lookup table tab of 2^bits entries.  Returns GDZ_OK or GDZ_E_LENS.
// strict: the code-length code, which zlib wants complete whatever it holds.
GDZ_HD uint32_t gdz_build(const uint8_t *lens, uint32_t n, GdzTab &T, uint16_t *tab, uint32_t bits, bool strict = false)
{
	GDZ_WAVE_FENCE();
	GDZ_LANES(lane) if (lane < 16) {
		uint32_t c = 0;
		GDZ_ROLLED for (uint32_t s = 0; s < n; ++s) c += lens[s] == lane;
		T.count[lane] = (uint16_t)(lane ? c : 0);
	}
	GDZ_WAVE_FENCE();
	int32_t left = 1;
	uint32_t total = 0, at = 0;
	bool over = false;
	GDZ_ROLLED for (uint32_t l = 1; l < 16; ++l) {
		const uint32_t c = GDZ_UNI(T.count[l]);
		left = (left << 1) - (int32_t)c;
		over |= left < 0;
		if (left < 0) left = 0; // (keeps the shift defined; the set is refused below)
		total += c;
	}
	if (over || (left > 0 && !(total == 0 || (!strict && total == 1 && GDZ_UNI(T.count[1]) == 1)))) return GDZ_E_LENS;
	GDZ_LANES(lane) if (lane == 0)
		GDZ_ROLLED for (uint32_t l = 0; l < 16; ++l) T.offs[l] = (uint16_t)at, at += T.count[l];
	GDZ_WAVE_FENCE();
	GDZ_LANES(lane) if (lane >= 1 && lane < 16) {
		uint32_t o = T.offs[lane];
		GDZ_ROLLED for (uint32_t s = 0; s < n; ++s) if (lens[s] == lane) T.sym[o++] = (uint16_t)s;
	}
	GDZ_WAVE_FENCE();
	GDZ_LANES(lane) GDZ_ROLLED for (uint32_t i = lane; i < (1u << bits); i += 64) tab[i] = (uint16_t)gdz_walk(T, i, bits);
	GDZ_WAVE_FENCE();
	return GDZ_OK;
}

struct GdzBits { // all of it wave-uniform
	uint64_t bb;
	uint32_t bc, ip, loaded_end; // bits in bb; input bytes moved into bb so far; the ring holds the bytes below loaded_end (of the last two chunks)
};

// input bytes [c * 1024, (c + 1) * 1024) into their slot of the ring, zero where the input has ended (R1)
GDZ_HD void gdz_load_chunk(GdzLds &L, const uint8_t *in, uint32_t in_len, uint32_t c)
{
	GDZ_WAVE_FENCE();
	GDZ_LANES(lane) {
		const uint32_t at = c * GDZ_CHUNK + lane * 16;
		GdzV16 v = {{0, 0, 0, 0}};
		if (at + 16 <= in_len) memcpy(&v, in + at, 16);
		else GDZ_ROLLED for (uint32_t j = 0; j < 16; ++j) if (at + j < in_len) {
			const uint32_t x = (uint32_t)in[at + j] << (8 * (j & 3)), q = j >> 2; // (no indexed access: the piece stays in registers)
			v.w[0] |= q == 0 ? x : 0u, v.w[1] |= q == 1 ? x : 0u, v.w[2] |= q == 2 ? x : 0u, v.w[3] |= q == 3 ? x : 0u;
		}
		*(GdzV16 *)(void *)&L.ring[(at & (GDZ_RING - 1)) >> 2] = v;
	}
	GDZ_WAVE_FENCE();
}
// at least 32 bits in the buffer unless the input is exhausted (exactly 32 when it was empty)
GDZ_HD void gdz_refill(GdzLds &L, const uint8_t *in, uint32_t in_len, GdzBits &B)
{
	if (B.bc > 32 || B.ip >= in_len) return;
	while (B.ip + 4 > B.loaded_end && B.loaded_end < in_len) gdz_load_chunk(L, in, in_len, B.loaded_end / GDZ_CHUNK), B.loaded_end += GDZ_CHUNK;
	const uint32_t n = in_len - B.ip < 4 ? in_len - B.ip : 4, idx = (B.ip & (GDZ_RING - 1)) >> 2;
	const uint32_t w0 = GDZ_UNI(L.ring[idx]), w1 = GDZ_UNI(L.ring[(idx + 1) & (GDZ_RING / 4 - 1)]);
	uint32_t v = (uint32_t)(((uint64_t)w1 << 32 | w0) >> (8 * (B.ip & 3)));
	if (n < 4) v &= (1u << (8 * n)) - 1u;
	B.bb |= (uint64_t)v << B.bc, B.bc += 8 * n, B.ip += n;
}
GDZ_HD bool gdz_need(GdzLds &L, const uint8_t *in, uint32_t in_len, GdzBits &B, uint32_t n) // n <= 32
{
	gdz_refill(L, in, in_len, B);
	return B.bc >= n;
}
GDZ_HD uint32_t gdz_take(GdzBits &B, uint32_t n) // n <= 32 bits that gdz_need has seen
{
	const uint32_t v = (uint32_t)(B.bb & (((uint64_t)1 << n) - 1));
	B.bb >>= n, B.bc -= n;
	return v;
}
// the next symbol of a code: its lookup table, then the walk; 0xffffffff with *rc set if there is none
GDZ_HD uint32_t gdz_symbol(GdzLds &L, const uint8_t *in, uint32_t in_len, GdzBits &B, const uint16_t *tab, uint32_t bits, const GdzTab &T, uint32_t *rc)
{
	gdz_refill(L, in, in_len, B);
	uint32_t e = GDZ_UNI(tab[(uint32_t)B.bb & ((1u << bits) - 1u)]);
	if (!(e & 15u)) e = GDZ_UNI(gdz_walk(T, (uint32_t)B.bb, 15));
	if (!(e & 15u)) { *rc = B.bc < 15 ? GDZ_E_INPUT : GDZ_E_CODE; return 0xffffffffu; }
	if ((e & 15u) > B.bc) { *rc = GDZ_E_INPUT; return 0xffffffffu; }
	B.bb >>= (e & 15u), B.bc -= (e & 15u);
	return e >> 4;
}

GDZ_HD uint32_t gdz_len_base(uint32_t s) // s = symbol - 257, 0 .. 28
{
	return s < 8 ? 3 + s : s == 28 ? 258 : 3 + ((4 + (s & 3)) << ((s >> 2) - 1));
}
GDZ_HD uint32_t gdz_len_extra(uint32_t s) { return s < 8 || s == 28 ? 0 : (s >> 2) - 1; }
GDZ_HD uint32_t gdz_dist_base(uint32_t s) // 0 .. 29
{
	return s < 4 ? 1 + s : 1 + ((2 + (s & 1)) << ((s >> 1) - 1));
}
GDZ_HD uint32_t gdz_dist_extra(uint32_t s) { return s < 4 ? 0 : (s >> 1) - 1; }

// One member: in[0, in_len) is its deflate stream, out[0, isize) the place of its output.  Returns GDZ_OK or the error, and in *out_len
// the bytes produced (written to out only when the stream was decoded to its end without error).  Every lane of the wavefront calls it
// with the same arguments.
GDZ_HD uint32_t gdz_inflate(GdzLds &L, const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t isize, uint32_t *out_len)
{
	*out_len = 0;
	if (isize > GDZ_WIN) return GDZ_E_ISIZE;
	const uint32_t pad = (uint32_t)((uintptr_t)out & 15u);
	uint8_t *const win = L.win + pad;
	GdzBits B = {0, 0, 0, 0};
	uint32_t op = 0, rc = GDZ_OK;
	bool fixed_built = false;
	for (bool last = false; !last && rc == GDZ_OK;) {
		if (!gdz_need(L, in, in_len, B, 3)) { rc = GDZ_E_INPUT; break; }
		last = gdz_take(B, 1) != 0;
		const uint32_t type = gdz_take(B, 2);
		if (type == 3) { rc = GDZ_E_BTYPE; break; }
		if (type == 0) {
			gdz_take(B, B.bc & 7u); // to the byte boundary
			if (!gdz_need(L, in, in_len, B, 32)) { rc = GDZ_E_INPUT; break; }
			const uint32_t len = gdz_take(B, 16), nlen = gdz_take(B, 16);
			if ((len ^ 0xffffu) != nlen) { rc = GDZ_E_STORED; break; }
			const uint32_t from = B.ip - B.bc / 8; // the buffer holds whole bytes now: in[from, ip)
			if (len > in_len - from) { rc = GDZ_E_INPUT; break; }
			if (len > isize - op) { rc = GDZ_E_OUTPUT; break; }
			GDZ_WAVE_FENCE();
			GDZ_LANES(lane) GDZ_ROLLED for (uint32_t k = lane; k < len; k += 64) win[op + k] = in[from + k];
			op += len;
			// go on behind the stored bytes: the ring restarts with the chunk that holds the next byte
			B.bb = 0, B.bc = 0, B.ip = from + len, B.loaded_end = B.ip / GDZ_CHUNK * GDZ_CHUNK;
			continue;
		}
		if (type == 1) {
			if (!fixed_built) {
				GDZ_WAVE_FENCE();
				GDZ_LANES(lane) {
					for (uint32_t s = lane; s < GDZ_MAX_LIT; s += 64) L.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
					if (lane < GDZ_MAX_DIST) L.lens[GDZ_MAX_LIT + lane] = 5;
				}
				gdz_build(L.lens, GDZ_MAX_LIT, L.tl, L.lit, GDZ_LIT_BITS);
				gdz_build(L.lens + GDZ_MAX_LIT, GDZ_MAX_DIST, L.td, L.dist, GDZ_DIST_BITS);
				fixed_built = true;
			}
		} else {
			fixed_built = false;
			if (!gdz_need(L, in, in_len, B, 14)) { rc = GDZ_E_INPUT; break; }
			const uint32_t hlit = gdz_take(B, 5) + 257, hdist = gdz_take(B, 5) + 1, hclen = gdz_take(B, 4) + 4;
			if (hlit > 286 || hdist > 30) { rc = GDZ_E_LENS; break; }
			GDZ_WAVE_FENCE();
			GDZ_LANES(lane) if (lane < 19) L.lens[lane] = 0;
			GDZ_WAVE_FENCE();
			for (uint32_t i = 0; i < hclen && rc == GDZ_OK; ++i) {
				if (!gdz_need(L, in, in_len, B, 3)) { rc = GDZ_E_INPUT; break; }
				const uint32_t sym = (uint32_t)"\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f"[i]; // the order of RFC 1951, 3.2.7
				L.lens[sym] = (uint8_t)gdz_take(B, 3);
			}
			if (rc != GDZ_OK) break;
			if ((rc = gdz_build(L.lens, 19, L.tc, L.clen, GDZ_CLEN_BITS, true)) != GDZ_OK) break;
			// the code lengths of both codes as one sequence: a repeat may run across the boundary
			const uint32_t n = hlit + hdist;
			uint32_t prev = 0;
			for (uint32_t i = 0; i < n && rc == GDZ_OK;) {
				const uint32_t s = gdz_symbol(L, in, in_len, B, L.clen, GDZ_CLEN_BITS, L.tc, &rc);
				if (rc != GDZ_OK) break;
				if (s < 16) { L.lens[i++] = (uint8_t)s, prev = s; continue; }
				uint32_t rep, val = 0;
				if (s == 16) {
					if (i == 0) { rc = GDZ_E_LENS; break; }
					if (!gdz_need(L, in, in_len, B, 2)) { rc = GDZ_E_INPUT; break; }
					val = prev, rep = 3 + gdz_take(B, 2);
				} else if (s == 17) {
					if (!gdz_need(L, in, in_len, B, 3)) { rc = GDZ_E_INPUT; break; }
					rep = 3 + gdz_take(B, 3);
				} else {
					if (!gdz_need(L, in, in_len, B, 7)) { rc = GDZ_E_INPUT; break; }
					rep = 11 + gdz_take(B, 7);
				}
				if (i + rep > n) { rc = GDZ_E_LENS; break; }
				GDZ_ROLLED for (uint32_t k = 0; k < rep; ++k) L.lens[i++] = (uint8_t)val;
				prev = val;
			}
			if (rc != GDZ_OK) break;
			GDZ_WAVE_FENCE();
			if (GDZ_UNI(L.lens[256]) == 0) { rc = GDZ_E_LENS; break; } // no end-of-block code
			if ((rc = gdz_build(L.lens, hlit, L.tl, L.lit, GDZ_LIT_BITS)) != GDZ_OK) break;
			if ((rc = gdz_build(L.lens + hlit, hdist, L.td, L.dist, GDZ_DIST_BITS)) != GDZ_OK) break;
		}
		// the symbol loop of a compressed block
		for (;;) {
			const uint32_t s = gdz_symbol(L, in, in_len, B, L.lit, GDZ_LIT_BITS, L.tl, &rc);
			if (rc != GDZ_OK) break;
			if (s < 256) {
				if (op >= isize) { rc = GDZ_E_OUTPUT; break; }
				win[op++] = (uint8_t)s;
				continue;
			}
			if (s == 256) break;
			if (s > 285) { rc = GDZ_E_CODE; break; }
			const uint32_t le = gdz_len_extra(s - 257);
			if (B.bc < le) { rc = GDZ_E_INPUT; break; } // (a code is at most 15 bits of the 32 a refill leaves: 5 more are there unless the input has ended)
			const uint32_t len = gdz_len_base(s - 257) + gdz_take(B, le);
			const uint32_t ds = gdz_symbol(L, in, in_len, B, L.dist, GDZ_DIST_BITS, L.td, &rc);
			if (rc != GDZ_OK) break;
			if (ds > 29) { rc = GDZ_E_CODE; break; }
			const uint32_t de = gdz_dist_extra(ds);
			if (B.bc < de) { rc = GDZ_E_INPUT; break; } // (15 + 13 bits of at least 32, likewise)
			const uint32_t dist = gdz_dist_base(ds) + gdz_take(B, de);
			if (dist > op) { rc = GDZ_E_DIST; break; }
			if (len > isize - op) { rc = GDZ_E_OUTPUT; break; }
			GDZ_WAVE_FENCE();
			const uint8_t *src = win + (op - dist);
			if (dist >= len) { GDZ_LANES(lane) GDZ_ROLLED for (uint32_t k = lane; k < len; k += 64) win[op + k] = src[k]; }
			else { GDZ_LANES(lane) GDZ_ROLLED for (uint32_t k = lane; k < len; k += 64) win[op + k] = src[k % dist]; }
			op += len;
		}
	}
	*out_len = op;
	if (rc != GDZ_OK) return rc;
	// the member to its place: aligned 16-byte pieces of L.win[pad, pad + op) = out[0, op), single bytes at the two ends (R2: op <= isize)
	GDZ_WAVE_FENCE();
	GDZ_LANES(lane) GDZ_ROLLED for (uint32_t a = lane * 16; a < pad + op; a += GDZ_CHUNK) {
		if (a >= pad && a + 16 <= pad + op) *(GdzV16 *)(void *)(out + (a - pad)) = *(const GdzV16 *)(const void *)(L.win + a);
		else GDZ_ROLLED for (uint32_t j = a < pad ? pad : a; j < a + 16 && j < pad + op; ++j) out[j - pad] = L.win[j];
	}
	return GDZ_OK;
}
