// K1 (register-resident form): the per-lane arithmetic of the wavefront ksw_extd2 kernel, written once for the
// device kernel (ksw_wave.hip.h) and for the host lock-step emulator used by tests/test_wave_emulator.py.
//
// Mapping (HiFi geometry, w = 1000): one 64-lane wavefront per alignment.  The reference's 16-lane SSE block
// [16m, 16m+15] of target positions is ONE GPU lane; lane = m mod 64, so the 64 lanes always hold the 64
// consecutive blocks [st_, st_+63] that can be touched by an anti-diagonal (n_col_ <= 64).  A lane therefore is
// either wholly inside the reference's 16-aligned computed window [st, en] or wholly outside it, which makes the
// reference's padding-cell behaviour (SURVEY Notes K1.1-K1.3) fall out of plain lane predication.
//
// Per lane the 16 cells are held as 8 packed registers per state array: register k = (cell k | cell k+8 << 16),
// so "row r-1, cell t-1" is register k-1 (no instruction) except for k = 0, which takes one DPP rotate from the
// previous lane plus one v_alignbit.  Arithmetic is packed 16-bit (v_pk_add/sub/max/min_i16): two cells per VALU
// instruction.  Values are kept as KEYS  8*value + tie + bias:
//     U,V: 8u+B1, 8v+B1      X: 8x+3+B1   Y: 8y+2+B1   X2: 8x2+1+B2   Y2: 8y2+B2      S: 8s+4+2*B1
//     B1 = 8*(q+e-1), B2 = 8*(q2+e2-1)
//   * a = X+V, b = Y+U carry bias 2*B1, a2 = X2+V, b2 = Y2+U carry B1+B2; with c2 = B1-B2 added to max(a2,b2) all
//     five candidates carry bias 2*B1 and tie codes 4 (S),3,2,1,0, so a chain of packed max gives both z (key & ~7)
//     and the reference's direction d = 4 - (key & 7): the strict-'>' priority order z,a,b,a2,b2 of
//     SR/ksw2_extd2_sse.c:235-242 is "largest value, then largest tie code".
//   * with B1 = 8(q+e-1) the no-continuation value x = -(q+e) is key -5 (y: -6) and every continuation value is
//     >= 0 (x2 = -(q2+e2): key -7, y2: -8 thanks to B2), so all four E/F continuation flags (:263-272) are the sign
//     bits of the stored X/Y/X2/Y2 registers.
// 8-bit wrap-around of the reference cannot occur for parameters accepted by gd_wave_supported() (all keys stay
// far inside int16), so 16-bit arithmetic reproduces the int8 results exactly; the emulator test and the GPU
// parity tests check that against the oracle.
//
// The score (approximate-max walk, :367-383) is obtained from the identity H(r,t)-H(r-1,t) = v(r,t),
// H(r,t+1)-H(r,t) = u(r,t+1)-v(r,t): the sum along ANY monotone in-band path from (0,0) to the last cell equals
// the reference's H0 (each unit square between two such paths contributes u+v'=v+u' identically, because both
// u(r,t) and v(r,t) are z minus the stored neighbours).  Each lane tracks 8*H at its cell 0; see gdw_track_*.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "ksw_common.h"

#if defined(__HIPCC__)
#define GDW_HD __host__ __device__ __forceinline__
#else
#define GDW_HD static inline
#endif

typedef uint32_t u32;

// ---- packed 16-bit helpers ---------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
typedef short gdw_v2s __attribute__((ext_vector_type(2)));
GDW_HD gdw_v2s gdw_as_v(u32 a) { return __builtin_bit_cast(gdw_v2s, a); }
GDW_HD u32 gdw_as_u(gdw_v2s a) { return __builtin_bit_cast(u32, a); }
GDW_HD u32 pk_add(u32 a, u32 b) { return gdw_as_u(gdw_as_v(a) + gdw_as_v(b)); }
GDW_HD u32 pk_sub(u32 a, u32 b) { return gdw_as_u(gdw_as_v(a) - gdw_as_v(b)); }
GDW_HD u32 pk_max(u32 a, u32 b) { return gdw_as_u(__builtin_elementwise_max(gdw_as_v(a), gdw_as_v(b))); }
GDW_HD u32 pk_min(u32 a, u32 b) { return gdw_as_u(__builtin_elementwise_min(gdw_as_v(a), gdw_as_v(b))); }
GDW_HD u32 gdw_perm(u32 s0, u32 s1, u32 sel) { return __builtin_amdgcn_perm(s0, s1, sel); }
GDW_HD u32 gdw_alignbit(u32 hi, u32 lo, u32 sh) { return __builtin_amdgcn_alignbit(hi, lo, sh); }
GDW_HD u32 gdw_alignbyte(u32 hi, u32 lo, u32 sh) { return __builtin_amdgcn_alignbyte(hi, lo, sh); }
#else
GDW_HD u32 pk_add(u32 a, u32 b) { return ((a + b) & 0xffffu) | ((((a >> 16) + (b >> 16)) & 0xffffu) << 16); }
GDW_HD u32 pk_sub(u32 a, u32 b) { return ((a - b) & 0xffffu) | ((((a >> 16) - (b >> 16)) & 0xffffu) << 16); }
GDW_HD u32 pk_max(u32 a, u32 b)
{
	int16_t al = (int16_t)a, bl = (int16_t)b, ah = (int16_t)(a >> 16), bh = (int16_t)(b >> 16);
	return (u32)(uint16_t)(al > bl ? al : bl) | (u32)(uint16_t)(ah > bh ? ah : bh) << 16;
}
GDW_HD u32 pk_min(u32 a, u32 b)
{
	int16_t al = (int16_t)a, bl = (int16_t)b, ah = (int16_t)(a >> 16), bh = (int16_t)(b >> 16);
	return (u32)(uint16_t)(al < bl ? al : bl) | (u32)(uint16_t)(ah < bh ? ah : bh) << 16;
}
GDW_HD u32 gdw_perm(u32 s0, u32 s1, u32 sel) // v_perm_b32: bytes 0-3 = s1, 4-7 = s0, 12 -> 0x00, >= 13 -> 0xff
{
	uint64_t src = (uint64_t)s0 << 32 | s1;
	u32 out = 0;
	for (int i = 0; i < 4; ++i) {
		u32 s = (sel >> (8 * i)) & 0xff, b;
		if (s <= 7) b = (u32)(src >> (8 * s)) & 0xff;
		else if (s == 12) b = 0;
		else if (s >= 13) b = 0xff;
		else b = ((src >> (16 * (s - 8) + 15)) & 1) ? 0xff : 0; // 8..11: sign of bytes 1,3,5,7 (unused here)
		out |= b << (8 * i);
	}
	return out;
}
GDW_HD u32 gdw_alignbit(u32 hi, u32 lo, u32 sh) { return (u32)((((uint64_t)hi << 32) | lo) >> (sh & 31)); }
GDW_HD u32 gdw_alignbyte(u32 hi, u32 lo, u32 sh) { return (u32)((((uint64_t)hi << 32) | lo) >> (8 * (sh & 3))); }
#endif
GDW_HD u32 gdw_bfi(u32 mask, u32 a, u32 b) { return (a & mask) | (b & ~mask); }
// the same with a wave-uniform mask (a constant, or derived from the anti-diagonal index): one v_bfi_b32 with the mask in an SGPR.
// The compiler splits the C form into v_and + v_and + v_or once the mask is a constant (~mask folds into a second constant).
#if defined(__HIP_DEVICE_COMPILE__)
GDW_HD u32 gdw_bfi_u(u32 mask, u32 a, u32 b)
{
	u32 d;
	asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(d) : "s"(mask), "v"(a), "v"(b));
	return d;
}
#else
GDW_HD u32 gdw_bfi_u(u32 mask, u32 a, u32 b) { return gdw_bfi(mask, a, b); }
#endif
// inside a wave-uniform `if`: the value passes through an empty asm statement, which the compiler neither removes nor executes
// speculatively, so the `if` stays a branch (host: nothing)
#if defined(__HIP_DEVICE_COMPILE__)
#define GDW_KEEP_BRANCH(v) asm volatile("" : "+v"(v))
#define GDW_RARE_S(s) asm volatile("" : "+s"(s)) // a wave-uniform value the compiler knows nothing about from here on
#else
#define GDW_KEEP_BRANCH(v) ((void)0)
#define GDW_RARE_S(s) ((void)0)
#endif
GDW_HD u32 gdw_pack2(int v) { return ((u32)v & 0xffffu) | ((u32)v << 16); }
GDW_HD int gdw_lo(u32 a) { return (int)(int16_t)(a & 0xffffu); }
GDW_HD int gdw_hi(u32 a) { return (int)(int16_t)(a >> 16); }

// ---- uniform constants -------------------------------------------------------------------------------------
struct WaveK {
	int32_t B1;                // 8*(q+e-1)
	u32 cx, cy, cx2, cy2;      // packed no-continuation / initial keys of X, Y, X2, Y2 (-5, -6, -7, -8)
	u32 c2;                    // packed B1 - B2: lifts max(a2, b2) to the bias of the other candidates
	u32 uv0;                   // packed initial key of U and V (value -(q+e))
	u32 zmax;                  // packed 8*sc_mch + 2*B1
	u32 te, te2;               // packed: tE = z8 - te (te = 8(q-1)); tE2 = z8 - te2 (te2 = B1 - 8*e2)
	u32 lut_lo, lut_hi;        // S-key bytes indexed by (T^Q)|TN: [match,mis,mis,mis] / [N,N,N,N]
	u32 s0;                    // S-key byte of score 0, replicated (the reference's zero-filled s[])
	int32_t key_open, key_e, key_ld, key_e2; // boundary keys of v1 / u[r]: -(q+e), -e, long_diff, -e2 (SR/ksw2_extd2_sse.c:158,162)
	int32_t long_thres;
	int32_t qe8;               // 8*(q+e)
};

static inline bool gdw_make_consts(const KswConst &C, WaveK &K)
{
	const int qe = C.q + C.e, qe2 = C.q2 + C.e2;
	K.B1 = 8 * (qe - 1);
	if (qe < 1) return false;
	K.cx = gdw_pack2(8 * -qe + 3 + K.B1), K.cy = gdw_pack2(8 * -qe + 2 + K.B1);
	const int B2 = 8 * (qe2 - 1);
	K.cx2 = gdw_pack2(8 * -qe2 + 1 + B2), K.cy2 = gdw_pack2(8 * -qe2 + B2);
	K.c2 = gdw_pack2(K.B1 - B2);
	K.uv0 = gdw_pack2(8 * -qe + K.B1);
	K.zmax = gdw_pack2(8 * C.sc_mch + 2 * K.B1);
	K.te = gdw_pack2(8 * (C.q - 1)), K.te2 = gdw_pack2(K.B1 - 8 * C.e2);
	const int km = 8 * C.sc_mch + 4 + 2 * K.B1, kx = 8 * C.sc_mis + 4 + 2 * K.B1, kn = 8 * C.sc_N + 4 + 2 * K.B1, k0 = 4 + 2 * K.B1;
	if (km < 0 || km > 255 || kx < 0 || kx > 255 || kn < 0 || kn > 255 || k0 > 255) return false; // S keys must fit a byte
	K.lut_lo = (u32)km | (u32)kx << 8 | (u32)kx << 16 | (u32)kx << 24;
	K.lut_hi = (u32)kn * 0x01010101u;
	K.s0 = (u32)k0 * 0x01010101u;
	K.key_open = 8 * -qe + K.B1, K.key_e = 8 * -C.e + K.B1, K.key_ld = 8 * C.long_diff + K.B1, K.key_e2 = 8 * -C.e2 + K.B1;
	K.long_thres = C.long_thres;
	K.qe8 = 8 * qe;
	// every key must stay well inside int16: |value| <= 127 => |key| <= 8*127 + 7 + 2*B1
	if (8 * 127 + 7 + 2 * K.B1 > 30000) return false;
	return true;
}

// boundary key of v1 (st == 0) and of u[r] (SR/ksw2_extd2_sse.c:158,162)
GDW_HD int gdw_edge_key(const WaveK &K, int r)
{
	return r == 0 ? K.key_open : r < K.long_thres ? K.key_e : r == K.long_thres ? K.key_ld : K.key_e2;
}

// ---- per-lane state ----------------------------------------------------------------------------------------
struct WaveLane {
	u32 U[8], V[8], X[8], Y[8], X2[8], Y2[8]; // packed keys, register k = cells (k, k+8) of the lane's block
	u32 Sb[4];   // S-key bytes, dword g = cells 4g..4g+3 (persistent: stale cells keep their old score)
	u32 Tb[4];   // target nt4 bytes of the block (0 beyond tlen)
	u32 Qc[4];   // query nt4 bytes facing the cells on the current anti-diagonal: cell i <-> query[r - (tb+i)]
	u32 SEL[4];  // v_perm selectors blending fresh scores into Sb (per byte: 4+i = take fresh, i = keep)
	u32 tn;      // != 0 iff the block's target bytes contain an N (4): only then the score index needs its N fix-up
	int32_t blk; // block index m held by the lane (m mod lanes == lane id)
	int32_t R;   // 8*H(r, 16m): score tracker at cell 0 of the block
};

// query byte facing cell t on anti-diagonal r; outside [0,qlen) the reference reads zeroed memory
GDW_HD u32 gdw_qbyte(const uint8_t *query, int qlen, int j) { return (j >= 0 && j < qlen) ? query[j] : 0u; }

// ---- the seam stream of the paired steady rows (gdw_quarter_rows, gdw_narrow_rows) ---------------------------------------------------
// The fresh query byte of a row is query[j], j = r - 16 pst_ (0 outside [0, qlen): gdw_seam_byte, ksw_wave.hip.h).  Over the paired rows j
// rises by one a row and steps back by 15 on the second row of a pair that took a block over: a sequential stream.  The stream keeps the
// aligned 8 bytes that hold query[j] (win, bytes outside the query zero) and the 8 after them (nxt), so a row takes its byte with a shift
// and no bounds test.  The row that enters a new window (byte 0 of it) moves nxt to win and loads the window after -- eight rows
// before its first byte is used, so no row waits for a load it has just issued.  16 pst_ is a multiple of 8: the byte's place in its
// window is (address of query + r) & 7 whatever pst_ is.  All of it is wave-uniform: scalar registers, and on the device one aligned dword
// load per four query bytes through the constant address space.  As in gdw_seam_byte, every dword loaded holds at least one byte of the
// query -- `query` may start at any byte alignment and its arena may end with its last dword.
// (tests/emul/seam_stream_test.cpp holds every paired row against gdw_qbyte and every load against that rule.)
#if defined(__HIP_DEVICE_COMPILE__)
GDW_HD u32 gdw_seam_load(const uint8_t *p /* 4-aligned, wave-uniform */)
{
	typedef const __attribute__((address_space(4))) u32 *gdw_const_u32p;
	return *(gdw_const_u32p)(uintptr_t)p;
}
GDW_HD uint64_t gdw_seam_load2(const uint8_t *p /* 8-aligned, wave-uniform */)
{
	typedef const __attribute__((address_space(4))) uint64_t *gdw_const_u64p;
	return *(gdw_const_u64p)(uintptr_t)p;
}
// what is before stays before: a window is taken out of nxt before the loads that overwrite nxt are issued, so they can land in its registers
#define GDW_SEAM_ORDER(w) asm volatile("" : "+s"(w) : : "memory")
#else
#ifndef GDW_SEAM_LOAD_HOOK
#define GDW_SEAM_LOAD_HOOK(p) ((void)0) // (a host test may look at every address the stream loads from)
#endif
GDW_HD u32 gdw_seam_load(const uint8_t *p)
{
	GDW_SEAM_LOAD_HOOK(p);
	return (u32)p[0] | (u32)p[1] << 8 | (u32)p[2] << 16 | (u32)p[3] << 24;
}
GDW_HD uint64_t gdw_seam_load2(const uint8_t *p) { return (uint64_t)gdw_seam_load(p + 4) << 32 | gdw_seam_load(p); }
#define GDW_SEAM_ORDER(w) ((void)0)
#endif
struct GdwSeam {
	uint64_t win; // the window of the row just served: byte k = query[jb + k], 0 at and beyond the query's end
	uint64_t nxt; // the 8 bytes after it as they were loaded; a dword that holds no byte of the query was not loaded and keeps what it held.
	              // Bytes beyond the query's end are cleared when the window moves to win, a window's worth of rows later: a refill only
	              // issues loads and uses nothing of them
};
// the two dwords of query[jb .. jb + 7], 0 <= jb, query + jb 8-aligned, into nxt; a dword without a byte of the query is not read
GDW_HD void gdw_seam_fetch(GdwSeam &S, const uint8_t *query, int qlen, int jb)
{
	if (jb + 4 < qlen) S.nxt = gdw_seam_load2(query + jb);
	else if (jb < qlen) S.nxt = gdw_seam_load(query + jb);
}
// ... and which of a window's bytes are below the query's end
GDW_HD uint64_t gdw_seam_inside(int qlen, int jb)
{
	int n = qlen - jb;
	n = n < 0 ? 0 : n > 8 ? 8 : n;
	return ~((~0ull << (4 * n)) << (4 * n)); // the low n bytes (in two steps: 8 n can be 64)
}
// The rows name their byte by (r, mb): j = r - 16 (mb >> 4), mb = m - 1 on the first row of a pair and m on the second (pst_ = mb >> 4).
// Whatever a refill works out from them stays inside its branch (GDW_RARE_S: the compiler would otherwise carry the window's address and
// index through every row as induction registers of their own); the steady row reads r only.
GDW_HD int gdw_seam_pos(const uint8_t *query, int r) { return (int)(((u32)(uintptr_t)query + (u32)r) & 7u); } // (16 (mb >> 4) is a multiple of 8)
// before the row (r, mb): the first paired row, and the second row of a pair that took a block over (the step back by 15).  The paired
// rows have r - 16 (mb >> 4) >= 17 (st0 >= 16 and a band of at least one cell), so no window starts below the query's first byte.
GDW_HD void gdw_seam_init(GdwSeam &S, const uint8_t *query, int qlen, int r, int mb)
{
	GDW_RARE_S(r);
	GDW_RARE_S(mb);
	const int pos = gdw_seam_pos(query, r);
	const int jb = r - ((mb >> 4) << 4) - pos - (pos == 0 ? 8 : 0); // (a row at byte 0 of a window moves nxt to win first)
	S.nxt = 0;
	gdw_seam_fetch(S, query, qlen, jb);
	S.win = S.nxt & gdw_seam_inside(qlen, jb);
	gdw_seam_fetch(S, query, qlen, jb + 8);
}
// the byte of row (r, mb), gdw_seam_byte(query, qlen, j); j is one more than on the call before, or what gdw_seam_init was called for
GDW_HD u32 gdw_seam_next(GdwSeam &S, const uint8_t *query, int qlen, int r, int mb)
{
	const int pos = gdw_seam_pos(query, r);
	if (pos == 0) {
		GDW_RARE_S(r);
		GDW_RARE_S(mb);
		const int j = r - ((mb >> 4) << 4);
		uint64_t w = S.nxt & gdw_seam_inside(qlen, j);
		GDW_SEAM_ORDER(w);
		S.win = w;
		gdw_seam_fetch(S, query, qlen, j + 8);
	}
	return (u32)(S.win >> (8 * pos)) & 0xffu;
}

// (re)load a lane for block m at anti-diagonal r: reference's initial fill (SR/ksw2_extd2_sse.c:107,111-116)
GDW_HD void gdw_load_block(WaveLane &L, const WaveK &K, int m, int r, const uint8_t *query, int qlen,
                           const uint8_t *target, int tlen)
{
	L.blk = m;
	const int tb = m << 4;
#pragma unroll
	for (int k = 0; k < 8; ++k) L.U[k] = K.uv0, L.V[k] = K.uv0, L.X[k] = K.cx, L.Y[k] = K.cy, L.X2[k] = K.cx2, L.Y2[k] = K.cy2;
#pragma unroll
	for (int g = 0; g < 4; ++g) {
		u32 tw = 0, qw = 0;
#pragma unroll
		for (int b = 0; b < 4; ++b) {
			const int t = tb + 4 * g + b;
			tw |= (t < tlen ? (u32)target[t] : 0u) << (8 * b);
			qw |= gdw_qbyte(query, qlen, r - t) << (8 * b);
		}
		L.Tb[g] = tw, L.Qc[g] = qw, L.Sb[g] = K.s0, L.SEL[g] = 0x03020100u;
	}
	L.tn = (L.Tb[0] | L.Tb[1] | L.Tb[2] | L.Tb[3]) & 0x04040404u;
	L.R = 0;
}

// the same for any block index (also below block 0 or beyond the target: the cone pass holds 64 consecutive blocks whatever they
// are); the query bytes are those facing the cells on anti-diagonal rq
GDW_HD void gdw_fresh_block(WaveLane &L, const WaveK &K, int blk, int rq, const uint8_t *query, int qlen, const uint8_t *target, int tlen)
{
	const int tb = blk * 16;
	L.blk = blk;
#pragma unroll
	for (int k = 0; k < 8; ++k) L.U[k] = K.uv0, L.V[k] = K.uv0, L.X[k] = K.cx, L.Y[k] = K.cy, L.X2[k] = K.cx2, L.Y2[k] = K.cy2;
#pragma unroll
	for (int g = 0; g < 4; ++g) {
		u32 tw = 0, qw = 0;
#pragma unroll
		for (int b = 0; b < 4; ++b) {
			const int t = tb + 4 * g + b;
			tw |= (t >= 0 && t < tlen ? (u32)target[t] : 0u) << (8 * b);
			qw |= gdw_qbyte(query, qlen, rq - t) << (8 * b);
		}
		L.Tb[g] = tw, L.Qc[g] = qw, L.Sb[g] = K.s0, L.SEL[g] = 0x03020100u;
	}
	L.tn = (L.Tb[0] | L.Tb[1] | L.Tb[2] | L.Tb[3]) & 0x04040404u;
	L.R = 0;
}

// uniform description of one anti-diagonal
struct WaveRow {
	int r, st0, en0, st_, en_, up;
	int use_array;   // boundary x1/x21/v1 come from the previous lane's row r-1 values (block st_-1 just retired)
	int v1key;       // otherwise: key of v1 (x1/x21 are always the no-continuation keys then)
	int set_tr;      // en >= r: cell t == r gets u/y/y2 reset (:160-163)
	int ukey;        // key of u[r] for that reset
	int m_first_valid = 0; // the caller already holds the lane mask "this lane's block is st_" (paired rows)
	u32 m_first = 0, m_first_h = 0; // (m_first_h: the same for a half block -- "the first half of block st_")
};

// selectors for the score blend of one lane: cells [st0, up) are rewritten (:166-180)
GDW_HD void gdw_make_sel(WaveLane &L, int st0, int up)
{
	const int tb = L.blk << 4;
	int lo = st0 - tb, hi = up - tb;
	lo = lo < 0 ? 0 : lo > 16 ? 16 : lo;
	hi = hi < 0 ? 0 : hi > 16 ? 16 : hi;
	const u32 bm = hi > lo ? (((1u << (hi - lo)) - 1u) << lo) : 0u; // bit i: cell i is rewritten
#pragma unroll
	for (int g = 0; g < 4; ++g) {
		const u32 n = (bm >> (4 * g)) & 15u;
		const u32 spread = (n * 0x00204081u) & 0x01010101u; // bit i of n -> bit 0 of byte i
		L.SEL[g] = 0x03020100u + (spread << 2);
	}
}

// The same selectors for the rows in the middle of a long alignment, where they depend on the lane only through its role: with
// d0 = st0 & 15, the lane of the lowest block st_ rewrites its cells >= d0, the lane of block top = up >> 4 its cells < d0 (up and
// st0 are congruent mod 16), the blocks between them all 16 cells and the blocks above top none.  The two selector sets are
// wave-uniform (scalar unit); a lane only picks.
GDW_HD void gdw_sel_uniform(int d0, u32 lo[4], u32 hi[4])
{
	const uint64_t C = 0x0404040404040404ull; // byte c of the 16-byte mask (f1:f0) = 4 iff cell c >= d0
	const uint64_t f0 = d0 < 8 ? C << (8 * d0) : 0ull, f1 = d0 < 8 ? C : C << (8 * (d0 - 8));
	lo[0] = 0x03020100u + (u32)f0, lo[1] = 0x03020100u + (u32)(f0 >> 32), lo[2] = 0x03020100u + (u32)f1, lo[3] = 0x03020100u + (u32)(f1 >> 32);
#pragma unroll
	for (int g = 0; g < 4; ++g) hi[g] = 0x0a080604u - lo[g]; // 0x03020100 + (0x04040404 - mask)
}
// (a select between two scalar values costs a copy into a vector register plus the select -- one scalar operand per instruction --
// so the picks are v_bfi_b32 with the scalar value as data and a 0 / ~0 lane mask; all_inside: no lane holds a block above top)
#if defined(__HIP_DEVICE_COMPILE__)
GDW_HD u32 gdw_bfi_s(u32 mask, u32 a_uniform, u32 b)
{
	u32 d;
	asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(d) : "v"(mask), "s"(a_uniform), "v"(b));
	return d;
}
#else
GDW_HD u32 gdw_bfi_s(u32 mask, u32 a_uniform, u32 b) { return gdw_bfi(mask, a_uniform, b); }
#endif
GDW_HD void gdw_pick_sel(WaveLane &L, int st_, int top, bool all_inside, const u32 lo[4], const u32 hi[4], u32 &m_lo)
{
	m_lo = L.blk == st_ ? ~0u : 0u;
	const u32 m_top = L.blk == top ? ~0u : 0u;
	u32 base = 0x07060504u;
	if (!all_inside) base = L.blk < top ? 0x07060504u : 0x03020100u;
#pragma unroll
	for (int g = 0; g < 4; ++g) L.SEL[g] = gdw_bfi_s(m_lo, lo[g], gdw_bfi_s(m_top, hi[g], base));
}

// advance the query window by one anti-diagonal: cell i now faces what cell i-1 faced.  Cell 0 takes the byte that cell 15
// of the block below faced on the previous anti-diagonal, i.e. the top byte of the previous lane's Qc[3] (`below`, fetched
// with the same DPP rotate as the DP state) -- the query streams through the lanes and no lane touches memory.  Only the
// lane holding the lowest block has nobody below it: it takes `seam`, the one fresh byte query[r - 16*lowest_block].
GDW_HD void gdw_shift_query(WaveLane &L, u32 below, bool is_lowest, u32 seam)
{
	const u32 in = is_lowest ? (seam << 24) : below;
	L.Qc[3] = gdw_alignbyte(L.Qc[3], L.Qc[2], 3);
	L.Qc[2] = gdw_alignbyte(L.Qc[2], L.Qc[1], 3);
	L.Qc[1] = gdw_alignbyte(L.Qc[1], L.Qc[0], 3);
	L.Qc[0] = gdw_alignbyte(L.Qc[0], in, 3);
}

// rewrite the persistent score bytes of this lane (every lane, active or not: the rewritten range may spill into
// the first block above the computed window).  any_tn: some lane of the wavefront holds a target N (uniform).
GDW_HD void gdw_update_scores(WaveLane &L, const WaveK &K, bool any_tn)
{
	// index of the AVX-512 score table (SR/ksw2_extd2_avx.c:183-209) folded into 3 bits: 0 match, 1-3 mismatch,
	// 4-7 sc_N.  target ^ query is already right except when both are N (4 ^ 4 = 0): set bit 2 when the target is N
	// and the query byte is not the reverse-complemented N (7 = 4 ^ 3, which the table scores as a mismatch vs N).
	// Without a target N in the block the fix-up term is zero, so wavefronts without any (almost all) skip it.
	if (any_tn) {
#pragma unroll
		for (int g = 0; g < 4; ++g) {
			const u32 x = (L.Tb[g] ^ L.Qc[g]) | (L.Tb[g] & ~(L.Qc[g] << 1) & 0x04040404u);
			L.Sb[g] = gdw_perm(gdw_perm(K.lut_hi, K.lut_lo, x), L.Sb[g], L.SEL[g]);
		}
	} else {
#pragma unroll
		for (int g = 0; g < 4; ++g) L.Sb[g] = gdw_perm(gdw_perm(K.lut_hi, K.lut_lo, L.Tb[g] ^ L.Qc[g]), L.Sb[g], L.SEL[g]);
	}
}

// reset of cell t == r (u, y, y2), only while en >= r (:160-163)
GDW_HD void gdw_reset_tr(WaveLane &L, const WaveK &K, const WaveRow &W)
{
	if (L.blk != (W.r >> 4)) return;
	const int k = W.r & 7;
	const u32 mask = (W.r & 8) ? 0xffff0000u : 0x0000ffffu;
	const u32 uk = gdw_pack2(W.ukey);
#pragma unroll
	for (int kk = 0; kk < 8; ++kk)
		if (kk == k) {
			L.U[kk] = gdw_bfi(mask, uk, L.U[kk]);
			L.Y[kk] = gdw_bfi(mask, K.cy, L.Y[kk]);
			L.Y2[kk] = gdw_bfi(mask, K.cy2, L.Y2[kk]);
		}
}

// One anti-diagonal for one ACTIVE lane.  pX/pV/pX2: register 7 of X/V/X2 of the previous lane (row r-1 values).
// bt: the lane's 16 backtrace bytes of this row (4 dwords; byte 4g+h = cell 2g+(h&1)+8*(h>>1)).
// backtrace byte = (4 - d) | nY2<<4 | nX2<<5 | nY<<6 | nX<<7, n* = "no continuation" (inverse of :263-272); bit 3 is undefined.
// DUAL = false: the single-affine recurrence of ksw_extz2 (K3).  With both gap models equal the second pair (a2, b2) can never
// win the priority chain (equal value, lower tie code) and its continuation flags are never read by the backtrack, so the whole
// X2 / Y2 half is dropped; the two flag bits are stored as "no continuation".
template <bool DUAL = true>
GDW_HD void gdw_compute(WaveLane &L, const WaveK &K, const WaveRow &W, u32 pX, u32 pV, u32 pX2, u32 bt[4])
{
	if (!W.use_array) { // first computed block: boundary scalars x1, v1, x21 (:149-159) instead of what the lane below handed over
		const u32 first = W.m_first_valid ? W.m_first : (L.blk == W.st_ ? ~0u : 0u); // (only the upper halves of the incoming dwords are looked at)
		pX = gdw_bfi_s(first, K.cx, pX), pV = gdw_bfi_s(first, gdw_pack2(W.v1key), pV);
		if (DUAL) pX2 = gdw_bfi_s(first, K.cx2, pX2);
	}
	const u32 inX = gdw_alignbit(L.X[7], pX, 16), inV = gdw_alignbit(L.V[7], pV, 16), inX2 = DUAL ? gdw_alignbit(L.X2[7], pX2, 16) : 0u;
	u32 zk_hi = 0;
#pragma unroll
	for (int k = 7; k >= 0; --k) {
		const u32 xin = k ? L.X[k - 1] : inX, vin = k ? L.V[k - 1] : inV, x2in = DUAL ? (k ? L.X2[k - 1] : inX2) : 0u;
		const u32 sk = gdw_perm(L.Sb[2 + (k >> 2)], L.Sb[k >> 2], 0x0c000c00u | (u32)(k & 3) | (u32)(4 + (k & 3)) << 16);
		const u32 a = pk_add(xin, vin), b = pk_add(L.Y[k], L.U[k]);
		u32 zk = pk_max(pk_max(sk, a), b), a2 = 0, b2 = 0;
		if (DUAL) {
			a2 = pk_add(x2in, vin), b2 = pk_add(L.Y2[k], L.U[k]);
			zk = pk_max(zk, pk_add(pk_max(a2, b2), K.c2));
		}
		const u32 z8 = pk_min(zk & 0xfff8fff8u, K.zmax);
		const u32 nV = pk_sub(z8, L.U[k]), nU = pk_sub(z8, vin); // (this order: U[k] is last read by nV, so nU can take its register)
		const u32 tE = pk_sub(z8, K.te);
		L.X[k] = pk_max(pk_sub(a, tE), K.cx), L.Y[k] = pk_max(pk_sub(b, tE), K.cy);
		if (DUAL) {
			const u32 tE2 = pk_sub(z8, K.te2);
			L.X2[k] = pk_max(pk_sub(a2, tE2), K.cx2), L.Y2[k] = pk_max(pk_sub(b2, tE2), K.cy2);
		}
		L.U[k] = nU, L.V[k] = nV;
		if (k & 1) zk_hi = zk;
		else {
			// flags of register pairs k (cells k, k+8) and k+1 (cells k+1, k+9) together: v_perm's sign selectors (8..11) turn the
			// sign of every 16-bit key -- "no continuation" -- into a 0x00 / 0xff byte, already in backtrace byte order, so the four
			// arrays merge with three v_bfi and no shift; the low nibble comes from the priority-chain key (bit 3 is undefined)
			const u32 mX = gdw_perm(L.X[k + 1], L.X[k], 0x0b090a08u), mY = gdw_perm(L.Y[k + 1], L.Y[k], 0x0b090a08u);
			u32 f;
			if (DUAL) {
				const u32 mX2 = gdw_perm(L.X2[k + 1], L.X2[k], 0x0b090a08u), mY2 = gdw_perm(L.Y2[k + 1], L.Y2[k], 0x0b090a08u);
				f = gdw_bfi_u(0x80808080u, mX, gdw_bfi_u(0x40404040u, mY, gdw_bfi_u(0x20202020u, mX2, mY2)));
			} else f = gdw_bfi_u(0x80808080u, mX, mY) | 0x30303030u;
			bt[k >> 1] = gdw_bfi_u(0xf0f0f0f0u, f, gdw_perm(zk_hi, zk, 0x06020400u));
		}
	}
}

// Rows [rA, rS), rS - rA even, of a long alignment for which, with m = (r - w + 1) >> 1:
//   r - w + 1 even:  st0 = m, en0 = m + w - 1        r - w + 1 odd:  st0 = m, en0 = m + w
// and neither the first block, the cell t == r, nor the last target column is involved (st0 >= 16, (en0 | 15) < r, en0 < tlen - 1):
//   st0 = max(0, r - qlen + 1, (r - w + 1) >> 1) is its last term iff r <= 2 qlen - w - 2 (and r >= w - 1),
//   en0 = min(tlen - 1, r, (r + w) >> 1) is its last term, and below tlen - 1, iff r < 2 (tlen - 1) - w (and r >= w).
GDW_HD void gdw_steady_rows(int qlen, int tlen, int w, int &rA, int &rS)
{
	rA = w + 48;
	if ((rA - w + 1) & 1) ++rA;
	const int a = 2 * (tlen - 1) - w, b = 2 * qlen - w - 1;
	rS = a < b ? a : b;
	rS = rS > rA ? rA + ((rS - rA) & ~1) : rA;
}

// Is the chunk [r0, r1] of the half-block cone [hb0, hb0 + 63] INTERIOR: every row in the middle part of the alignment
// (gdw_steady_rows) and all 512 cells of the cone, on every row, inside the cells whose scores are rewritten ([st0, up)) and inside the
// computed blocks (<= en_)?  Then no lane ever is the first block, resets a cell or keeps a stale score, and the rows need no band
// arithmetic at all (gdw_cone_row_half_fast).  st0 and en0 never decrease, and up >= st0 + 16 * nblkA on both rows of a pair.
GDW_HD bool gdw_cone_interior_half(int r0, int r1, int hb0, int qlen, int tlen, int w)
{
	int rA, rS;
	gdw_steady_rows(qlen, tlen, w, rA, rS);
	if (r0 < rA || r1 >= rS || r0 <= 0) return false;
	int st0a, en0a, st0b, en0b;
	gd_band(r0, qlen, tlen, w, st0a, en0a);
	gd_band(r1, qlen, tlen, w, st0b, en0b);
	const int nblkA = (w - 1 + 16) >> 4;
	return 8 * hb0 >= st0b && 8 * (hb0 + 64) <= st0a + 16 * nblkA && ((hb0 + 63) >> 1) <= (en0a >> 4);
}
// ---- score tracking ----------------------------------------------------------------------------------------
// sum of the 16 V keys / of the U keys of cells 1..15 of a lane (horizontal step across a block)
GDW_HD int gdw_sum16(const u32 A[8])
{
	u32 s = pk_add(pk_add(pk_add(A[0], A[1]), pk_add(A[2], A[3])), pk_add(pk_add(A[4], A[5]), pk_add(A[6], A[7])));
	return gdw_lo(s) + gdw_hi(s);
}
// what the predecessor lane contributes to the tracker of the block activated above it on this anti-diagonal:
//   8*H(r,16m) = 8*H(r,16(m-1)) + sum_{i=1..15} U_i - sum_{i=0..15} V_i  [+ U_0 of the new block, added there]
GDW_HD int gdw_track_handoff(const WaveLane &L) { return L.R + gdw_sum16(L.U) - gdw_lo(L.U[0]) - gdw_sum16(L.V); }

// key of cell `slot` (0..15) of a packed array
GDW_HD int gdw_cell(const u32 A[8], int slot)
{
	u32 v = 0;
#pragma unroll
	for (int k = 0; k < 8; ++k)
		if (k == (slot & 7)) v = A[k];
	return (slot & 8) ? gdw_hi(v) : gdw_lo(v);
}
// 8*H(r, 16m+sl) from 8*H(r,16m): partial horizontal walk inside one block
GDW_HD int gdw_track_to_slot(const WaveLane &L, int sl)
{
	int acc = L.R;
	for (int i = 0; i < sl; ++i) acc += gdw_cell(L.U, i + 1) - gdw_cell(L.V, i);
	return acc;
}

// ---- host-side admission test --------------------------------------------------------------------------------
// The wave kernel takes an alignment iff (a) every anti-diagonal fits `lanes` blocks incl. the score-row spill,
// (b) the band never empties, (c) each block's tracker can be seeded from the block below when it enters the band
// and the final cell can be reached from cell 0 of the last block (the band must be >= 17 cells wide there).
// The definition: condition (c) block by block (~5.6 us for a 50 kbp alignment -- 70 ms of one thread per ONT mini-batch when the planner
// asked it for every alignment).  Kept as the reference form of gd_wave_geometry_ok below; tests/emul/plan_test.cpp compares the two on
// millions of random geometries.
static inline bool gd_wave_geometry_ok_loop(int qlen, int tlen, int w, int lanes)
{
	if (w < 0) w = tlen > qlen ? tlen : qlen;
	if (qlen < 1 || tlen < 1) return false;
	if (gd_ncol16(qlen, tlen, w) > lanes) return false;
	// (b): for w >= 1 the band of every anti-diagonal is non-empty iff the corner is inside the band
	if (w < 1 || tlen - qlen > w || qlen - tlen > w) return false;
	// (c)
	const int mlast = (tlen - 1) >> 4;
	for (int m = 1; m <= mlast; ++m) {
		int rs = 16 * m > 32 * m - w ? 16 * m : 32 * m - w; // first anti-diagonal with en0 >= 16m
		int s0, e0;
		gd_band(rs, qlen, tlen, w, s0, e0);
		if (e0 != 16 * m || s0 > 16 * (m - 1)) return false;
	}
	{
		int rb = tlen - 1 > 2 * (tlen - 1) - w ? tlen - 1 : 2 * (tlen - 1) - w; // first anti-diagonal with en0 == tlen-1
		int s0, e0;
		gd_band(rb, qlen, tlen, w, s0, e0);
		if (e0 != tlen - 1 || s0 > 16 * mlast) return false;
	}
	return true;
}

// The same in O(1): as functions of the block index m, rs = max(16 m, 32 m - w), the three terms of en0 = min(tlen - 1, rs, (rs + w) >> 1)
// and the three of st0 = max(0, rs - qlen + 1, (rs - w + 1) >> 1) are (floors of) linear functions with breakpoints only where two of them
// cross -- m = w / 16 (rs changes its form), rs = 2 qlen - w - 1 (the two non-constant terms of st0) -- so each of the two conditions,
// an inequality between such a function and 16 m / 16 (m - 1), can only change its truth value next to a breakpoint or at an end of
// [1, mlast]: it is enough to test a few m around each.
// (GDW_HD: the 64-lane kernel asks it for the quarter rung of its ladder, once per alignment, with wave-uniform arguments)
GDW_HD bool gd_wave_geometry_ok(int qlen, int tlen, int w, int lanes)
{
	if (w < 0) w = tlen > qlen ? tlen : qlen;
	if (qlen < 1 || tlen < 1) return false;
	if (gd_ncol16(qlen, tlen, w) > lanes) return false;
	if (w < 1 || tlen - qlen > w || qlen - tlen > w) return false;
	const int mlast = (tlen - 1) >> 4;
	auto block_ok = [&](int m) -> bool {
		if (m < 1 || m > mlast) return true;
		const int rs = 16 * m > 32 * m - w ? 16 * m : 32 * m - w;
		int s0, e0;
		gd_band(rs, qlen, tlen, w, s0, e0);
		return e0 == 16 * m && s0 <= 16 * (m - 1);
	};
	const int rx = 2 * qlen - w - 1; // the anti-diagonal on which r - qlen + 1 overtakes (r - w + 1) >> 1
	const int around[4] = {w >> 4, rx > 0 ? (rx + w) / 32 : 0, rx > 0 ? rx / 16 : 0, mlast - 1};
#pragma unroll
	for (int a = 0; a < 4; ++a)
#pragma unroll
		for (int d = -2; d <= 2; ++d)
			if (!block_ok(around[a] + d)) return false;
#pragma unroll
	for (int m = 1; m <= 3; ++m)
		if (!block_ok(m)) return false;
	{
		int rb = tlen - 1 > 2 * (tlen - 1) - w ? tlen - 1 : 2 * (tlen - 1) - w; // first anti-diagonal with en0 == tlen-1
		int s0, e0;
		gd_band(rb, qlen, tlen, w, s0, e0);
		if (e0 != tlen - 1 || s0 > 16 * mlast) return false;
	}
	return true;
}

static inline bool gd_wave_scoring_ok(const KswConst &C)
{
	WaveK K;
	if (!gdw_make_consts(C, K)) return false;
	// no 8-bit wrap-around anywhere in the reference recurrence for these magnitudes (see ksw_wave_core.h)
	const int mis = C.sc_mis < 0 ? -C.sc_mis : C.sc_mis, n = C.sc_N < 0 ? -C.sc_N : C.sc_N;
	return C.sc_mch > 0 && C.sc_mch + 2 * (C.q2 + C.e2) + (mis > n ? mis : n) + (C.q + C.e) <= 120;
}

static inline bool gd_wave_supported(int qlen, int tlen, int w, int lanes)
{
	return qlen + tlen < (1 << 21) && gd_wave_geometry_ok(qlen, tlen, w, lanes); // (a row's offset into the backtrace is a 32-bit quantity)
}

// the checkpointed backtrace of the wide-band kernels (ksw_wave.hip.h, "the same with a CHECKPOINTED backtrace")
#define GD_CK_ROWS 480  // the cells a walk can visit inside one chunk, and all they depend on, span at most 62 HALF blocks (gdw_cone_row_half; <= 31 blocks for gdw_cone_row)
#define GD_CK_REGS 136 // dwords per lane per snapshot: 2 x (48 state + 16 Sb/Tb/Qc/SEL + tn, blk, R) + Rf + pad
static inline __host__ __device__ size_t gd_ck_bytes(int qlen, int tlen, int /*row_bytes*/)
{
	const size_t rows = (size_t)qlen + tlen - 1, n_ck = (rows + GD_CK_ROWS - 1) / GD_CK_ROWS;
	return n_ck * (size_t)GD_CK_REGS * 64 * 4 + (size_t)GD_CK_ROWS * 1024; // snapshots + one chunk of 64-block rows
}

// ---- half blocks (wide bands on a 96-block ring: ksw_extd2_wave96c_kernel) -------------------------------------------------------
// A band of w = 1300 has 83 blocks in flight.  On the 128-position ring (two blocks per lane) 36 % of the lanes idle; here a lane
// holds ONE block of ring positions 0..63 plus HALF a block (8 cells) of positions 64..95 -- twelve packed registers per state
// array instead of sixteen, 86 % of them busy.  A half block keeps its 8 cells as 4 packed registers, register j = cells (j, j+4), so
// "cell t-1" is again the register before (j = 0: the incoming dword of the half / block below).  Both halves of a block are inside
// or outside the reference's 16-aligned window together; everything that is defined per cell (which scores are rewritten, the
// reset of cell t == r, the boundary scalars of the first computed cell) carries over with the half's first target position
// tb = 16 * blk + 8 * half.
struct WaveHalf {
	u32 U[4], V[4], X[4], Y[4], X2[4], Y2[4];
	u32 Sb[2], Tb[2], Qc[2], SEL[2];
	u32 tn;
	int32_t blk, half;
	int32_t R; // 8*H(r, tb): score tracker at the half's first cell
};

GDW_HD void gdw_load_half(WaveHalf &H, const WaveK &K, int m, int half, int r, const uint8_t *query, int qlen, const uint8_t *target, int tlen)
{
	H.blk = m, H.half = half;
	const int tb = (m << 4) + (half << 3);
#pragma unroll
	for (int k = 0; k < 4; ++k) H.U[k] = K.uv0, H.V[k] = K.uv0, H.X[k] = K.cx, H.Y[k] = K.cy, H.X2[k] = K.cx2, H.Y2[k] = K.cy2;
#pragma unroll
	for (int g = 0; g < 2; ++g) {
		u32 tw = 0, qw = 0;
#pragma unroll
		for (int b = 0; b < 4; ++b) {
			const int t = tb + 4 * g + b;
			tw |= (t < tlen ? (u32)target[t] : 0u) << (8 * b);
			qw |= gdw_qbyte(query, qlen, r - t) << (8 * b);
		}
		H.Tb[g] = tw, H.Qc[g] = qw, H.Sb[g] = K.s0, H.SEL[g] = 0x03020100u;
	}
	H.tn = (H.Tb[0] | H.Tb[1]) & 0x04040404u;
	H.R = 0;
}

// selector dword g of a half block of which cells [lo, hi) are rewritten, 0 <= lo, hi <= 8: per lane in gdw_make_sel_half, on the scalar
// unit in gdw_sel_step_half -- one definition for both
GDW_HD u32 gdw_sel_from_range_half(int lo, int hi, int g)
{
	const u32 bm = hi > lo ? (((1u << (hi - lo)) - 1u) << lo) : 0u;
	const u32 n = (bm >> (4 * g)) & 15u;
	const u32 spread = (n * 0x00204081u) & 0x01010101u;
	return 0x03020100u + (spread << 2);
}
GDW_HD void gdw_make_sel_half(WaveHalf &H, int st0, int up)
{
	const int tb = (H.blk << 4) + (H.half << 3);
	int lo = st0 - tb, hi = up - tb;
	lo = lo < 0 ? 0 : lo > 8 ? 8 : lo;
	hi = hi < 0 ? 0 : hi > 8 ? 8 : hi;
#pragma unroll
	for (int g = 0; g < 2; ++g) H.SEL[g] = gdw_sel_from_range_half(lo, hi, g);
}

// THE TWO-LANE UPDATE of the paired steady rows (gdw_narrow_rows, gdw_quarter_rows).  Where a pair's two rows share one window
// [m, up), up = m + 16 nblk with nblk = (w + 15) >> 4 = (w + 16) >> 4 (w no multiple of 16), the pair with counter m rewrites the cells
// of pair m - 1 less cell m - 1, plus cell up - 1: the selectors of exactly two lanes change, the one holding cell m - 1 and the one
// holding cell up - 1 (2 nblk <= 62 half blocks, 4 nblk <= 60 quarter blocks apart on the ring of 64: never the same lane).  up - m is a
// multiple of 16, so both cells sit at the same place c of their half / quarter block: the lower lane goes on rewriting its cells
// [c + 1, 8), the upper lane now rewrites [0, c + 1) -- the limits gdw_make_sel_half clamps st0 - tb and up - tb to, as they come out for
// these two lanes (tests/emul/sel_step_test.cpp holds every lane against gdw_make_sel_half outright).  Lanes and dwords are functions of
// (m, w) alone: scalar unit, then v_writelane_b32.  Not for a pair that takes a block over (m & 15 == 0: the lanes of the retired block
// reload) -- there and on the first pair every lane makes its selectors.
struct GdwSelStep {
	int lane[2];   // the lanes of cell m - 1 and of cell up - 1
	int word[2];   // half form: which of SEL[0] / SEL[1] changes there (quarter form: 0)
	u32 sel[2][2]; // the lane's selector dwords after the change (quarter form: [k][0] only); [k][1 - word[k]] is what the lane holds already,
	               // so a caller may write both dwords of the lane instead of choosing a register by a wave-uniform branch
};
GDW_HD GdwSelStep gdw_sel_step_half(int m, int w)
{
	const int up = m + (((w + 15) >> 4) << 4), c = (m - 1) & 7;
	GdwSelStep S;
	S.lane[0] = ((m - 1) >> 3) & 63, S.lane[1] = ((up - 1) >> 3) & 63;
	S.word[0] = S.word[1] = c >> 2;
	// gdw_sel_from_range_half(c + 1, 8, g) and (0, c + 1, g) without the masks and the multiplies: byte i of selector dword g is i + 4
	// where cell 4 g + i is rewritten, so over the lane's two dwords the lower lane adds 4 to the bytes above c -- eight bytes of 4 shifted
	// up by c + 1 bytes (in two steps: c + 1 can be 8) -- and the upper lane to the other bytes
	const uint64_t t = (0x0404040404040404ull << (8 * c)) << 8;
#pragma unroll
	for (int g = 0; g < 2; ++g) S.sel[0][g] = 0x03020100u + (u32)(t >> (32 * g)), S.sel[1][g] = 0x07060504u - (u32)(t >> (32 * g));
	return S;
}

// the same with the choice of the lowest block's lane as a 0 / ~0 lane mask (one v_bfi with the scalar seam byte as data)
GDW_HD void gdw_shift_query_m(WaveLane &L, u32 below, u32 m_lowest, u32 seam)
{
	const u32 in = gdw_bfi_s(m_lowest, seam << 24, below);
	L.Qc[3] = gdw_alignbyte(L.Qc[3], L.Qc[2], 3);
	L.Qc[2] = gdw_alignbyte(L.Qc[2], L.Qc[1], 3);
	L.Qc[1] = gdw_alignbyte(L.Qc[1], L.Qc[0], 3);
	L.Qc[0] = gdw_alignbyte(L.Qc[0], in, 3);
}

GDW_HD void gdw_shift_query_half(WaveHalf &H, u32 below, bool is_lowest, u32 seam)
{
	const u32 in = is_lowest ? (seam << 24) : below;
	H.Qc[1] = gdw_alignbyte(H.Qc[1], H.Qc[0], 3);
	H.Qc[0] = gdw_alignbyte(H.Qc[0], in, 3);
}

GDW_HD void gdw_shift_query_half_m(WaveHalf &H, u32 below, u32 m_lowest, u32 seam) // (the lowest half's lane as a 0 / ~0 mask)
{
	const u32 in = gdw_bfi_s(m_lowest, seam << 24, below);
	H.Qc[1] = gdw_alignbyte(H.Qc[1], H.Qc[0], 3);
	H.Qc[0] = gdw_alignbyte(H.Qc[0], in, 3);
}

GDW_HD void gdw_update_scores_half(WaveHalf &H, const WaveK &K, bool any_tn)
{
#pragma unroll
	for (int g = 0; g < 2; ++g) {
		u32 x = H.Tb[g] ^ H.Qc[g];
		if (any_tn) x |= H.Tb[g] & ~(H.Qc[g] << 1) & 0x04040404u;
		H.Sb[g] = gdw_perm(gdw_perm(K.lut_hi, K.lut_lo, x), H.Sb[g], H.SEL[g]);
	}
}

// the same for the paired steady rows, the target-N term under a branch the device keeps (see gdw_update_scores_quarter_n)
GDW_HD void gdw_update_scores_half_n(WaveHalf &H, const WaveK &K, u32 any_tn /* wave-uniform, a number: 0 = no lane's target bytes hold an N */, u32 lut_lo /* K.lut_lo, wherever the caller keeps it */)
{
	u32 x[2] = {H.Tb[0] ^ H.Qc[0], H.Tb[1] ^ H.Qc[1]};
	if (any_tn != 0) {
		u32 n0 = H.Tb[0] & ~(H.Qc[0] << 1) & 0x04040404u, n1 = H.Tb[1] & ~(H.Qc[1] << 1) & 0x04040404u;
		GDW_KEEP_BRANCH(n0);
		x[0] |= n0, x[1] |= n1;
	}
#pragma unroll
	for (int g = 0; g < 2; ++g) H.Sb[g] = gdw_perm(gdw_perm(K.lut_hi, lut_lo, x[g]), H.Sb[g], H.SEL[g]);
}

GDW_HD void gdw_reset_tr_half(WaveHalf &H, const WaveK &K, const WaveRow &W)
{
	if (H.blk != (W.r >> 4) || H.half != ((W.r >> 3) & 1)) return;
	const int c = W.r & 7, k = c & 3;
	const u32 mask = (c & 4) ? 0xffff0000u : 0x0000ffffu;
	const u32 uk = gdw_pack2(W.ukey);
#pragma unroll
	for (int kk = 0; kk < 4; ++kk)
		if (kk == k) {
			H.U[kk] = gdw_bfi(mask, uk, H.U[kk]);
			H.Y[kk] = gdw_bfi(mask, K.cy, H.Y[kk]);
			H.Y2[kk] = gdw_bfi(mask, K.cy2, H.Y2[kk]);
		}
}

// one anti-diagonal of an ACTIVE half block.  pX / pV / pX2: the last packed register of X / V / X2 of the (half) block below, row r-1
// values.  BT = false: state and score only (the first pass of the checkpointed form); BT = true: bt[2] receives the half's 8
// backtrace bytes, coded as in gdw_compute, byte 4g + h = cell 2g + (h & 1) + 4 (h >> 1).
template <bool BT = false>
GDW_HD void gdw_compute_half(WaveHalf &H, const WaveK &K, const WaveRow &W, u32 pX, u32 pV, u32 pX2, u32 *bt = nullptr)
{
	if (!W.use_array) {
		const u32 first = W.m_first_valid ? W.m_first_h : ((H.blk == W.st_ && H.half == 0) ? ~0u : 0u);
		pX = gdw_bfi_s(first, K.cx, pX), pV = gdw_bfi_s(first, gdw_pack2(W.v1key), pV), pX2 = gdw_bfi_s(first, K.cx2, pX2);
	}
	const u32 inX = gdw_alignbit(H.X[3], pX, 16), inV = gdw_alignbit(H.V[3], pV, 16), inX2 = gdw_alignbit(H.X2[3], pX2, 16);
	u32 zk_hi = 0;
#pragma unroll
	for (int k = 3; k >= 0; --k) {
		const u32 xin = k ? H.X[k - 1] : inX, vin = k ? H.V[k - 1] : inV, x2in = k ? H.X2[k - 1] : inX2;
		const u32 sk = gdw_perm(H.Sb[1], H.Sb[0], 0x0c000c00u | (u32)k | (u32)(4 + k) << 16);
		const u32 a = pk_add(xin, vin), b = pk_add(H.Y[k], H.U[k]);
		const u32 a2 = pk_add(x2in, vin), b2 = pk_add(H.Y2[k], H.U[k]);
		const u32 zk = pk_max(pk_max(pk_max(sk, a), b), pk_add(pk_max(a2, b2), K.c2));
		const u32 z8 = pk_min(zk & 0xfff8fff8u, K.zmax);
		const u32 nV = pk_sub(z8, H.U[k]), nU = pk_sub(z8, vin);
		const u32 tE = pk_sub(z8, K.te), tE2 = pk_sub(z8, K.te2);
		H.X[k] = pk_max(pk_sub(a, tE), K.cx), H.Y[k] = pk_max(pk_sub(b, tE), K.cy);
		H.X2[k] = pk_max(pk_sub(a2, tE2), K.cx2), H.Y2[k] = pk_max(pk_sub(b2, tE2), K.cy2);
		H.U[k] = nU, H.V[k] = nV;
		if (BT) {
			if (k & 1) zk_hi = zk;
			else {
				const u32 mX = gdw_perm(H.X[k + 1], H.X[k], 0x0b090a08u), mY = gdw_perm(H.Y[k + 1], H.Y[k], 0x0b090a08u);
				const u32 mX2 = gdw_perm(H.X2[k + 1], H.X2[k], 0x0b090a08u), mY2 = gdw_perm(H.Y2[k + 1], H.Y2[k], 0x0b090a08u);
				const u32 f = gdw_bfi_u(0x80808080u, mX, gdw_bfi_u(0x40404040u, mY, gdw_bfi_u(0x20202020u, mX2, mY2)));
				bt[k >> 1] = gdw_bfi_u(0xf0f0f0f0u, f, gdw_perm(zk_hi, zk, 0x06020400u));
			}
		}
	}
}

// a half block out of a block's full record (register k = cells (k, k+8)): cells 8h + j and 8h + j + 4 are the 16-bit halves h of
// registers j and j + 4
GDW_HD u32 gdw_half_pick(u32 rj, u32 rj4, int h) { return h ? (rj >> 16) | (rj4 & 0xffff0000u) : (rj & 0xffffu) | (rj4 << 16); }
GDW_HD void gdw_half_from_lane(const WaveLane &L, int h, WaveHalf &H)
{
#pragma unroll
	for (int j = 0; j < 4; ++j) {
		H.U[j] = gdw_half_pick(L.U[j], L.U[j + 4], h), H.V[j] = gdw_half_pick(L.V[j], L.V[j + 4], h);
		H.X[j] = gdw_half_pick(L.X[j], L.X[j + 4], h), H.Y[j] = gdw_half_pick(L.Y[j], L.Y[j + 4], h);
		H.X2[j] = gdw_half_pick(L.X2[j], L.X2[j + 4], h), H.Y2[j] = gdw_half_pick(L.Y2[j], L.Y2[j + 4], h);
	}
#pragma unroll
	for (int g = 0; g < 2; ++g) {
		H.Sb[g] = h ? L.Sb[2 + g] : L.Sb[g], H.Tb[g] = h ? L.Tb[2 + g] : L.Tb[g];
		H.Qc[g] = h ? L.Qc[2 + g] : L.Qc[g], H.SEL[g] = h ? L.SEL[2 + g] : L.SEL[g];
	}
	H.tn = (H.Tb[0] | H.Tb[1]) & 0x04040404u;
	H.blk = L.blk, H.half = h, H.R = 0;
}
// the pristine half block of any index (also below block 0 or beyond the target), its query bytes those of anti-diagonal rq
GDW_HD void gdw_fresh_half(WaveHalf &H, const WaveK &K, int blk, int half, int rq, const uint8_t *query, int qlen, const uint8_t *target, int tlen)
{
	const int tb = blk * 16 + half * 8;
	H.blk = blk, H.half = half;
#pragma unroll
	for (int k = 0; k < 4; ++k) H.U[k] = K.uv0, H.V[k] = K.uv0, H.X[k] = K.cx, H.Y[k] = K.cy, H.X2[k] = K.cx2, H.Y2[k] = K.cy2;
#pragma unroll
	for (int g = 0; g < 2; ++g) {
		u32 tw = 0, qw = 0;
#pragma unroll
		for (int b = 0; b < 4; ++b) {
			const int t = tb + 4 * g + b;
			tw |= (t >= 0 && t < tlen ? (u32)target[t] : 0u) << (8 * b);
			qw |= gdw_qbyte(query, qlen, rq - t) << (8 * b);
		}
		H.Tb[g] = tw, H.Qc[g] = qw, H.Sb[g] = K.s0, H.SEL[g] = 0x03020100u;
	}
	H.tn = (H.Tb[0] | H.Tb[1]) & 0x04040404u;
	H.R = 0;
}

GDW_HD int gdw_sum8(const u32 A[4])
{
	const u32 s = pk_add(pk_add(A[0], A[1]), pk_add(A[2], A[3]));
	return gdw_lo(s) + gdw_hi(s);
}
// what a half block contributes to the tracker of the (half) block above it: 8*H(r, tb + 8) = 8*H(r, tb) + sum_{i=1..7} U_i - sum_{i=0..7} V_i [+ U_0 there]
GDW_HD int gdw_track_handoff_half(const WaveHalf &H) { return H.R + gdw_sum8(H.U) - gdw_lo(H.U[0]) - gdw_sum8(H.V); }
// key of cell `slot` (0..7) of a half's packed array
GDW_HD int gdw_cell_half(const u32 A[4], int slot)
{
	u32 v = 0;
#pragma unroll
	for (int k = 0; k < 4; ++k)
		if (k == (slot & 3)) v = A[k];
	return (slot & 4) ? gdw_hi(v) : gdw_lo(v);
}
GDW_HD int gdw_track_to_slot_half(const WaveHalf &H, int sl)
{
	int acc = H.R;
	for (int i = 0; i < sl; ++i) acc += gdw_cell_half(H.U, i + 1) - gdw_cell_half(H.V, i);
	return acc;
}
// The snapshots keep the 16-cell layout of WaveLane (register k = cells (k, k+8)) whatever held the block: a half block provides
// the low (half 0) or high (half 1) 16 bits of the eight registers of each array -- cell k of the half is this value.
GDW_HD u32 gdw_half_cell16(const u32 A[4], int k) { return (k & 4) ? (A[k & 3] >> 16) : (A[k & 3] & 0xffffu); }

// ---- the narrow form of the 64-lane kernel: ONE HALF BLOCK per lane ------------------------------------------------------------------
// Lane l holds the half block hidx = 2 blk + half with hidx mod 64 == l (half == l & 1 for good, blk mod 32 == l >> 1): a ring of 32
// blocks, every block split over two neighbouring lanes, so both halves of a block enter and leave the reference's 16-aligned window
// together and the half below is always the previous lane (wave_ror:1, lane 63 -> lane 0).  Four packed registers per state array: a row
// costs half the recurrence instructions of the one-block-per-lane form.  Backtrace rows are 64 x 8 bytes, half block hidx at
// (hidx & 63) * 8, bytes inside a half as gdw_compute_half writes them.
// GD_W_NARROW: the widest band whose window plus score-row spill fits 32 blocks whatever the geometry -- the rewritten scores [st0, up)
// span ((w + 16) >> 4) * 16 cells from any st0 mod 16, i.e. at most ((w + 16) >> 4) + 1 blocks (gd_ncol16 for long sequences).
#define GD_W_NARROW 495
// The admission test in terms of blocks (the 32-block ring) ...
static inline bool gd_narrow_supported(int qlen, int tlen, int w)
{
	return qlen + tlen < (1 << 21) && gd_wave_geometry_ok(qlen, tlen, w, 32);
}
// ... its loop form (block by block; tests/emul/narrow_plan_test.cpp compares the two on random geometries) ...
static inline bool gd_narrow_supported_loop(int qlen, int tlen, int w)
{
	return qlen + tlen < (1 << 21) && gd_wave_geometry_ok_loop(qlen, tlen, w, 32);
}
// ... and what the half-block rows themselves need, anti-diagonal by anti-diagonal, which every admitted geometry must satisfy (same
// test): the band never empties; every half block the score row touches has a lane (a window of at most 64 half blocks from the lowest
// computed block on); the half block that enters the band finds the tracker of the half below it (the band reaches down to that half's
// first cell); the walk to the last cell starts in a half whose first cell is in the band.
static inline bool gd_narrow_rows_ok(int qlen, int tlen, int w)
{
	if (w < 0) w = tlen > qlen ? tlen : qlen;
	if (qlen < 1 || tlen < 1 || w < 1 || qlen + tlen >= (1 << 21)) return false;
	if (gd_ncol16(qlen, tlen, w) > 32) return false; // (a row of the reference's own backtrace: what the slot is sized for is never less)
	int prev_en0 = -1, have_f = 0;
	for (int r = 0; r <= qlen + tlen - 2; ++r) {
		int st0, en0;
		gd_band(r, qlen, tlen, w, st0, en0);
		if (st0 > en0) return false;
		const int up = st0 + (((en0 - st0 + 16) >> 4) << 4);
		if (((up - 1) >> 3) - 2 * (st0 >> 4) > 63) return false;
		if (r > 0 && en0 != prev_en0 && (en0 & 7) == 0 && st0 > en0 - 8) return false;
		if (en0 == tlen - 1 && !have_f) {
			if (st0 > ((tlen - 1) & ~7)) return false;
			have_f = 1;
		}
		prev_en0 = en0;
	}
	return true;
}

// The certificate: does the score S' of the alignment in the band wn prove that the alignment in any wider band is the same?  A path
// that leaves the band |t - q| <= D = wn reaches a diagonal at distance > D on one side and comes back to the end corner at distance
// delta = tlen - qlen: two gaps of net length >= D and >= D -/+ delta, and what is left of the shorter sequence scores at most a per column.
//   UB+ = a min(qlen - (D - delta), tlen - D) - cost(D) - cost(D - delta)   (D - delta >= 0)
//   UB- = a min(qlen - D, tlen - (D + delta)) - cost(D) - cost(D + delta)   (D + delta >= 0)
//   cost(k) = min(q + k e, q2 + k e2), k > 0; 0 else.
// With |delta| <= D and S' > max(UB+, UB-) every such path scores below S', so every cell on a co-optimal path has the same value in both
// bands, and the strict-'>' priority chain and the continuation flags give the same bytes along the walk.
// (a: the largest entry of the scoring matrix -- sc_mch for every scoring in use)
struct GdNarrowArg {
	int32_t w;             // the narrow band to try first (0: off)
	int32_t a, q, e, q2, e2;
	int32_t wq;            // the band of the quarter-block rows, tried before it (GD_W_QUARTER; 0: that rung is not offered)
	// the compact arena (ksw_plan.h): where a GD_NARROW_TRY box that needs its full-band rows after all claims them
	int32_t drain;         // 0: the main launch, claims go to the overflow pool; k > 0: the k-th drain launch behind it, claims go to the whole arena
	int32_t last;          // this is the last launch of the batch's 64-lane kernel: a claim that finds no room is counted (a planner bug)
	int32_t list;          // where the pending list starts, in words of the counter array (0: the batch has none)
	int64_t claim_off;     // the pool's byte offset in the arena (a drain launch: 0)
	int64_t claim_units;   // ... and its size in units of 256 bytes; < 0: the slots are full-size, nothing is ever claimed
};
// the counters of a 64-lane launch behind the six of the ladder (see the kernel): boxes that claimed from the pool, boxes served by a
// drain launch, boxes of the main launch that found no room in the pool (the length of the pending list), boxes left without rows after
// the last launch, then the claim counter (units of 256 bytes) of the main launch and of every drain launch, then the pending list
enum : int { GD_CNT_POOL = 6, GD_CNT_DRAINED = 7, GD_CNT_PENDING = 8, GD_CNT_LEFT = 9, GD_CNT_CLAIM = 10 };
GDW_HD uint32_t gd_full_units(int qlen, int tlen) { return (uint32_t)(((size_t)(qlen + tlen - 1) * 1024 + 64 + 255) >> 8); } // the full-band slot of a box of the 64-lane kernel
// THE CLAIM of a launch, for the kernel and for its replay on the host (ksw_plan.h, gd_drain_rounds): the launch's counter stood at `at`
// units before the atomic add of `need`; the box has its rows at `at` iff they end inside the `units` the launch may hand out
GDW_HD bool gd_claim_fits(uint32_t at, uint32_t need, int64_t units) { return (int64_t)at + (int64_t)need <= units; }
static inline GdNarrowArg gd_narrow_arg(const KswConst &C, int w, int wq = 0)
{
	GdNarrowArg A;
	A.drain = 0, A.last = 1, A.list = 0, A.claim_off = 0, A.claim_units = -1;
	A.w = w, A.wq = w > 0 ? wq : 0, A.q = C.q, A.e = C.e, A.q2 = C.q2, A.e2 = C.e2;
	A.a = C.sc_mch > C.sc_mis ? C.sc_mch : C.sc_mis;
	if (C.sc_N > A.a) A.a = C.sc_N;
	return A;
}
GDW_HD int gd_gap_cost(const GdNarrowArg &A, int k)
{
	if (k <= 0) return 0;
	const int c1 = A.q + k * A.e, c2 = A.q2 + k * A.e2;
	return c1 < c2 ? c1 : c2;
}
GDW_HD bool gd_band_certified(const GdNarrowArg &A, int qlen, int tlen, int score)
{
	const int D = A.w, delta = tlen - qlen;
	if (delta > D || -delta > D) return false;
	bool ok = true;
	if (D - delta >= 0) {
		const int l1 = qlen - (D - delta), l2 = tlen - D;
		const int ub = A.a * (l1 < l2 ? l1 : l2) - gd_gap_cost(A, D) - gd_gap_cost(A, D - delta);
		ok = ok && score > ub;
	}
	if (D + delta >= 0) {
		const int l1 = qlen - D, l2 = tlen - (D + delta);
		const int ub = A.a * (l1 < l2 ? l1 : l2) - gd_gap_cost(A, D) - gd_gap_cost(A, D + delta);
		ok = ok && score > ub;
	}
	return ok;
}

// what the planner writes into KswTask::pad of an alignment of the 64-lane kernel
enum : int32_t { GD_NARROW_NO = 0,   // one block per lane at its own band
                 GD_NARROW_TRY = 1,  // w > GD_W_NARROW: the half-block rows at GD_W_NARROW first, the full band if the certificate fails
                 GD_NARROW_OWN = 2 };// w <= GD_W_NARROW: the half-block rows at its own band, nothing to certify
static inline int32_t gd_narrow_mode(int qlen, int tlen, int w)
{
	if (w < 0) w = tlen > qlen ? tlen : qlen;
	if (w <= GD_W_NARROW) return gd_narrow_supported(qlen, tlen, w) ? GD_NARROW_OWN : GD_NARROW_NO;
	const int delta = tlen - qlen;
	if (delta > GD_W_NARROW || -delta > GD_W_NARROW) return GD_NARROW_NO;
	return gd_narrow_supported(qlen, tlen, GD_W_NARROW) ? GD_NARROW_TRY : GD_NARROW_NO;
}

// ---- the quarter form of the 64-lane kernel: ONE QUARTER BLOCK per lane -------------------------------------------------------------
// Lane l holds the quarter block qidx = 4 blk + quarter with qidx mod 64 == l (quarter == l & 3 for good, blk mod 16 == l >> 2): a ring of
// 16 blocks, every block spread over four neighbouring lanes, so the four quarters of a block enter and leave the reference's 16-aligned
// window together and the quarter below is always the previous lane (wave_ror:1).  A quarter keeps its 4 cells as 2 packed registers per
// state array, register j = cells (j, j + 2), so "cell t-1" is again the register before (j = 0: the incoming dword of the quarter below)
// and it has ONE dword each of score bytes, target bytes, query bytes and selectors.  Everything that is defined per cell carries over with
// the quarter's first target position tb = 16 blk + 4 quarter, exactly as for halves; the score tracker hands over every 4 cells.
// Backtrace rows are 64 x 4 = 256 bytes, quarter block qidx at (qidx & 63) * 4, and inside a quarter BYTE c IS CELL c (the packed order
// (0, 2 | 1, 3) of the registers and the byte order of gdw_compute's flag merge cancel): target position t of a row sits at byte t & 255.
// GD_W_QUARTER: the widest band with ((w + 16) >> 4) + 1 <= 16 -- window plus score-row spill fit the 16 blocks whatever the geometry.
#define GD_W_QUARTER 239
struct WaveQuarter {
	u32 U[2], V[2], X[2], Y[2], X2[2], Y2[2];
	u32 Sb, Tb, Qc, SEL;
	u32 tn;
	int32_t blk, quarter;
	int32_t R; // 8*H(r, tb): score tracker at the quarter's first cell
};

GDW_HD void gdw_load_quarter(WaveQuarter &H, const WaveK &K, int m, int quarter, int r, const uint8_t *query, int qlen, const uint8_t *target, int tlen)
{
	H.blk = m, H.quarter = quarter;
	const int tb = (m << 4) + (quarter << 2);
#pragma unroll
	for (int k = 0; k < 2; ++k) H.U[k] = K.uv0, H.V[k] = K.uv0, H.X[k] = K.cx, H.Y[k] = K.cy, H.X2[k] = K.cx2, H.Y2[k] = K.cy2;
	u32 tw = 0, qw = 0;
#pragma unroll
	for (int b = 0; b < 4; ++b) {
		const int t = tb + b;
		tw |= (t < tlen ? (u32)target[t] : 0u) << (8 * b);
		qw |= gdw_qbyte(query, qlen, r - t) << (8 * b);
	}
	H.Tb = tw, H.Qc = qw, H.Sb = K.s0, H.SEL = 0x03020100u;
	H.tn = H.Tb & 0x04040404u;
	H.R = 0;
}

// the selector dword of a quarter block of which cells [lo, hi) are rewritten, 0 <= lo, hi <= 4 (per lane, and in gdw_sel_step_quarter)
GDW_HD u32 gdw_sel_from_range_quarter(int lo, int hi)
{
	const u32 n = hi > lo ? (((1u << (hi - lo)) - 1u) << lo) : 0u; // bit i: cell i is rewritten
	const u32 spread = (n * 0x00204081u) & 0x01010101u;
	return 0x03020100u + (spread << 2);
}
GDW_HD void gdw_make_sel_quarter(WaveQuarter &H, int st0, int up)
{
	const int tb = (H.blk << 4) + (H.quarter << 2);
	int lo = st0 - tb, hi = up - tb;
	lo = lo < 0 ? 0 : lo > 4 ? 4 : lo;
	hi = hi < 0 ? 0 : hi > 4 ? 4 : hi;
	H.SEL = gdw_sel_from_range_quarter(lo, hi);
}
// the two-lane update of a steady pair's selectors (see gdw_sel_step_half), for quarter blocks: cells [c + 1, 4) and [0, c + 1)
GDW_HD GdwSelStep gdw_sel_step_quarter(int m, int w)
{
	const int up = m + (((w + 15) >> 4) << 4), c = (m - 1) & 3;
	GdwSelStep S;
	S.lane[0] = ((m - 1) >> 2) & 63, S.lane[1] = ((up - 1) >> 2) & 63;
	S.word[0] = S.word[1] = 0;
	// gdw_sel_from_range_quarter(c + 1, 4) and (0, c + 1) without the mask, the multiply and a branch for c == 3: byte i of a selector is
	// i + 4 where cell i is rewritten, so the lower lane adds 4 to the bytes above c -- 0x04040404 shifted up by c + 1 bytes, what leaves
	// the dword dropped -- and the upper lane to the other bytes
	const u32 t = (u32)(0x0404040400ull << (8 * c));
	S.sel[0][0] = 0x03020100u + t, S.sel[1][0] = 0x07060504u - t;
	S.sel[0][1] = S.sel[1][1] = 0;
	return S;
}

// cell 0 takes the byte that cell 3 of the quarter below faced on the previous anti-diagonal: the top byte of the previous lane's Qc
GDW_HD void gdw_shift_query_quarter(WaveQuarter &H, u32 below, bool is_lowest, u32 seam)
{
	const u32 in = is_lowest ? (seam << 24) : below;
	H.Qc = gdw_alignbyte(H.Qc, in, 3);
}
GDW_HD void gdw_shift_query_quarter_m(WaveQuarter &H, u32 below, u32 m_lowest, u32 seam) // (the lowest quarter's lane as a 0 / ~0 mask)
{
	const u32 in = gdw_bfi_s(m_lowest, seam << 24, below);
	H.Qc = gdw_alignbyte(H.Qc, in, 3);
}

GDW_HD void gdw_update_scores_quarter(WaveQuarter &H, const WaveK &K, bool any_tn)
{
	u32 x = H.Tb ^ H.Qc;
	if (any_tn) x |= H.Tb & ~(H.Qc << 1) & 0x04040404u;
	H.Sb = gdw_perm(gdw_perm(K.lut_hi, K.lut_lo, x), H.Sb, H.SEL);
}

// the same for the paired steady rows: the target-N term under a branch the device keeps (an empty asm statement in it: the compiler may not
// turn the branch into a select and compute the term on every row; targets without N -- nearly all -- then skip it on the scalar unit)
GDW_HD void gdw_update_scores_quarter_n(WaveQuarter &H, const WaveK &K, u32 any_tn /* wave-uniform, a number: 0 = no lane's target bytes hold an N */, u32 lut_lo /* K.lut_lo, wherever the caller keeps it */)
{
	u32 x = H.Tb ^ H.Qc;
	if (any_tn != 0) {
		u32 n = H.tn & ~(H.Qc << 1); // (H.tn = H.Tb & 0x04040404)
		GDW_KEEP_BRANCH(n);
		x |= n;
	}
	H.Sb = gdw_perm(gdw_perm(K.lut_hi, lut_lo, x), H.Sb, H.SEL);
}

GDW_HD void gdw_reset_tr_quarter(WaveQuarter &H, const WaveK &K, const WaveRow &W)
{
	if (H.blk != (W.r >> 4) || H.quarter != ((W.r >> 2) & 3)) return;
	const int c = W.r & 3, k = c & 1;
	const u32 mask = (c & 2) ? 0xffff0000u : 0x0000ffffu;
	const u32 uk = gdw_pack2(W.ukey);
#pragma unroll
	for (int kk = 0; kk < 2; ++kk)
		if (kk == k) {
			H.U[kk] = gdw_bfi(mask, uk, H.U[kk]);
			H.Y[kk] = gdw_bfi(mask, K.cy, H.Y[kk]);
			H.Y2[kk] = gdw_bfi(mask, K.cy2, H.Y2[kk]);
		}
}

// one anti-diagonal of an ACTIVE quarter block.  pX / pV / pX2: register 1 of X / V / X2 of the quarter below, row r-1 values (W.m_first_h:
// "the first quarter of block st_").  bt: the quarter's 4 backtrace bytes, coded as in gdw_compute; byte c = cell c: the sign selectors
// 0x0b090a08 pick (reg 0 low, reg 1 low, reg 0 high, reg 1 high) = cells (0, 1, 2, 3), and so does 0x06020400 for the priority-chain keys.
GDW_HD void gdw_compute_quarter(WaveQuarter &H, const WaveK &K, const WaveRow &W, u32 pX, u32 pV, u32 pX2, u32 &bt)
{
	if (!W.use_array) {
		const u32 first = W.m_first_valid ? W.m_first_h : ((H.blk == W.st_ && H.quarter == 0) ? ~0u : 0u);
		pX = gdw_bfi_s(first, K.cx, pX), pV = gdw_bfi_s(first, gdw_pack2(W.v1key), pV), pX2 = gdw_bfi_s(first, K.cx2, pX2);
	}
	const u32 inX = gdw_alignbit(H.X[1], pX, 16), inV = gdw_alignbit(H.V[1], pV, 16), inX2 = gdw_alignbit(H.X2[1], pX2, 16);
	u32 zk_hi = 0;
#pragma unroll
	for (int k = 1; k >= 0; --k) {
		const u32 xin = k ? H.X[0] : inX, vin = k ? H.V[0] : inV, x2in = k ? H.X2[0] : inX2;
		const u32 sk = gdw_perm(0u, H.Sb, 0x0c000c00u | (u32)k | (u32)(2 + k) << 16);
		const u32 a = pk_add(xin, vin), b = pk_add(H.Y[k], H.U[k]);
		const u32 a2 = pk_add(x2in, vin), b2 = pk_add(H.Y2[k], H.U[k]);
		const u32 zk = pk_max(pk_max(pk_max(sk, a), b), pk_add(pk_max(a2, b2), K.c2));
		const u32 z8 = pk_min(zk & 0xfff8fff8u, K.zmax);
		const u32 nV = pk_sub(z8, H.U[k]), nU = pk_sub(z8, vin);
		const u32 tE = pk_sub(z8, K.te), tE2 = pk_sub(z8, K.te2);
		H.X[k] = pk_max(pk_sub(a, tE), K.cx), H.Y[k] = pk_max(pk_sub(b, tE), K.cy);
		H.X2[k] = pk_max(pk_sub(a2, tE2), K.cx2), H.Y2[k] = pk_max(pk_sub(b2, tE2), K.cy2);
		H.U[k] = nU, H.V[k] = nV;
		if (k) zk_hi = zk;
		else {
			const u32 mX = gdw_perm(H.X[1], H.X[0], 0x0b090a08u), mY = gdw_perm(H.Y[1], H.Y[0], 0x0b090a08u);
			const u32 mX2 = gdw_perm(H.X2[1], H.X2[0], 0x0b090a08u), mY2 = gdw_perm(H.Y2[1], H.Y2[0], 0x0b090a08u);
			const u32 f = gdw_bfi_u(0x80808080u, mX, gdw_bfi_u(0x40404040u, mY, gdw_bfi_u(0x20202020u, mX2, mY2)));
			bt = gdw_bfi_u(0xf0f0f0f0u, f, gdw_perm(zk_hi, zk, 0x06020400u));
		}
	}
}

GDW_HD int gdw_sum4(const u32 A[2])
{
	const u32 s = pk_add(A[0], A[1]);
	return gdw_lo(s) + gdw_hi(s);
}
// what a quarter contributes to the tracker of the quarter above it: 8*H(r, tb + 4) = 8*H(r, tb) + sum_{i=1..3} U_i - sum_{i=0..3} V_i [+ U_0 there]
GDW_HD int gdw_track_handoff_quarter(const WaveQuarter &H) { return H.R + gdw_sum4(H.U) - gdw_lo(H.U[0]) - gdw_sum4(H.V); }
// key of cell `slot` (0..3) of a quarter's packed array
GDW_HD int gdw_cell_quarter(const u32 A[2], int slot)
{
	const u32 a0 = A[0], a1 = A[1]; // (both read first: a select between values, never an indexed access)
	const u32 v = (slot & 1) ? a1 : a0;
	return (slot & 2) ? gdw_hi(v) : gdw_lo(v);
}
GDW_HD int gdw_track_to_slot_quarter(const WaveQuarter &H, int sl)
{
	int acc = H.R;
	for (int i = 0; i < sl; ++i) acc += gdw_cell_quarter(H.U, i + 1) - gdw_cell_quarter(H.V, i);
	return acc;
}

// The admission test in terms of blocks (the 16-block ring), usable in the kernel ...
GDW_HD bool gd_quarter_supported(int qlen, int tlen, int w)
{
	return qlen + tlen < (1 << 21) && gd_wave_geometry_ok(qlen, tlen, w, 16);
}
// ... its loop form (tests/emul/quarter_plan_test.cpp compares the two on random geometries) ...
static inline bool gd_quarter_supported_loop(int qlen, int tlen, int w)
{
	return qlen + tlen < (1 << 21) && gd_wave_geometry_ok_loop(qlen, tlen, w, 16);
}
// ... and what the quarter-block rows themselves need, anti-diagonal by anti-diagonal (gd_narrow_rows_ok with quarter indices): the band
// never empties; every quarter the score row touches has a lane (a window of at most 64 quarters from the lowest computed block on); the
// quarter that enters the band ((en0 & 3) == 0) finds the tracker of the quarter below it; the walk to the last cell starts in a quarter
// whose first cell is in the band.
static inline bool gd_quarter_rows_ok(int qlen, int tlen, int w)
{
	if (w < 0) w = tlen > qlen ? tlen : qlen;
	if (qlen < 1 || tlen < 1 || w < 1 || qlen + tlen >= (1 << 21)) return false;
	if (gd_ncol16(qlen, tlen, w) > 16) return false;
	int prev_en0 = -1, have_f = 0;
	for (int r = 0; r <= qlen + tlen - 2; ++r) {
		int st0, en0;
		gd_band(r, qlen, tlen, w, st0, en0);
		if (st0 > en0) return false;
		const int up = st0 + (((en0 - st0 + 16) >> 4) << 4);
		if (((up - 1) >> 2) - 4 * (st0 >> 4) > 63) return false;
		if (r > 0 && en0 != prev_en0 && (en0 & 3) == 0 && st0 > en0 - 4) return false;
		if (en0 == tlen - 1 && !have_f) {
			if (st0 > ((tlen - 1) & ~3)) return false;
			have_f = 1;
		}
		prev_en0 = en0;
	}
	return true;
}

// The first rung of the kernel's ladder, decided in the kernel from the planner's mark and the geometry: the band at which a marked
// alignment runs the quarter-block rows first, or 0.  A band wider than wq (GD_NARROW_TRY, or GD_NARROW_OWN with wq < w <= GD_W_NARROW):
// at wq, to be certified with D = wq (gd_band_certified needs |delta| <= wq); GD_NARROW_OWN with w <= wq: at its own band, nothing to
// certify.  wq == 0: the rung is not offered.  (w: the alignment's band, already made non-negative.)
GDW_HD int gd_quarter_rung(int mode, int qlen, int tlen, int w, int wq)
{
	if (wq <= 0 || mode == GD_NARROW_NO) return 0;
	if (w <= wq) return mode == GD_NARROW_OWN && gd_quarter_supported(qlen, tlen, w) ? w : 0;
	const int delta = tlen - qlen;
	if (delta > wq || -delta > wq) return 0;
	return gd_quarter_supported(qlen, tlen, wq) ? wq : 0;
}
