// K2 for long alignments, the part of the wavefront walks that is the same on every backtrace layout: the walk state, the byte of the
// register-resident kernels, and the consumption of one fetched WINDOW -- the 64 cells (i0 - k, j0 - k), k = 0..63, of the diagonal the
// walk stands on -- from wave-uniform 64-bit masks.  Shared with the host emulator (tests/emul/walk_emul.cpp): plain C++, no lane
// operations; on the device the masks are ballots of per-lane values (gd_walk_consume, ksw_backtrack.hip.h).
//
// ksw_backtrack (SR/ksw2.h:131-163) visits one cell per iteration.  An alignment of similar sequences stays in state 0 on one diagonal
// for hundreds of cells between two gaps, and every cell of such a run does the same thing: direction 0, push one M, step diagonally.
// A run inside the window is therefore taken in ONE step: the cells whose byte says "diagonal" and that lie inside the stored window of
// their row form the mask `plain`; in state 0 the number of consecutive plain cells from k on is a count of trailing zeros, and n
// iterations of the reference's loop that each leave the state at 0 and push one M are push(M, n), i -= n, j -= n.  Every other cell
// takes exactly the reference's step, with its bits pulled out of the masks.  The visited cells, the state machine and the emitted ops
// are those of ksw_backtrack.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "ksw_common.h"

#if defined(__HIPCC__)
#define GDK_HD __host__ __device__ __forceinline__
#else
#define GDK_HD static inline
#endif

// byte of the register-resident kernels, (4-d) | nY2<<4 | nX2<<5 | nY<<6 | nX<<7 with n* = "no continuation" (bit 3 undefined) -> the
// reference's backtrace byte d | cX<<3 | cY<<4 | cX2<<5 | cY2<<6 (SR/ksw2.h:127-130)
GDK_HD uint32_t gd_bt_decode(uint32_t b)
{
	const uint32_t nb = ~b;
	return (4u - (b & 7u)) | ((nb >> 4) & 0x08u) | ((nb >> 2) & 0x10u) | (nb & 0x20u) | ((nb << 2) & 0x40u);
}

// A walk in resumable form: the cell it stands on, the state of ksw_backtrack, the op run being extended (`last`, flushed when the op
// changes) and the number of ops flushed so far.
struct GdWalk { int i, j, state, have, nc; uint32_t last; };
GDK_HD void gd_walk_init(GdWalk &W, int qlen, int tlen) { W.i = tlen - 1, W.j = qlen - 1, W.state = 0, W.have = 0, W.nc = 0, W.last = 0; }

// ksw_push_cigar (SR/ksw2.h:115-125) on a CIGAR of `cap` ops: ops past the capacity are counted, not stored.  `store`: does this caller
// write (on the device: lane 0 of the wavefront)?
GDK_HD void gd_walk_push(GdWalk &W, uint32_t *cg, int cap, bool store, uint32_t op, uint32_t len)
{
	if (W.have && (W.last & 0xf) == op) W.last += len << 4;
	else {
		if (W.have) { if (W.nc < cap && store) cg[W.nc] = W.last; ++W.nc; }
		W.last = len << 4 | op, W.have = 1;
	}
}

// The 64 cells of a window, bit k = cell (i0 - k, j0 - k):
//   valid       the cell exists and belongs to this call: ik >= 0, jk >= 0, ik + jk >= r0 (the first anti-diagonal of the rows at hand)
//   f1, f2      the cell lies outside the stored window of its row: force_state 1 (above off_end) / 2 (below off); its byte counts as 0
//   d0, d1, d2  the three direction bits of the reference's byte
//   c1 .. c4    its continuation bit for state s, tmp >> (s + 2) & 1
struct GdWalkMasks { uint64_t valid, f1, f2, d0, d1, d2, c1, c2, c3, c4; };

GDK_HD int gd_walk_ctz64(uint64_t x) { return __builtin_ctzll(x); } // (x != 0)

// Consumes the window from k = 0 for as long as the walk moves diagonally: until a step that is not diagonal (the walk has left the
// window's diagonal), an invalid cell (the matrix or the rows at hand end) or k = 64.  The caller fetches the next window from (W.i, W.j).
// Returns the number of loop iterations (runs and single cells), which only the emulator reads.
GDK_HD int gd_walk_window(GdWalk &W, uint32_t *cg, int cap, bool store, const GdWalkMasks &M)
{
	const uint64_t plain = M.valid & ~(M.d0 | M.d1 | M.d2 | M.f1 | M.f2);
	int k = 0, steps = 0;
	while (k < 64 && (M.valid >> k & 1)) {
		++steps;
		if (W.state == 0) {
			const uint64_t stop = ~(plain >> k); // (the k bits shifted in at the top end a run at the window's end)
			const int n = stop ? gd_walk_ctz64(stop) : 64;
			if (n > 0) {
				gd_walk_push(W, cg, cap, store, 0, (uint32_t)n);
				W.i -= n, W.j -= n, k += n;
				continue;
			}
		}
		// one cell of ksw_backtrack
		const int d = (int)(M.d0 >> k & 1) | (int)(M.d1 >> k & 1) << 1 | (int)(M.d2 >> k & 1) << 2;
		if (W.state != 0) {
			const uint64_t c = W.state == 1 ? M.c1 : W.state == 2 ? M.c2 : W.state == 3 ? M.c3 : W.state == 4 ? M.c4 : 0; // (directions are 0..4: no state above 4)
			if (!(c >> k & 1)) W.state = 0;
		}
		if (W.state == 0) W.state = d;
		if (M.f1 >> k & 1) W.state = 1;
		if (M.f2 >> k & 1) W.state = 2;
		if (W.state == 0) { gd_walk_push(W, cg, cap, store, 0, 1); --W.i, --W.j, ++k; }
		else {
			if (W.state == 1 || W.state == 3) { gd_walk_push(W, cg, cap, store, 2, 1); --W.i; }
			else { gd_walk_push(W, cg, cap, store, 1, 1); --W.j; }
			break;
		}
	}
	return steps;
}

// the rest of ksw_backtrack once the walk has left the matrix: the run along its edge and the last op.  Returns n_cigar.
GDK_HD int gd_walk_tail(GdWalk &W, uint32_t *cg, int cap, bool store)
{
	if (W.i >= 0) gd_walk_push(W, cg, cap, store, 2, (uint32_t)(W.i + 1));
	if (W.j >= 0) gd_walk_push(W, cg, cap, store, 1, (uint32_t)(W.j + 1));
	if (W.have) { if (W.nc < cap && store) cg[W.nc] = W.last; ++W.nc; }
	return W.nc;
}
