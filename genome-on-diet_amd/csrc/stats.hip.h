// The kernel of the statistics accumulator (stats.h holds its statements):
//   stats_scatter_kernel  one wavefront per record, four to a block of 256 like the other two scatter kernels, the blocks striding over the
//                         table of record starts: PASS 1 validates as coverage does, the READ pass takes the whole SEQ and QUAL, the
//                         ALIGNMENT pass walks the real CIGAR in the pileup's PASS 2 shape and compares every aligned base with its
//                         reference base (stats.h).
// WHERE THE ADDS GO.  The block tables (every table but read_len: GdtLayout::n_lds cells, 5 326 with the default options) live in local
// memory as uint32, zeroed at block start, added to with local-memory atomics and flushed at block end: the non-zero cells only, as
// 64-bit global atomicAdds.  Every record of a short-read batch hits the same 150 rows, and per-base global atomics would run at the
// L2's same-address rate; the flush is a cost per block, so the launch takes at most GDT_MAX_BLOCKS blocks.  read_len takes one global
// add per read.  The summary is kept in a register per lane over all records of a wavefront (lane i: counter i) and added once.
// Plain HIP, vector atomics only.
// SAME-ADDRESS ADDS are reduced across the wavefront before they touch local memory:
//   the row `cycles`   per-lane registers, one wave sum per record (stats.h, WHAT STAYS IN REGISTERS)
//   subst, base_qual   GdtWave::add_hot: up to GDT_HOT_ROUNDS times the first pending lane's cell goes to every lane, the lanes with that
//                      cell are counted by ballot and popcount and one of them adds the count; lanes still pending after that add by
//                      themselves.  The diagonal of subst is four cells; binned qualities are a handful of cells.
// NO uint32 CELL OVERFLOWS.  A record raises a cell by at most 254 * gdt_weight (a quality byte is at most 254).  The four wavefronts
// of a block step through the table together; at the top of every step they publish the weights of their records, and if the weight
// held since the last flush plus the step's would pass `bound` (2^24: 254 * 2^24 < 2^32) the block flushes first.  A record heavier than
// bound / 4 does not use local memory at all: its adds go to the global cells (GdtWave::direct).  So a cell holds at most 254 * bound.
// A record is only looked at where it lies inside the buffer, every load is checked against its own end and every add against its table
// (stats.h, BOUNDS).
// RESOURCES as the compiler reports them: 56 VGPRs, 106 SGPRs, no scratch memory, 7 wavefronts per SIMD; 21 336 bytes of local memory
// with the default options (5 326 cells and the eight weight words), 72 024 at the ends of the option ranges.  The layout of the twelve
// tables rides in scalar registers and part of it is kept in lanes of vector registers, which is what lifts the count above the other
// two scatter kernels' (genome-on-diet_amd/build.py checks the report: at most 64 VGPRs, no scratch).
#pragma once
#include <hip/hip_runtime.h>
#include "pile.hip.h"
#include "stats.h"

enum { GDT_HOT_ROUNDS = 4 };

struct GdtDev {
	uint64_t *cells;         // GdtLayout::n_all
	const uint32_t *clen;    // n_ref
	const uint32_t *S;       // the index's packed reference
	const uint64_t *seq_off; // n_ref
	uint64_t *first_bad;     // min over the call's bad records of (index << 8 | reason)
	uint64_t bound;
	uint32_t n_ref;
	GdtOpt opt;
	GdtLayout Y;
};

struct GdtWave {
	uint32_t *lds;
	uint64_t *cells;
	uint32_t n_lds, n_all, direct;
	__device__ __forceinline__ void add(uint32_t cell, uint64_t v) const
	{
		if (cell >= n_all || v == 0) return;
		if (cell < n_lds && !direct) atomicAdd((unsigned *)(lds + cell), (unsigned)v);
		else atomicAdd((unsigned long long *)(cells + cell), (unsigned long long)v);
	}
	// the lanes that call this together are counted per cell: one lane of a cell adds for all of them
	__device__ __forceinline__ void add_hot(uint32_t cell) const
	{
		bool pending = true;
#pragma unroll 1
		for (int r = 0; r < GDT_HOT_ROUNDS && pending; ++r) {
			const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)cell);
			if (cell == first) {
				const unsigned long long same = __ballot(1);
				if ((threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(same)) add(cell, (uint64_t)__builtin_popcountll(same));
				pending = false;
			}
		}
		if (pending) add(cell, 1);
	}
};

// the block tables into the global cells, and zero again; every thread of the block, between two barriers of the caller's
__device__ __forceinline__ void gdt_flush(uint32_t *lds, uint64_t *cells, uint32_t n_lds)
{
	for (uint32_t i = threadIdx.x; i < n_lds; i += 256) {
		const uint32_t v = lds[i];
		if (v) atomicAdd((unsigned long long *)(cells + i), (unsigned long long)v), lds[i] = 0;
	}
}

__global__ __launch_bounds__(256) void stats_scatter_kernel(const uint8_t *__restrict__ buf, uint64_t len, const uint64_t *__restrict__ start, uint64_t n_rec, GdtDev D)
{
	extern __shared__ uint32_t gdt_lds[]; // the block tables, then the weights of two steps
	const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const uint64_t stride = (uint64_t)gridDim.x * 4;
	uint32_t *wts = gdt_lds + D.Y.n_lds;
	for (uint32_t i = threadIdx.x; i < D.Y.n_lds + 8; i += 256) gdt_lds[i] = 0;
	GdtWave W;
	W.lds = gdt_lds, W.cells = D.cells, W.n_lds = D.Y.n_lds, W.n_all = D.Y.n_all, W.direct = 0;
	uint64_t acc = 0;  // lane i < GDT_N_SUMMARY: counter i of the summary over this wavefront's records
	uint64_t held = 0; // the weight in the block tables since the last flush: the same in every thread
	uint32_t step = 0;
	for (uint64_t j0 = (uint64_t)blockIdx.x * 4; j0 < n_rec; j0 += stride, step ^= 1u) { // block-uniform
		const uint64_t j = j0 + wave;
		GdcHead H;
		const uint8_t *rec = buf;
		uint32_t is_read = 0, is_aln = 0, bits = 0;
		if (j < n_rec) {
			const uint32_t reason = gdc_record_pass1(buf, len, start[j], lane, D.n_ref, D.clen, &H, &rec);
			bits = gdt_classes(H, reason, D.opt.excl_flags, D.opt.min_mapq, &is_read, &is_aln);
			if (reason && lane == 0) atomicMin((unsigned long long *)D.first_bad, (unsigned long long)(j << 8 | reason));
		}
		// the step's weight
		uint64_t weight = j < n_rec ? gdt_weight(H, is_read, is_aln) : 0;
		W.direct = weight > D.bound / 4;
		if (W.direct) weight = 0;
		if (lane == 0) wts[4 * step + wave] = (uint32_t)weight; // (bound / 4 is below 2^32)
		__syncthreads(); // every add of the step before has been made
		const uint64_t all = (uint64_t)wts[4 * step] + wts[4 * step + 1] + wts[4 * step + 2] + wts[4 * step + 3];
		if (held + all > D.bound) {
			gdt_flush(gdt_lds, D.cells, D.Y.n_lds);
			held = 0;
			__syncthreads();
		}
		held += all;
		if (lane < GDT_S_READS) acc += bits >> lane & 1u;
		if (!is_read && !is_aln) continue; // (wave-uniform; the barrier of this step is behind us)
		uint32_t lead, trail;
		gdt_hard_ends(rec, H, &lead, &trail);
		lead = gdc_uni(lead), trail = gdc_uni(trail);
		GdtRecord R;
		gdt_record_clear(&R);
		if (is_read) {
			GdtReadLane A, T;
			gdt_read_lane_clear(&A);
			gdt_read_share(W, D.Y, rec, H, lead, trail, D.opt.cycles, lane, &A);
			T.a = gdc_wave_sum32(A.a), T.g = gdc_wave_sum32(A.g);
			const bool tail = (uint64_t)(H.flag & 0x10u ? trail : lead) + H.l_seq > D.opt.cycles; // (wave-uniform) some base lies in row `cycles`
#pragma unroll
			for (int c = 0; c < 5; ++c) T.tb[c] = tail ? gdc_wave_sum32(A.tb[c]) : 0u;
			T.tqn = tail ? gdc_wave_sum32(A.tqn) : 0u, T.tqs = tail ? gdc_wave_sum64(A.tqs) : 0u;
			if (lane == 0) gdt_read_close(W, D.Y, H, D.opt, T);
			R.v[GDT_S_READS - GDT_S_READS] = 1, R.v[GDT_S_READ_BASES - GDT_S_READS] = H.l_seq;
		}
		if (is_aln) {
			GdtAlnLane A;
			gdt_aln_lane_clear(&A);
			const uint64_t seq_base = gdc_uni(D.seq_off[H.refID]); // (PASS 1: 0 <= refID < n_ref)
			const uint32_t clen = gdc_uni(D.clen[H.refID]);
			uint32_t carry_r = (uint32_t)H.pos, carry_q = 0;
#pragma unroll 1
			for (uint32_t b0 = 0; b0 < H.n_ops; b0 += 64) {
				uint32_t L, rl, ql, tot_r, tot_q, s, n;
				const uint32_t kind = gdp_op(rec, H, b0 + lane, &L, &rl, &ql);
				const uint32_t r = carry_r + gdc_wave_scan(rl, &tot_r) - rl, q = carry_q + gdc_wave_scan(ql, &tot_q) - ql;
				gdt_op_share(W, D.Y, rec, H, D.opt.max_indel, b0 + lane, kind, L, &A);
				unsigned long long runs = __ballot((int)(kind == GDP_K_BASES && H.l_seq > 0 && gdp_run_of(kind, r, (uint32_t)H.pos, L, &s, &n)));
				while (runs) { // wave-uniform: one run after another, every lane on each
					const int jn = __builtin_ctzll(runs);
					runs &= runs - 1;
					const uint32_t su = (uint32_t)__builtin_amdgcn_readlane((int)s, jn), nu = (uint32_t)__builtin_amdgcn_readlane((int)n, jn), qu = (uint32_t)__builtin_amdgcn_readlane((int)q, jn);
					gdt_run_share(W, D.Y, rec, H, D.S, seq_base, clen, lead, trail, D.opt.cycles, su, nu, qu, lane, &A);
				}
				carry_r += tot_r, carry_q += tot_q;
			}
			// (a record holds fewer than 2^31 aligned bases and operations, and deletes fewer bases than its contig has; a lane's share of the other sums is below 2^52)
			const uint32_t m = gdc_wave_sum32(A.m), x = gdc_wave_sum32(A.x), o = gdc_wave_sum32(A.o), tcn = gdc_wave_sum32(A.tcn), tcx = gdc_wave_sum32(A.tcx);
			const uint32_t ie = gdc_wave_sum32(A.ie), de = gdc_wave_sum32(A.de), db = gdc_wave_sum32(A.db);
			const uint64_t ib = gdc_wave_sum64(A.ib), sc = gdc_wave_sum64(A.sc), hc = gdc_wave_sum64(A.hc);
			if (lane == 0) gdt_aln_close(W, D.Y, H, D.opt, m, x, tcn, tcx, ie, de);
			gdt_aln_record(H, m, x, o, ie, ib, de, db, sc, hc, &R);
		}
#pragma unroll
		for (int i = 0; i < GDT_N_SUMMARY - GDT_S_READS; ++i)
			if (lane == (uint32_t)(GDT_S_READS + i)) acc += R.v[i];
	}
	if (lane < GDT_N_SUMMARY && acc) atomicAdd((unsigned long long *)(D.cells + D.Y.off[GDT_T_SUMMARY] + lane), (unsigned long long)acc);
	__syncthreads();
	gdt_flush(gdt_lds, D.cells, D.Y.n_lds);
}
