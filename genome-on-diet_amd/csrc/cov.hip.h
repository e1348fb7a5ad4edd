// The kernels of the coverage accumulator (cov.h holds their statements):
//   cov_scatter_kernel  one wavefront per record, four to a block of 256 like bam_gather_kernel, the wavefronts striding over the table of
//                       record starts: PASS 1 validates (lane l sums the operations l, l + 64, ..., two wave reductions), PASS 2 scatters
//                       +1 / -1 into the difference array and sums the qualities of the M = X runs, the runs taken one after another by
//                       all 64 lanes.
//   cov_carry_kernel    one thread: the previous chunk's last depth added to a chunk's first slot, before hipCUB sums the chunk.
//   cov_window_kernel   one wavefront per window of the summed array: positions with depth > 0 and the depth sum.
// ATOMICS.  Every add is an integer atomicAdd (int on the difference array, unsigned long long on the counters; atomicMin on the cell of
// the first bad record): plain HIP, vector atomics only.  Integer sums do not depend on the order of arrival, so every result is
// reproducible bit for bit, which a float accumulator would not be.  Contention is kept off the counters: a record's scalars are reduced
// across its wavefront first and lanes 0 .. 5 then issue ONE instruction that adds the contig's counters; the ten summary counters are
// 0 / 1 per record, so lane i keeps counter i in a register over all records of its wavefront and adds it once, at the end.  The
// difference array takes two adds per M = X run at addresses the reads spread over the reference.
// A record is only looked at where it lies inside the buffer, every load is checked against its own end and every add against its
// contig's slots (cov.h, BOUNDS).  No local memory, no scratch memory (genome-on-diet_amd/build.py checks the compiler's resource
// report: at most 32 VGPRs, so the pass of batch i can start beside the DP wavefronts of batch i + 1).
#pragma once
#include <hip/hip_runtime.h>
#include "cov.h"

struct GdcDev {
	int32_t *diff;          // total_len + 1 slots
	const uint64_t *base;   // n_ref + 1
	const uint32_t *clen;   // n_ref
	uint64_t *contig;       // n_ref x GDC_N_CONTIG
	uint64_t *summary;      // GDC_N_SUMMARY
	uint64_t *first_bad;    // min over the call's bad records of (index << 8 | reason)
	uint32_t n_ref, excl_flags, min_mapq;
};

struct GdcAtomicAdd {
	__device__ __forceinline__ void operator()(int32_t *p, int v) const // v is +1 or -1: both through one register that holds 1
	{
		if (v > 0) atomicAdd(p, 1);
		else atomicSub(p, 1);
	}
};

// The cross-lane sums go through DPP row shifts and row broadcasts, not through __shfl: a shuffle is a ds_bpermute whose per-lane index
// the compiler keeps in a register of its own for every distance (twelve of the kernel's 32), a DPP operand costs none.
//   row_shr:1 / 2 / 4 / 8   the inclusive sums inside every row of 16 lanes (a lane without a source adds the `old` operand, 0)
//   row_bcast15, rows 1, 3  lane 15 of row 0 / 2 onto row 1 / 3;   row_bcast31, rows 2, 3: lane 31 onto rows 2 and 3
// Every caller is in wave-uniform control flow: all 64 lanes are active.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ uint32_t gdc_dpp_add(uint32_t v)
{
	return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
// inclusive prefix sum over the lanes, and the total (wave-uniform, in a scalar register)
__device__ __forceinline__ uint32_t gdc_wave_scan(uint32_t v, uint32_t *total)
{
	v = gdc_dpp_add<0x111, 0xf>(v), v = gdc_dpp_add<0x112, 0xf>(v), v = gdc_dpp_add<0x114, 0xf>(v), v = gdc_dpp_add<0x118, 0xf>(v);
	v = gdc_dpp_add<0x142, 0xa>(v), v = gdc_dpp_add<0x143, 0xc>(v);
	*total = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
	return v;
}
__device__ __forceinline__ uint32_t gdc_wave_sum32(uint32_t v)
{
	uint32_t t;
	(void)gdc_wave_scan(v, &t);
	return t;
}
// a lane's share is below 2^52 (an operation is below 2^28 and a record holds fewer than 2^29 of them, 2^23 per lane; a quality sum is
// below 2^39): two limbs of 26 bits, whose 64-lane sums fit 32 bits
__device__ __forceinline__ uint64_t gdc_wave_sum64(uint64_t v)
{
	const uint32_t lo = gdc_wave_sum32((uint32_t)v & 0x3ffffffu), hi = gdc_wave_sum32((uint32_t)(v >> 26));
	return ((uint64_t)hi << 26) + lo;
}

// a wave-uniform value the compiler cannot see as one (it came through byte loads): into scalar registers
__device__ __forceinline__ uint32_t gdc_uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t gdc_uni(uint64_t v) { return (uint64_t)gdc_uni((uint32_t)(v >> 32)) << 32 | gdc_uni((uint32_t)v); }

// What both scatter kernels (this one and pile_scatter_kernel) do first with the record at buf + at, all 64 lanes of its wavefront in
// step: the head (lane i loads word i of the fixed bytes; the fields are scalars from there on), PASS 1 over the operations and the
// verdict.  *Hp and *recp are the record's; returns gdc_decide's reason, wave-uniform.
__device__ __forceinline__ uint32_t gdc_record_pass1(const uint8_t *buf, uint64_t len, uint64_t at, uint32_t lane, uint32_t n_ref, const uint32_t *clen, GdcHead *Hp,
                                                     const uint8_t **recp)
{
	GdcHead &H = *Hp;
	const uint8_t *rec = *recp = buf + at;
	uint32_t head = GDC_BAD_FIELDS;
	if (at <= len && len - at >= GDS_FIXED) {
		const uint32_t mine = lane < GDS_FIXED / 4 ? gdc_ld32(rec + 4 * lane) : 0u;
		uint32_t w[GDS_FIXED / 4];
#pragma unroll
		for (int i = 0; i < GDS_FIXED / 4; ++i) w[i] = (uint32_t)__builtin_amdgcn_readlane((int)mine, i);
		head = gdc_uni(gdc_head_words(rec, len - at, w, &H));
		H.ops_at = gdc_uni(H.ops_at), H.n_ops = gdc_uni(H.n_ops), H.has_qual = gdc_uni(H.has_qual); // (these may come from loads of their own)
	} else H.n = 0, H.ops_at = H.qual_at = 0, H.refID = H.pos = -1, H.n_ops = H.mapq = H.flag = H.l_seq = H.has_qual = 0;
	// PASS 1
	uint64_t ref = 0, qry = 0;
	uint32_t bad_op = 0;
	if (!head)
#pragma unroll 1
		for (uint32_t k = lane; k < H.n_ops; k += 64) {
			uint32_t L, rl, ql;
			(void)gdc_op(rec, H, k, &L, &rl, &ql, &bad_op);
			ref += rl, qry += ql;
		}
	ref = gdc_wave_sum64(ref), qry = gdc_wave_sum64(qry);
	bad_op = __any((int)bad_op) ? 1u : 0u;
	return gdc_decide(H, head, n_ref, clen, ref, qry, bad_op);
}

__global__ __launch_bounds__(256) void cov_scatter_kernel(const uint8_t *__restrict__ buf, uint64_t len, const uint64_t *__restrict__ start, uint64_t n_rec, GdcDev D)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t stride = (uint64_t)gridDim.x * 4;
	uint32_t acc = 0; // (a call holds fewer than 2^31 records) lane i < GDC_N_SUMMARY: counter i of the summary over this wavefront's records
	for (uint64_t j = (uint64_t)blockIdx.x * 4 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); j < n_rec; j += stride) {
		GdcHead H;
		const uint8_t *rec;
		const uint32_t reason = gdc_record_pass1(buf, len, start[j], lane, D.n_ref, D.clen, &H, &rec);
		uint32_t counted;
		const uint32_t bits = gdc_summary_bits(H, reason, D.excl_flags, D.min_mapq, &counted);
		if (lane < GDC_N_SUMMARY) acc += bits >> lane & 1u;
		if (reason && lane == 0) atomicMin((unsigned long long *)D.first_bad, (unsigned long long)(j << 8 | reason));
		if (!counted) continue;
		// PASS 2
		const uint64_t base = gdc_uni(D.base[H.refID]); // (vector loads: the tables may alias the arrays the atomics write, as far as the compiler knows)
		const uint32_t clen = gdc_uni(D.clen[H.refID]);
		uint32_t carry_r = (uint32_t)H.pos, carry_q = 0;
		uint32_t depth = 0; // (this lane's runs: below the contig's length)
		uint64_t sumq = 0;
		for (uint32_t b0 = 0; b0 < H.n_ops; b0 += 64) {
			uint32_t L, rl, ql, tot_r, tot_q, unused = 0;
			const uint32_t m = gdc_op(rec, H, b0 + lane, &L, &rl, &ql, &unused);
			const uint32_t r = carry_r + gdc_wave_scan(rl, &tot_r) - rl, q = carry_q + gdc_wave_scan(ql, &tot_q) - ql;
			if (m) {
				gdc_scatter(GdcAtomicAdd(), D.diff, base, clen, r, L);
				depth += L;
			}
			if (H.has_qual) {
				unsigned long long runs = __ballot(m && L);
				while (runs) { // wave-uniform: one run after another, every lane on each
					const int jn = __builtin_ctzll(runs);
					runs &= runs - 1;
					sumq += gdc_qual_share(rec, H, (uint32_t)__builtin_amdgcn_readlane((int)q, jn), (uint32_t)__builtin_amdgcn_readlane((int)L, jn), lane);
				}
			}
			carry_r += tot_r, carry_q += tot_q;
		}
		const uint64_t depth_all = gdc_wave_sum64(depth), sumq_all = gdc_wave_sum64(sumq);
		if (lane < GDC_N_CONTIG && lane != GDC_C_COV) { // one instruction: lanes 0, 2, 3, 4, 5 add the contig's counters
			const uint64_t v = lane == GDC_C_READS ? 1u : lane == GDC_C_DEPTH ? depth_all : lane == GDC_C_MAPQ ? H.mapq : lane == GDC_C_BASEQ ? sumq_all : (H.has_qual ? depth_all : 0u);
			if (v) atomicAdd((unsigned long long *)(D.contig + (uint64_t)H.refID * GDC_N_CONTIG + lane), (unsigned long long)v);
		}
	}
	if (lane < GDC_N_SUMMARY && acc) atomicAdd((unsigned long long *)(D.summary + lane), (unsigned long long)acc);
}

__global__ void cov_carry_kernel(int32_t *diff, uint64_t at)
{
	if (threadIdx.x == 0 && blockIdx.x == 0 && at) diff[at] += diff[at - 1];
}

__global__ __launch_bounds__(256) void cov_window_kernel(const uint32_t *__restrict__ depth, const uint64_t *__restrict__ base, const uint64_t *__restrict__ wbase, uint32_t n_ref,
                                                         uint32_t window, uint64_t n_win, uint32_t *__restrict__ cov_out, uint64_t *__restrict__ sum_out)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t stride = (uint64_t)gridDim.x * 4;
	for (uint64_t w = (uint64_t)blockIdx.x * 4 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); w < n_win; w += stride) {
		uint64_t beg, end, sum;
		uint32_t cov;
		(void)gdc_window_range(base, wbase, n_ref, window, w, &beg, &end);
		gdc_window_share(depth, beg, end, lane, &cov, &sum);
		cov = gdc_wave_sum32(cov), sum = gdc_wave_sum64(sum);
		if (lane == 0) cov_out[w] = cov, sum_out[w] = sum;
	}
}
