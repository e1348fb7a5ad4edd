// The kernels of the pileup accumulator (pile.h holds their statements):
//   pile_scatter_kernel  one wavefront per record, four to a block of 256 like cov_scatter_kernel, the wavefronts striding over the table
//                        of record starts: PASS 1 validates as coverage does, PASS 2 piles the bases of every M = X run, the positions
//                        of every D run and the anchor of every I into the eight uint32 counters of their positions.  The runs of a
//                        round of 64 operations are taken one after another by all 64 lanes (pile.h).
//   pile_call_kernel     one thread per position of a range: the consensus byte and the 0 / 1 site flag (gdp_call).
//   pile_site_kernel     one thread per position of a range: a site writes its row at the offset hipCUB's exclusive sum gave its flag.
// ATOMICS.  Every add is an integer atomicAdd (unsigned on the counters, unsigned long long on the summary; atomicMin on the cell of the
// first bad record): plain HIP, vector atomics only.  A wave instruction of the scatter adds to up to 64 consecutive rows of 32 bytes,
// one dword in each, so the reads' own bases decide which dword: contention is what the pileup's depth makes it.  The eleven 0 / 1
// summary counters are kept in a register per lane over all records of a wavefront and added once; skipped_baseq is reduced across the
// wavefront and added once per record.
// No local memory, no scratch memory (genome-on-diet_amd/build.py checks the compiler's resource report: at most 32 VGPRs each).
#pragma once
#include <hip/hip_runtime.h>
#include "cov.hip.h"
#include "pile.h"

struct GdpDev {
	uint32_t *cnt;           // 8 x total
	const GdpRegion *regs;   // n_reg
	const uint32_t *clen;    // n_ref
	uint64_t *summary;       // GDP_N_SUMMARY
	uint64_t *first_bad;     // min over the call's bad records of (index << 8 | reason)
	uint32_t n_ref, n_reg, excl_flags, min_mapq, min_baseq;
};

struct GdpWave {
	__device__ __forceinline__ uint32_t uni(uint32_t v) const { return gdc_uni(v); }
	__device__ __forceinline__ uint64_t uni64(uint64_t v) const { return gdc_uni(v); }
	__device__ __forceinline__ void add(uint32_t *p) const { atomicAdd((unsigned *)p, 1u); }
};

__global__ __launch_bounds__(256) void pile_scatter_kernel(const uint8_t *__restrict__ buf, uint64_t len, const uint64_t *__restrict__ start, uint64_t n_rec, GdpDev D)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t stride = (uint64_t)gridDim.x * 4;
	GdpWave W;
	uint32_t acc = 0; // (a call holds fewer than 2^31 records) lane i < GDP_S_SKIPPED_BASEQ: counter i of the summary over this wavefront's records
	for (uint64_t j = (uint64_t)blockIdx.x * 4 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); j < n_rec; j += stride) {
		GdcHead H;
		const uint8_t *rec;
		const uint32_t reason = gdc_record_pass1(buf, len, start[j], lane, D.n_ref, D.clen, &H, &rec);
		uint32_t counted;
		const uint32_t bits = gdp_summary_bits(H, reason, D.excl_flags, D.min_mapq, &counted);
		if (lane < GDP_S_SKIPPED_BASEQ) acc += bits >> lane & 1u;
		if (reason && lane == 0) atomicMin((unsigned long long *)D.first_bad, (unsigned long long)(j << 8 | reason));
		if (!counted) continue;
		// PASS 2
		uint32_t carry_r = (uint32_t)H.pos, carry_q = 0, skipped = 0;
#pragma unroll 1
		for (uint32_t b0 = 0; b0 < H.n_ops; b0 += 64) {
			uint32_t L, rl, ql, tot_r, tot_q, s, n;
			const uint32_t kind = gdp_op(rec, H, b0 + lane, &L, &rl, &ql);
			const uint32_t r = carry_r + gdc_wave_scan(rl, &tot_r) - rl, q = carry_q + gdc_wave_scan(ql, &tot_q) - ql;
			unsigned long long runs = __ballot((int)gdp_run_of(kind, r, (uint32_t)H.pos, L, &s, &n));
			while (runs) { // wave-uniform: one run after another, every lane on each
				const int jn = __builtin_ctzll(runs);
				runs &= runs - 1;
				const uint32_t ku = (uint32_t)__builtin_amdgcn_readlane((int)kind, jn), su = (uint32_t)__builtin_amdgcn_readlane((int)s, jn);
				const uint32_t nu = (uint32_t)__builtin_amdgcn_readlane((int)n, jn), qu = (uint32_t)__builtin_amdgcn_readlane((int)q, jn);
				const uint32_t i0 = gdp_region_lower(W, D.regs, D.n_reg, (uint32_t)H.refID, su);
				skipped += gdp_run_share(W, D.cnt, D.regs, D.n_reg, i0, rec, H, ku, su, nu, qu, D.min_baseq, lane);
			}
			carry_r += tot_r, carry_q += tot_q;
		}
		const uint32_t skipped_all = gdc_wave_sum32(skipped); // (a record holds fewer than 2^31 bases)
		if (lane == 0 && skipped_all) atomicAdd((unsigned long long *)(D.summary + GDP_S_SKIPPED_BASEQ), (unsigned long long)skipped_all);
	}
	if (lane < GDP_S_SKIPPED_BASEQ && acc) atomicAdd((unsigned long long *)(D.summary + lane), (unsigned long long)acc);
}

// the positions [t0, t0 + m) of all: their rows are cnt[8 t .. 8 t + 8), read as two 16-byte loads
struct GdpCallIn {
	const uint32_t *cnt;
	const GdpRegion *regs;
	const uint32_t *S;
	const uint64_t *seq_off;
	uint64_t t0, m;
	uint32_t n_reg;
	GdpCallOpt opt;
};
__device__ __forceinline__ uint32_t gdp_call_position(const GdpCallIn &I, uint64_t k, uint32_t *c, uint32_t *rid, uint32_t *pos, uint32_t *refc, uint8_t *cons, uint32_t *depth, uint32_t *alt)
{
	const uint64_t t = I.t0 + k;
	const uint4 a = *(const uint4 *)(I.cnt + t * GDP_N_CNT), b = *(const uint4 *)(I.cnt + t * GDP_N_CNT + 4);
	c[0] = a.x, c[1] = a.y, c[2] = a.z, c[3] = a.w, c[4] = b.x, c[5] = b.y, c[6] = b.z, c[7] = b.w;
	const uint32_t i = gdp_region_of(I.regs, I.n_reg, t);
	const GdpRegion R = I.regs[i];
	*rid = R.rid, *pos = R.beg + (uint32_t)(t - R.off);
	*refc = gdp_ref_base(I.S, I.seq_off[R.rid] + *pos);
	return gdp_call(c, *refc, I.opt, cons, depth, alt);
}
// cons / flag with alt: either may be NULL.  alt[k] is the alt allele of a site (the site kernel reads it there, so that it need not call again)
__global__ __launch_bounds__(256) void pile_call_kernel(GdpCallIn I, uint8_t *__restrict__ cons, uint32_t *__restrict__ flag, uint8_t *__restrict__ alt_out)
{
	const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (k >= I.m) return;
	uint32_t c[GDP_N_CNT], rid, pos, refc, depth, alt;
	uint8_t cb;
	const uint32_t site = gdp_call_position(I, k, c, &rid, &pos, &refc, &cb, &depth, &alt);
	if (cons) cons[k] = cb;
	if (flag) flag[k] = site, alt_out[k] = (uint8_t)alt;
}
// rows[offs[k]] for every site k of the range (flag[k] != 0, its alt in alt[k]); n_rows: the room of rows
__global__ __launch_bounds__(256) void pile_site_kernel(GdpCallIn I, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ offs, const uint8_t *__restrict__ alt, uint32_t *__restrict__ rows,
                                                        uint32_t n_rows)
{
	const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (k >= I.m || !flag[k]) return;
	const uint32_t o = offs[k];
	if (o >= n_rows) return;
	uint32_t *row = rows + (size_t)o * 13;
	const uint64_t t = I.t0 + k;
	const GdpRegion R = I.regs[gdp_region_of(I.regs, I.n_reg, t)];
	const uint32_t pos = R.beg + (uint32_t)(t - R.off);
	row[0] = R.rid, row[1] = pos, row[2] = gdp_ref_base(I.S, I.seq_off[R.rid] + pos), row[3] = alt[k];
	const uint4 a = *(const uint4 *)(I.cnt + t * GDP_N_CNT), b = *(const uint4 *)(I.cnt + t * GDP_N_CNT + 4);
	row[4] = a.x + a.y + a.z + a.w + b.x + b.y; // depth, as gdp_call forms it
	row[5] = a.x, row[6] = a.y, row[7] = a.z, row[8] = a.w, row[9] = b.x, row[10] = b.y, row[11] = b.z, row[12] = b.w;
}
