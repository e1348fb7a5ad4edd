// FASTQ blocks on the device (fastx_dev.h holds the per-lane statements and the argument why a strict record is kseq_read's):
//   fastx_count_kernel   newlines per 1 KiB tile (one wavefront, one 16-byte load per lane) and the first '\r' of the block
//   hipcub exclusive scan of the counts (the driver, gdiet_hip.hip)
//   fastx_write_kernel   the offset of every newline, in order
//   fastx_record_kernel  one thread per four complete lines: the record table and first_bad, the first record that is not strict
//   fastx_encode_kernel  per mini-batch: the nt4 codes of the selected reads at their place in the resident batch, and "holds U/u"
// They run on the reader's stream beside the DP kernel of the batches in flight, so they keep to the budget of the other side kernels:
// at most 32 VGPRs, no scratch (genome-on-diet_amd/build.py checks the compiler's resource report).
#pragma once
#include <hip/hip_runtime.h>
#include "fastx_dev.h"

struct GdxMeta { uint32_t first_cr, first_bad; }; // both start as GDX_NONE

// the lane's 16 bytes; blk is allocated in whole tiles, so the load is inside the buffer for every lane of every tile
__device__ __forceinline__ void gdx_load16(const uint8_t *blk, uint32_t at, uint32_t w[4])
{
	const uint4 v = *(const uint4 *)(blk + at);
	w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
}

__global__ __launch_bounds__(64) void fastx_count_kernel(const uint8_t *__restrict__ blk, uint32_t n, uint32_t *__restrict__ counts, GdxMeta *__restrict__ meta)
{
	const uint32_t lane = threadIdx.x, at = blockIdx.x * GDX_TILE + lane * GDX_LANE_BYTES;
	uint32_t w[4];
	gdx_load16(blk, at, w);
	const uint32_t valid = gdx_valid16(at, n);
	const uint32_t c = __builtin_popcount(gdx_eq_mask16(w, '\n', valid)); // 0 .. 16
	const uint32_t crm = gdx_eq_mask16(w, '\r', valid);
	// the tile's count from one ballot per bit of the lanes' counts: scalar population counts, no lane exchanges
	uint32_t total = 0;
	for (int bit = 0; bit < 5; ++bit) total += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64((c >> bit & 1u) != 0)) << bit;
	if (lane == 0) counts[blockIdx.x] = total;
	const uint64_t has_cr = __builtin_amdgcn_ballot_w64(crm != 0);
	if (has_cr && lane == (uint32_t)__builtin_ctzll(has_cr)) atomicMin(&meta->first_cr, at + (uint32_t)__builtin_ctz(crm)); // the tile's first one
}

// tile_off: the exclusive scan of counts; nl has room for cap offsets (the driver has checked the total against it)
__global__ __launch_bounds__(64) void fastx_write_kernel(const uint8_t *__restrict__ blk, uint32_t n, const uint32_t *__restrict__ tile_off, uint32_t *__restrict__ nl, uint32_t cap)
{
	const uint32_t lane = threadIdx.x, at = blockIdx.x * GDX_TILE + lane * GDX_LANE_BYTES;
	uint32_t w[4];
	gdx_load16(blk, at, w);
	uint32_t m = gdx_eq_mask16(w, '\n', gdx_valid16(at, n));
	const uint32_t c = __builtin_popcount(m);
	uint32_t x = c; // inclusive scan over the lanes
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t y = (uint32_t)__shfl_up((int)x, d);
		if (lane >= (uint32_t)d) x += y;
	}
	uint32_t o = tile_off[blockIdx.x] + x - c;
	while (m) {
		if (o < cap) nl[o] = at + (uint32_t)__builtin_ctz(m);
		m &= m - 1, ++o;
	}
}

__global__ __launch_bounds__(256) void fastx_record_kernel(const uint8_t *__restrict__ blk, const uint32_t *__restrict__ nl, uint32_t n_cand, GdxRec *__restrict__ rec, GdxMeta *__restrict__ meta)
{
	const uint32_t r = blockIdx.x * 256u + threadIdx.x;
	bool bad = false;
	if (r < n_cand) {
		GdxRec R;
		bad = !gdx_record(blk, nl, r, meta->first_cr, R);
		rec[r] = R;
	}
	const uint64_t b = __builtin_amdgcn_ballot_w64(bad);
	if (b && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(b)) atomicMin(&meta->first_bad, r); // the wavefront's first one
}

// The device reads of a mini-batch are runs of consecutive records of device blocks.  Run k holds the device reads [dev_first, next run's
// dev_first): records first_rec .. of its block, reads out_first .. of the batch.
struct GdxSeg {
	const uint8_t *blk;
	const GdxRec *rec;
	int32_t first_rec, out_first, dev_first, pad;
};

// one wavefront per device read d < n_dev
__global__ __launch_bounds__(64) void fastx_encode_kernel(int32_t n_dev, int32_t n_seg, const GdxSeg *__restrict__ seg, const int64_t *__restrict__ roff, uint8_t *__restrict__ reads,
                                                          uint8_t *__restrict__ uflag)
{
	__builtin_amdgcn_s_setprio(3);
	const int32_t d = blockIdx.x;
	if (d >= n_dev) return;
	int32_t lo = 0, hi = n_seg - 1; // the last run with dev_first <= d
	while (lo < hi) {
		const int32_t mid = (lo + hi + 1) >> 1;
		if (seg[mid].dev_first <= d) lo = mid; else hi = mid - 1;
	}
	const GdxSeg S = seg[lo];
	const GdxRec *R = S.rec + S.first_rec + (d - S.dev_first);
	const int32_t i = S.out_first + (d - S.dev_first);
	const uint8_t *src = S.blk + R->seq_off;
	const uint32_t len = R->seq_len;
	uint8_t *dst = reads + roff[i];
	bool u = false;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
	for (uint32_t k = threadIdx.x; k < len; k += 64) { // (kept rolled: the register budget)
		const uint32_t c = src[k];
		dst[k] = (uint8_t)gdx_nt4(c);
		u |= gdx_is_u(c);
	}
	const uint64_t any = __builtin_amdgcn_ballot_w64(u);
	if (threadIdx.x == 0) uflag[i] = any ? 1 : 0;
}
