// Blocks of a reference FASTA on the device (ref_fasta.h holds the per-lane statements and the argument why a claimed block is
// kseq_read's).  One wavefront per 1 KiB tile, one 16-byte load per lane, as in fastx_dev.hip.h:
//   ref_classify_kernel  per tile: the class of the last line that starts in it (0: none), and whether the tile disqualifies the block
//   hipcub exclusive take-the-last scan of the classes, seeded with the state at byte 0 (the driver)
//   ref_count_kernel     per tile: bases, header starts, header ends, given the class of the line running into the tile
//   hipcub exclusive sum of the counts
//   ref_write_kernel     gdx_nt4 of every base at d_nt4[base0 + rank]; one GdrHdr row per header line
//   ref_pack_kernel      at the end of the file: d_nt4 -> S, eight bases per word (the inverse of idx_unpack_kernel)
// Every store is checked against the capacity of its buffer.
#pragma once
#include <hip/hip_runtime.h>
#include "fastx_dev.hip.h"
#include "ref_fasta.h"

struct GdrTakeLast {
	__host__ __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return gdr_take_last(a, b); }
};
struct GdrCntSum {
	__host__ __device__ __forceinline__ GdrCnt operator()(const GdrCnt &a, const GdrCnt &b) const
	{
		GdrCnt c = {a.bases + b.bases, a.hstart + b.hstart, a.hend + b.hend, 0};
		return c;
	}
};

// the lane's masks: blk is allocated in whole tiles, so every 16-byte load is inside the buffer; the byte in front of the lane decides
// whether its first byte starts a line (at == 0: the state at byte 0 does)
__device__ __forceinline__ GdrLane gdr_lane_load(const uint8_t *blk, uint32_t at, uint32_t n, int state_in, uint32_t w[4], uint32_t &valid)
{
	gdx_load16(blk, at, w);
	valid = gdx_valid16(at, n);
	return gdr_lane_masks(w, valid, gdr_prev_nl(blk, at, n, state_in));
}

__global__ __launch_bounds__(64) void ref_classify_kernel(const uint8_t *__restrict__ blk, uint32_t n, int state_in, uint32_t *__restrict__ code, GdrMeta *__restrict__ meta)
{
	const uint32_t lane = threadIdx.x, at = blockIdx.x * GDX_TILE + lane * GDX_LANE_BYTES;
	uint32_t w[4], valid;
	const GdrLane L = gdr_lane_load(blk, at, n, state_in, w, valid);
	const uint32_t c = gdr_lane_code(L);
	const uint64_t has = __builtin_amdgcn_ballot_w64(c != 0), ishdr = __builtin_amdgcn_ballot_w64(c == GDR_HD);
	const uint64_t bad = __builtin_amdgcn_ballot_w64(L.bad != 0);
	if (lane == 0) {
		code[blockIdx.x] = gdr_tile_code(has, ishdr);
		if (bad) atomicOr(&meta->bad, 1u);
	}
}

// tile_in: the exclusive take-the-last scan of code[]
__global__ __launch_bounds__(64) void ref_count_kernel(const uint8_t *__restrict__ blk, uint32_t n, int state_in, const uint32_t *__restrict__ tile_in, GdrCnt *__restrict__ counts)
{
	const uint32_t lane = threadIdx.x, at = blockIdx.x * GDX_TILE + lane * GDX_LANE_BYTES;
	uint32_t w[4], valid;
	const GdrLane L = gdr_lane_load(blk, at, n, state_in, w, valid);
	const uint32_t c = gdr_lane_code(L);
	const uint64_t has = __builtin_amdgcn_ballot_w64(c != 0), ishdr = __builtin_amdgcn_ballot_w64(c == GDR_HD);
	uint32_t bases, hend;
	gdr_lane_split(L, valid, gdr_class_in(has, ishdr, lane, tile_in[blockIdx.x]), bases, hend);
	// the three counts of the lane (0 .. 16 each) in one word, summed over the lanes from one ballot per bit
	const uint32_t x = (uint32_t)__builtin_popcount(bases) | (uint32_t)__builtin_popcount(L.hdr) << 5 | (uint32_t)__builtin_popcount(hend) << 10;
	uint32_t tb = 0, ts = 0, te = 0;
#pragma unroll
	for (int bit = 0; bit < 5; ++bit) {
		tb += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64((x >> bit & 1u) != 0)) << bit;
		ts += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64((x >> (5 + bit) & 1u) != 0)) << bit;
		te += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64((x >> (10 + bit) & 1u) != 0)) << bit;
	}
	if (lane == 0) {
		GdrCnt C = {tb, ts, te, 0};
		counts[blockIdx.x] = C;
	}
}

// tile_off: the exclusive sum of counts[].  nt4 has room for nt4_cap bases, rows for row_cap headers.
__global__ __launch_bounds__(64) void ref_write_kernel(const uint8_t *__restrict__ blk, uint32_t n, int state_in, const uint32_t *__restrict__ tile_in, const GdrCnt *__restrict__ tile_off,
                                                       uint8_t *__restrict__ nt4, uint64_t base0, uint64_t nt4_cap, GdrHdr *__restrict__ rows, uint32_t row_cap, GdrMeta *__restrict__ meta)
{
	const uint32_t lane = threadIdx.x, at = blockIdx.x * GDX_TILE + lane * GDX_LANE_BYTES;
	uint32_t w[4], valid;
	const GdrLane L = gdr_lane_load(blk, at, n, state_in, w, valid);
	const uint32_t c = gdr_lane_code(L);
	const uint64_t has = __builtin_amdgcn_ballot_w64(c != 0), ishdr = __builtin_amdgcn_ballot_w64(c == GDR_HD);
	uint32_t bases, hend;
	gdr_lane_split(L, valid, gdr_class_in(has, ishdr, lane, tile_in[blockIdx.x]), bases, hend);
	// exclusive scan over the lanes of the three counts, eleven bits each: a tile has at most 1024 bases, and a header line takes two
	// bytes at least, so at most 513 header starts or ends
	const uint32_t mine = (uint32_t)__builtin_popcount(bases) | (uint32_t)__builtin_popcount(L.hdr) << 11 | (uint32_t)__builtin_popcount(hend) << 22;
	uint32_t x = mine;
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t y = (uint32_t)__shfl_up((int)x, d);
		if (lane >= (uint32_t)d) x += y;
	}
	x -= mine;
	const GdrCnt T = tile_off[blockIdx.x];
	const uint32_t rb = T.bases + (x & 0x7ffu), rs = T.hstart + (x >> 11 & 0x7ffu), re = T.hend + (x >> 22);
	const uint32_t hd_in = state_in == GDR_HD ? 1u : 0u;
	gdr_lane_write(L, bases, hend, w, at, rb, rs, re, hd_in, nt4, base0, nt4_cap, rows, row_cap, meta);
}

__global__ __launch_bounds__(256) void ref_pack_kernel(const uint64_t *__restrict__ nt4x8, uint32_t *__restrict__ S, uint64_t n_words, uint64_t sum)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n_words) S[i] = gdr_pack_word(nt4x8[i], i, sum);
}
