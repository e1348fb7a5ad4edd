// The kernels of the coordinate sort of BAM records (bam_sort.h holds their statements):
//   bam_key_kernel      one thread per record: key, index and size from the record's own bytes at start[k]
//   bam_permute_kernel  one thread per OUTPUT record: source offset and size of the record the stable sort put at place j (the sizes then
//                       go through an exclusive scan: the sorted offsets)
//   bam_gather_kernel   one wavefront per OUTPUT record, four to a block of 256 like bam_encode_kernel: the lanes copy the record from its
//                       source offset to its sorted offset, sum the reference length of its CIGAR field (lane l the words l, l + 64, ...,
//                       then a wave reduction in registers) and lane 0 writes the record's 32-byte index row.
// The gather takes its source offsets from a table, so the merge of several sorted runs uses it unchanged with the offsets of its plan.
// A record is only moved when both of its ranges lie inside their buffers, and every load and store is checked against the record's
// own end on top of that (bam_sort.h, BOUNDS).  No local memory, no scratch memory (genome-on-diet_amd/build.py checks the compiler's
// resource report: at most 32 VGPRs, so the pass can start beside the DP wavefronts of the batches in flight).
#pragma once
#include <hip/hip_runtime.h>
#include "bam_sort.h"

__global__ __launch_bounds__(256) void bam_key_kernel(const uint8_t *__restrict__ buf, uint64_t len, const uint64_t *__restrict__ start, uint64_t n_rec, uint64_t *__restrict__ key,
                                                      uint32_t *__restrict__ idx, uint32_t *__restrict__ size)
{
	const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (k >= n_rec) return;
	uint64_t v;
	size[k] = gds_key(buf, len, start[k], &v);
	key[k] = v, idx[k] = (uint32_t)k;
}

__global__ __launch_bounds__(256) void bam_permute_kernel(const uint32_t *__restrict__ idx, const uint64_t *__restrict__ start, const uint32_t *__restrict__ size, uint64_t n_rec,
                                                          uint64_t *__restrict__ src, uint64_t *__restrict__ psize)
{
	const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (j >= n_rec) return;
	const uint32_t k = idx[j];
	const bool ok = k < n_rec;
	src[j] = ok ? start[k] : 0, psize[j] = ok ? size[k] : 0;
}

__global__ __launch_bounds__(256) void bam_gather_kernel(const uint8_t *__restrict__ in, uint64_t in_len, const uint64_t *__restrict__ src, const uint64_t *__restrict__ psize,
                                                         const uint64_t *__restrict__ dst, uint64_t n_rec, uint8_t *__restrict__ out, uint64_t out_len, GdsRow *__restrict__ rows)
{
	const uint64_t j = (uint64_t)blockIdx.x * 4 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (j >= n_rec) return;
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t s = src[j], d = dst[j], n = psize[j];
	if (n < GDS_FIXED || s > in_len || in_len - s < n || d > out_len || out_len - d < n) { // a row that says so: the host counts them
		if (lane == 0) {
			GdsRow r;
			r.key = ~(uint64_t)0, r.out = ~(uint64_t)0, r.refID = -1, r.pos = -1, r.end = 0, r.bin = 0, r.flag = 0;
			rows[j] = r;
		}
		return;
	}
	const uint8_t *rec = in + s;
	gds_gather_lane(rec, out + d, n, lane);
	uint32_t ref_len = gds_ref_len_lane(rec, n, lane);
	for (int m = 32; m; m >>= 1) ref_len += (uint32_t)__shfl_xor((int)ref_len, m, 64);
	if (lane == 0) rows[j] = gds_row(rec, d, ref_len);
}
