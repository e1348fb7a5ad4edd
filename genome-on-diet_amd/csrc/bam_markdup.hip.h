// The kernels of duplicate marking (bam_markdup.h holds their statements):
//   dup_key_kernel      one wavefront per record, four to a block of 256 like bam_gather_kernel: the head as the accumulators take it (lane
//                       i loads word i of the fixed bytes, the fields are scalars from there on), the real CIGAR in rounds of 64 words
//                       (reference length: a wave sum; first and last operation other than S and H: scalars from the round's ballot), the
//                       clip run of the record's strand (a wave sum), the QUAL bytes in dwords dealt over the lanes (a wave sum).  Lane 0
//                       writes {key, score} and the entry's place; an ineligible record writes the sentinel key, a bad one the cell of
//                       the first bad record as well (atomicMin, as cov_scatter_kernel).
//   dup_permute_kernel  one thread per entry: the key of the entry the first sort (by descending score) put at place i, for the second sort.
//   dup_decide_kernel   one thread per sorted entry: a duplicate sets the bit of its place in the bitmap (an integer atomicOr); the counts
//                       of eligible entries and duplicates are reduced over the wavefront (ballots) and added once per wavefront; an entry
//                       that starts a group finds the group's end by bisection, and the largest size goes through a wave reduction and
//                       one atomicMax.
//   dup_apply_kernel    one thread per record of a buffer: bit 0x400 of an eligible record rewritten with a byte store, and the flag of
//                       its index row.
// Plain HIP, vector stores and vector atomics only.  A record is only looked at where it lies inside the buffer, and every load is checked
// against its own end (bam_markdup.h, BOUNDS).  No local memory, no scratch memory (genome-on-diet_amd/build.py checks the compiler's
// resource report: at most 32 VGPRs, so the passes can start beside the DP wavefronts of the batches in flight, like the sort's).
#pragma once
#include <hip/hip_runtime.h>
#include "bam_markdup.h"
#include "cov.hip.h"

// a record starts at rows[j].out (a resident result of the sort) or at start[j] (a table of starts): one of the two is given
__global__ __launch_bounds__(256) void dup_key_kernel(const uint8_t *__restrict__ buf, uint64_t len, const uint64_t *__restrict__ start, const GdsRow *__restrict__ rows, uint64_t n_rec,
                                                      uint64_t *__restrict__ key, uint32_t *__restrict__ score, uint32_t *__restrict__ idx, uint64_t *__restrict__ first_bad)
{
	const uint64_t j = (uint64_t)blockIdx.x * 4 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (j >= n_rec) return;
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t at = gdc_uni(rows ? rows[j].out : start[j]);
	const uint8_t *rec = buf + at;
	GdcHead H;
	uint32_t reason = GDC_BAD_FIELDS;
	if (at <= len && len - at >= GDS_FIXED) {
		const uint32_t mine = lane < GDS_FIXED / 4 ? gdc_ld32(rec + 4 * lane) : 0u;
		uint32_t w[GDS_FIXED / 4];
#pragma unroll
		for (int i = 0; i < GDS_FIXED / 4; ++i) w[i] = (uint32_t)__builtin_amdgcn_readlane((int)mine, i);
		reason = gdc_uni(gdc_head_words(rec, len - at, w, &H));
		H.ops_at = gdc_uni(H.ops_at), H.n_ops = gdc_uni(H.n_ops);
	} else H.n = 0, H.ops_at = H.qual_at = 0, H.refID = H.pos = -1, H.n_ops = H.mapq = H.flag = H.l_seq = H.has_qual = 0;
	uint64_t k64 = GDM_SENTINEL;
	uint32_t sc = 0;
	if (!reason && gdm_eligible(H.flag, H.refID, H.pos)) {
		const uint32_t rev = H.flag >> 4 & 1u;
		uint32_t first = H.n_ops, last1 = 0, bad_op = 0;
		uint64_t ref = 0;
#pragma unroll 1
		for (uint32_t b0 = 0; b0 < H.n_ops; b0 += 64) {
			const uint32_t other = gdm_round_lane(rec, H, b0 + lane, &ref, &bad_op);
			gdm_round_mask(__ballot((int)other), b0, H.n_ops, &first, &last1);
		}
		ref = gdc_wave_sum64(ref);
		const uint64_t clip = gdc_wave_sum64(gdm_clip_lane(rec, H, rev ? last1 : 0u, rev ? H.n_ops : first, lane));
		reason = __any((int)bad_op) ? (uint32_t)GDC_BAD_OP : gdm_key(H.refID, H.pos, rev, ref, clip, &k64);
		if (!reason) sc = gdc_wave_sum32(gdm_qual_share(rec, H, lane));
		else k64 = GDM_SENTINEL;
	}
	if (lane == 0) {
		key[j] = k64, score[j] = sc;
		if (idx) idx[j] = (uint32_t)j;
		if (reason) atomicMin((unsigned long long *)first_bad, (unsigned long long)(j << 8 | reason));
	}
}

__global__ __launch_bounds__(256) void dup_permute_kernel(const uint32_t *__restrict__ idx, const uint64_t *__restrict__ key, uint64_t n, uint64_t *__restrict__ pkey)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint32_t k = idx[i];
	pkey[i] = k < n ? key[k] : GDM_SENTINEL;
}

// st: eligible, duplicates, max_group
__global__ __launch_bounds__(256) void dup_decide_kernel(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ place, uint64_t n, uint32_t *__restrict__ bitmap,
                                                         uint32_t *__restrict__ st)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	const bool in = i < n;
	const bool elig = in && skey[i] != GDM_SENTINEL, dup = in && gdm_is_dup(skey, i);
	if (dup) {
		const uint32_t p = place[i];
		if (p < n) atomicOr(bitmap + (p >> 5), 1u << (p & 31u));
	}
	uint32_t size = elig && !dup ? (uint32_t)(gdm_group_end(skey, n, i) - i) : 0u;
	for (int m = 32; m; m >>= 1) {
		const uint32_t o = (uint32_t)__shfl_xor((int)size, m, 64);
		size = o > size ? o : size;
	}
	const uint32_t n_elig = (uint32_t)__popcll(__ballot((int)elig)), n_dup = (uint32_t)__popcll(__ballot((int)dup));
	if ((threadIdx.x & 63u) == 0) {
		if (n_elig) atomicAdd(st, n_elig);
		if (n_dup) atomicAdd(st + 1, n_dup);
		if (size) atomicMax(st + 2, size);
	}
}

// the records of buf[0, len) start at rows[k].out or at start[k]; record k takes bit bit0 + k of the bitmap
__global__ __launch_bounds__(256) void dup_apply_kernel(uint8_t *__restrict__ buf, uint64_t len, const uint64_t *__restrict__ start, GdsRow *__restrict__ rows, uint64_t n,
                                                        const uint32_t *__restrict__ bitmap, uint32_t bit0)
{
	const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (k >= n) return;
	const uint64_t at = rows ? rows[k].out : start[k];
	if (at > len || len - at < 20) return;
	const uint32_t nf = gdm_apply(buf + at, gdm_bit(bitmap, (uint64_t)bit0 + k));
	if (rows) rows[k].flag = (uint16_t)nf;
}
