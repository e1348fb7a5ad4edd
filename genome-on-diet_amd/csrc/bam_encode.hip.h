// BAM alignment records written on the device: one wavefront per record (four records per block of 256 threads), the statements of
// bam_record.h.  The record table and its pools are the host's (bam_flatten.h); every record goes to its own 64-bit offset of a resident
// stream, the buffer bgzf_deflate_kernel then reads, so the uncompressed records never exist on the host.
//
// A row is only written when it lies inside the stream (out + 4 + block_size <= stream_len), and every store of gdb_encode is checked
// against the record's own end: whatever a row holds, nothing is written outside [stream, stream + stream_len).  Records are not
// 4-byte aligned in the stream, so all stores are byte stores; the lanes of a wavefront store neighbouring bytes.  No local memory, no
// cross-lane operation, no scratch memory (genome-on-diet_amd/build.py checks the compiler's resource report: at most 32 VGPRs, so the
// kernel of batch i can start beside the DP wavefronts of batch i + 1).
#pragma once
#include <hip/hip_runtime.h>
#include "bam_record.h"

__global__ __launch_bounds__(256) void bam_encode_kernel(const GdbRec *__restrict__ rec, uint64_t n_rec, const uint8_t *__restrict__ text, const uint32_t *__restrict__ cig,
                                                         const uint8_t *__restrict__ blob, uint8_t *__restrict__ stream, uint64_t stream_len)
{
	// (the wavefront's number through readfirstlane: the compiler then knows the row is wave-uniform and reads it with scalar loads)
	const uint64_t k = (uint64_t)blockIdx.x * 4 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (k >= n_rec) return;
	const GdbRec r = rec[k];
	if (r.out > stream_len || stream_len - r.out < 4ull + r.block_size) return;
	(void)gdb_encode(r, text, cig, blob, stream, threadIdx.x & 63u);
}
