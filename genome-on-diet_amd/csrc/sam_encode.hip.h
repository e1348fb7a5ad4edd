// SAM lines written on the device: one wavefront per line (four lines per block of 256 threads), the statements of sam_record.h.  The
// table and its pools are the host's (sam_flatten.h); every line goes to its own 64-bit offset of a resident stream, the buffer
// bgzf_deflate_kernel then reads, so on that route the uncompressed text never exists on the host.
//
// A row is only written when it lies inside the stream (out + size <= stream_len), and every store of gds_format is checked against the
// line's own end: whatever a row holds, nothing is written outside [stream, stream + stream_len).  All stores are byte stores; the lanes
// of a wavefront store neighbouring bytes.  The one cross-lane operation is the wave scan that places the CIGAR's operations
// (gds_wave_scan: six shuffles per round of 64 operations): every loop around it is wave-uniform, so all 64 lanes reach it together.  No
// local memory, no scratch memory (genome-on-diet_amd/build.py checks the compiler's resource report: at most 32 VGPRs, so the kernel
// of batch i can start beside the DP wavefronts of batch i + 1).
#pragma once
#include <hip/hip_runtime.h>
#include "sam_record.h"

__global__ __launch_bounds__(256) void sam_encode_kernel(const GdsRec *__restrict__ rec, uint64_t n_rec, const uint8_t *__restrict__ text, const uint32_t *__restrict__ cig,
                                                         const uint8_t *__restrict__ blob, const uint8_t *__restrict__ rname, const uint64_t *__restrict__ rname_off,
                                                         uint8_t *__restrict__ stream, uint64_t stream_len)
{
	// (the wavefront's number through readfirstlane: the compiler then knows the row is wave-uniform and reads it with scalar loads)
	const uint64_t k = (uint64_t)blockIdx.x * 4 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (k >= n_rec) return;
	const GdsRec r = rec[k];
	if (r.out > stream_len || stream_len - r.out < r.size) return;
	(void)gds_format(r, text, cig, blob, rname, rname_off, stream, threadIdx.x & 63u);
}
