// BAM records unpacked on the device: one wavefront per kept record (four records per block of 256 threads), the statements of
// bam_in.h.  The row table is the host's walk (gdi_walk): a row says where the record's SEQ nibbles and QUAL bytes stand in the block,
// which is uploaded once, and where its text -- seq NUL [qual NUL] -- goes in a resident text buffer, from which fastx_encode_kernel later
// builds the resident batches and which comes back to the host in one copy.
//
// The host has checked every row against the block and the text buffer (gdi_rows_inside); the kernel checks the same ranges again,
// wave-uniformly, and skips a row that fails, and every store of gdi_unpack is checked against the record's own text range: whatever a row
// holds, nothing is read outside [blk, blk + blk_len) or written outside [text, text + text_len).  Records are not aligned in either
// buffer, so loads and stores are byte-wide; the lanes of a wavefront touch neighbouring bytes.  The letters and the complement come
// from constants: no table in memory, no local memory, no cross-lane operation, no scratch memory (genome-on-diet_amd/build.py checks
// the compiler's resource report: at most 32 VGPRs, so the kernel can start beside the DP wavefronts of the batches in flight).
#pragma once
#include <hip/hip_runtime.h>
#include "bam_in.h"

__global__ __launch_bounds__(256) void bam_unpack_kernel(const GdiRow *__restrict__ rows, uint64_t n_rows, const uint8_t *__restrict__ blk, uint64_t blk_len,
                                                         uint8_t *__restrict__ text, uint64_t text_len)
{
	// (the wavefront's number through readfirstlane: the compiler then knows the row is wave-uniform and reads it with scalar loads)
	const uint64_t k = (uint64_t)blockIdx.x * 4 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (k >= n_rows) return;
	const GdiRow r = rows[k];
	if (r.dst > r.dst_end || r.dst_end > text_len) return;
	if ((uint64_t)r.seq_off + (r.l_seq + 1ull) / 2 > blk_len) return;
	if (!(r.flags & GDI_NOQUAL) && (uint64_t)r.qual_off + r.l_seq > blk_len) return;
	gdi_unpack(r, blk, text, threadIdx.x & 63u, 64u);
}
