// BGZF members written on the device: one wavefront per member (grid = members, 64 threads), a DEFLATE encoder with CRC32 whose
// statements are those of bgzf_deflate.h (match search over 64 positions side by side, a wave-uniform greedy pass, several dynamic or
// fixed blocks per member, the stored fallback; the split of the work, determinism and the rules W1-W4 are argued there), and the small
// kernel that gathers the members from their slots to their final offsets.
//
// Resources: 104656 bytes of local memory per wavefront (GddLds), so one wavefront per CU and 256 on the device; a mini-batch of SAM
// text is about 1600 members.  Local memory bounds the kernel to one wavefront per SIMD at most, so registers up to 128 cost no
// occupancy; no scratch memory (genome-on-diet_amd/build.py checks the compiler's resource report).  Every store is a vector store or
// plain C++; the local-memory atomics are max, add and or on 32-bit words.
#pragma once
#include <hip/hip_runtime.h>
#include "bgzf_deflate.h"

struct GddResult { uint32_t rc, member_len; };

// in[0, in_len) cut every GDD_MAX_IN bytes; member i goes to slots + i * GDD_SLOT; res[i]: {GDD_* code, the member's bytes}
__global__ __launch_bounds__(64) void bgzf_deflate_kernel(const uint8_t *__restrict__ in, uint64_t in_len, uint32_t n_members, uint8_t *__restrict__ slots, GddResult *__restrict__ res)
{
	__shared__ GddLds L;
	const uint32_t i = blockIdx.x;
	if (i >= n_members) return;
	const uint64_t at = (uint64_t)i * GDD_MAX_IN;
	if (at > in_len) return;
	const uint32_t n = in_len - at < GDD_MAX_IN ? (uint32_t)(in_len - at) : (uint32_t)GDD_MAX_IN;
	uint32_t member_len = 0;
	const uint32_t rc = gdd_deflate(L, in + at, n, slots + (uint64_t)i * GDD_SLOT, &member_len);
	if (threadIdx.x == 0) res[i].rc = rc, res[i].member_len = member_len;
}

// member i: slots[i * GDD_SLOT, + len[i]) -> out[off[i], + len[i]) (off: the host's prefix sum; the driver has checked both against the
// buffers).  One block per member: single bytes up to the first 4-byte boundary of the destination and behind the last, words between.
__global__ __launch_bounds__(256) void bgzf_pack_kernel(const uint8_t *__restrict__ slots, const uint64_t *__restrict__ off, const uint32_t *__restrict__ len, uint32_t n_members,
                                                        uint8_t *__restrict__ out)
{
	const uint32_t i = blockIdx.x;
	if (i >= n_members) return;
	const uint32_t n = len[i] <= GDD_SLOT ? len[i] : (uint32_t)GDD_SLOT;
	const uint8_t *src = slots + (uint64_t)i * GDD_SLOT;
	uint8_t *dst = out + off[i];
	const uint32_t lead = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u, front = lead < n ? lead : n, words = (n - front) / 4u;
	for (uint32_t k = threadIdx.x; k < front; k += blockDim.x) dst[k] = src[k];
	for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) {
		uint32_t v;
		__builtin_memcpy(&v, src + front + 4u * w, 4);
		*(uint32_t *)(void *)(dst + front + 4u * w) = v;
	}
	for (uint32_t k = front + 4u * words + threadIdx.x; k < n; k += blockDim.x) dst[k] = src[k];
}
