// BGZF members inflated on the device: one wavefront per member (grid = members, 64 threads), a full DEFLATE decoder whose statements
// are those of bgzf_inflate.h (stored, fixed and dynamic blocks; the split of the work between the scalar chain and the 64 lanes, the
// staging of the output in local memory and the rules that keep it safe on any input bytes are argued there).
//
// Resources: 72656 bytes of local memory per wavefront (GdzLds), so two wavefronts per CU and 512 on the device; a read of 8 MiB brings
// about 130 members, so it is the number of members, not the footprint, that bounds what runs side by side.  No scratch memory
// (genome-on-diet_amd/build.py checks the compiler's resource report).  Every store is a vector store or plain C++.
#pragma once
#include <hip/hip_runtime.h>
#include "bgzf.h"
#include "bgzf_inflate.h"

struct GdzResult { uint32_t rc, out_len; };

// raw: the bytes of the members; m[i]: where member i's deflate stream lies in raw and where its output goes in out (GdBgzfMember; the
// driver has checked every range against both buffers); res[i]: {GDZ_* code, bytes produced}
__global__ __launch_bounds__(64) void bgzf_inflate_kernel(const uint8_t *__restrict__ raw, const GdBgzfMember *__restrict__ m, uint32_t n_members, uint8_t *__restrict__ out,
                                                          GdzResult *__restrict__ res)
{
	__shared__ GdzLds L;
	const uint32_t i = blockIdx.x;
	if (i >= n_members) return;
	const GdBgzfMember M = m[i];
	uint32_t out_len = 0;
	const uint32_t rc = gdz_inflate(L, raw + M.in_off, M.in_len, out + M.out_off, M.isize, &out_len);
	if (threadIdx.x == 0) res[i].rc = rc, res[i].out_len = out_len;
}
