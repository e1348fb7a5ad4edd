// The cs / MD difference strings of a batch's alignment records on the device (write_cs_or_MD, LR/format.c:150-268): one wavefront
// per record runs gdd_record (map_diffstr.h) -- once without stores for the record's length, once, after an exclusive scan of the
// lengths, into its slice of a dense text buffer.  The encoded reads and the 4-bit reference are read where they already are.
#pragma once
#include <hip/hip_runtime.h>
#include "map_diffstr.h"

struct GddWaveDev { // the wave-wide interface of map_diffstr.h on a gfx950 wavefront
	unsigned lane;
	__device__ __forceinline__ uint64_t ballot(bool p) const { return __builtin_amdgcn_ballot_w64(p); }
	__device__ __forceinline__ unsigned prefix(uint64_t m) const { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }
	__device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
	__device__ __forceinline__ void put(char *out, uint32_t at, char c) const { out[at] = c; }
};

// WRITE = false: len[i] = length of record i's string.  WRITE = true: the string at text[off[i] ..).
// Like map_post_wave_kernel these wavefronts run beside the DP kernel of the next batch in flight (five wavefronts of 96 VGPRs per
// SIMD): raised priority, and at most 32 VGPRs so that one can start in the registers a full house of those leaves free
// (genome-on-diet_amd/build.py checks the compiler's resource report).
template <bool WRITE, int MODE>
__global__ __launch_bounds__(64) void map_diffstr_kernel(int64_t n, GddIn in, int64_t *__restrict__ len, const int64_t *__restrict__ off, char *__restrict__ text)
{
	__builtin_amdgcn_s_setprio(3);
	const int64_t i = blockIdx.x;
	if (i >= n) return;
	GddWaveDev w;
	w.lane = threadIdx.x;
	if (WRITE) {
		const int64_t o = (int64_t)gdd_uni64(w, (uint64_t)off[i]);
		(void)gdd_record<MODE>(w, in, i, text + o);
	} else {
		const int64_t l = gdd_record<MODE>(w, in, i, (char *)nullptr);
		if (w.lane == 0) len[i] = l;
	}
}

template <bool WRITE>
static void map_diffstr_launch(int mode, hipStream_t s, int64_t n, const GddIn &in, int64_t *len, const int64_t *off, char *text)
{
	const dim3 grid((unsigned)n), block(64);
	if (mode == GDD_MD) hipLaunchKernelGGL((map_diffstr_kernel<WRITE, GDD_MD>), grid, block, 0, s, n, in, len, off, text);
	else if (mode == GDD_CS) hipLaunchKernelGGL((map_diffstr_kernel<WRITE, GDD_CS>), grid, block, 0, s, n, in, len, off, text);
	else hipLaunchKernelGGL((map_diffstr_kernel<WRITE, GDD_CS_LONG>), grid, block, 0, s, n, in, len, off, text);
}
