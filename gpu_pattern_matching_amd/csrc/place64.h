// 64-bit placement: what the passes that write a packed byte output (rewrite.hip, and through range_pack.h extract.hip and format.hip) share on top of the
// record-pass core.  Internal to the library, gfx950 only.  Two launches of 64-bit block sums over the input cells give
// every used cell its end in the output; the copy kernels find the cells of a tile of OUTPUT by a search on those ends.
#pragma once

#include "record_pass.h"

namespace acm_rp {

constexpr uint32_t kTileBytes = 16384;            // output bytes a copy kernel's workgroup owns
constexpr size_t kMaxBytes = 0x7FFFFFFFul - 16;   // 2^31 - 17: the longest text and the longest output

// sum over the block of v.  Every thread gets the sum.  red: kWaves cells.
__device__ __forceinline__ int64_t block_sum64(int64_t v, int64_t *red)
{
	for (int o = 32; o > 0; o >>= 1)
		v += __shfl_xor((long long)v, o, 64);
	__syncthreads();   // (red of an earlier call is no longer read)
	if (lane_id() == 0)
		red[threadIdx.x / 64] = v;
	__syncthreads();
	int64_t s = 0;
	for (int w = 0; w < kWaves; w++)
		s += red[w];
	return s;
}

// exclusive prefix of v over the block in thread order, and the block's total.  red: kWaves cells.
__device__ __forceinline__ int64_t block_prefix64(int64_t v, int64_t *red, int64_t &total)
{
	const uint32_t lane = lane_id(), wave = threadIdx.x / 64;
	int64_t inc = v;
	for (int o = 1; o < 64; o <<= 1) {
		const int64_t up = __shfl_up((long long)inc, o, 64);
		inc += lane >= (uint32_t)o ? up : 0;
	}
	__syncthreads();
	if (lane == 63)
		red[wave] = inc;
	__syncthreads();
	int64_t before = 0;
	total = 0;
	for (uint32_t w = 0; w < (uint32_t)kWaves; w++) {
		before += w < wave ? red[w] : 0;
		total += red[w];
	}
	return before + inc - v;
}

__device__ __forceinline__ int32_t sat32(int64_t v)
{
	return (int32_t)max((int64_t)INT32_MIN, min(v, (int64_t)INT32_MAX));
}

// number of cells of the sorted a[0, n) that are <= key, found by the whole wave, 64 samples a step (record_pass.h,
// wave_upper_bound).  Every lane passes the same arguments and gets the same answer, in [0, n], sorted or not.
__device__ inline uint32_t wave_upper_bound64(const int64_t *a, uint32_t n, int64_t key)
{
	const uint32_t lane = lane_id();
	uint32_t lo = 0, hi = n;
	while (lo < hi) {
		const uint32_t step = (hi - lo + 63) / 64;
		const uint32_t idx = lo + lane * step;
		const bool le = idx < hi && a[idx] <= key;
		const uint64_t b = __ballot(le);
		const uint32_t run = b == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~b);   // the leading lanes that are <= key
		if (step == 1)
			return min(lo + run, hi);
		if (run == 0)
			return lo;
		const uint32_t nlo = lo + (run - 1) * step + 1, nhi = min(hi, lo + run * step);
		lo = nlo;
		hi = nhi;
	}
	return lo;
}

__device__ __forceinline__ uint32_t upper_bound64(const int64_t *a, uint32_t n, int64_t key)
{
	uint32_t lo = 0, hi = n;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (a[mid] <= key)
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo;
}

// the 16 bytes at text + sx, 0 <= sx and sx + 16 <= n
template <bool UNALIGNED>
__device__ __forceinline__ uint4 load_source(const uint8_t *text, int64_t sx)
{
	if (UNALIGNED) {
		uint4 v;
		__builtin_memcpy(&v, text + sx, 16);
		return v;
	}
	const uint4 *p = (const uint4 *)(text + (sx & ~(int64_t)15));
	const uint32_t sh = (uint32_t)sx & 15;
	const uint4 lo = p[0];
	if (sh == 0)
		return lo;
	const uint4 hi = p[1];   // (sh > 0: its first byte lies in front of sx + 16 <= n, so it is readable whole)
	const uint32_t b = sh & 3;
#define AB(h, l) __builtin_amdgcn_alignbyte(h, l, b)
	switch (sh >> 2) {
	case 0: return make_uint4(AB(lo.y, lo.x), AB(lo.z, lo.y), AB(lo.w, lo.z), AB(hi.x, lo.w));
	case 1: return make_uint4(AB(lo.z, lo.y), AB(lo.w, lo.z), AB(hi.x, lo.w), AB(hi.y, hi.x));
	case 2: return make_uint4(AB(lo.w, lo.z), AB(hi.x, lo.w), AB(hi.y, hi.x), AB(hi.z, hi.y));
	default: return make_uint4(AB(hi.x, lo.w), AB(hi.y, hi.x), AB(hi.z, hi.y), AB(hi.w, hi.z));
	}
#undef AB
}

// exclusive prefix maximum of v (>= 0) over the block in thread order, and the block's maximum.  red: kWaves cells.
__device__ __forceinline__ int64_t block_prefix_max64(int64_t v, int64_t *red, int64_t &total)
{
	const uint32_t lane = lane_id(), wave = threadIdx.x / 64;
	int64_t inc = v;
	for (int o = 1; o < 64; o <<= 1) {
		const int64_t up = __shfl_up((long long)inc, o, 64);
		inc = lane >= (uint32_t)o ? max(inc, up) : inc;
	}
	__syncthreads();
	if (lane == 63)
		red[wave] = inc;
	__syncthreads();
	int64_t before = 0;
	total = 0;
	for (uint32_t w = 0; w < (uint32_t)kWaves; w++) {
		before = w < wave ? max(before, red[w]) : before;
		total = max(total, red[w]);
	}
	const int64_t up = __shfl_up((long long)inc, 1, 64);
	return lane > 0 ? max(before, up) : before;
}

// 16 source bytes v, of which [lo, hi) go to tile[base + lo, base + hi): dwords where a whole one is owed
__device__ __forceinline__ void lds_put(uint8_t *tile, const uint4 &v, int lo, int hi, int base)
{
	const uint32_t w[6] = { 0, v.x, v.y, v.z, v.w, 0 };
	const int sh = base & 3, base4 = base - sh;   // (two's complement: sh in 0..3 for a negative base too)
#pragma unroll
	for (int k = 0; k < 5; k++) {
		// the destination dword at base4 + 4 * k holds source bytes i0 .. i0 + 3
		const int i0 = 4 * k - sh;
		if (i0 + 4 <= lo || i0 >= hi)
			continue;
		const uint32_t d = sh == 0 ? w[k + 1] : __builtin_amdgcn_alignbyte(w[k + 1], w[k], (uint32_t)(4 - sh));
		if (i0 >= lo && i0 + 4 <= hi) {
			*(uint32_t *)(tile + base4 + 4 * k) = d;
		} else {
#pragma unroll
			for (int c = 0; c < 4; c++)
				if (i0 + c >= lo && i0 + c < hi)
					tile[base4 + 4 * k + c] = (uint8_t)(d >> (8 * c));
		}
	}
}

}  // namespace acm_rp
