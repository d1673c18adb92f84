// ASCII case folding (acm_automaton_set_nocase): fold(b) = b - 0x20 for 'a' <= b <= 'z', b otherwise
// -- toupper in the C locale; bytes >= 0x80 stay as they are.  One definition for the host (pattern
// bytes, tables) and the kernels (text bytes where they are compared with pattern bytes or hashed).
// The word forms fold every byte lane at once, without a carry between lanes: l + 0x1F sets bit 7
// of a lane for l >= 'a', l + 0x05 for l > 'z'; bit 7 of the byte itself excludes 0x80..0xFF.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace acm {

__host__ __device__ __forceinline__ uint32_t fold_byte(uint32_t b)
{
	return b - 0x61u <= 0x19u ? b - 0x20u : b;
}

__host__ __device__ __forceinline__ uint32_t fold32(uint32_t x)
{
	const uint32_t l = x & 0x7F7F7F7Fu;
	const uint32_t m = (l + 0x1F1F1F1Fu) & ~(l + 0x05050505u) & ~x & 0x80808080u;
	return x ^ (m >> 2);
}

__host__ __device__ __forceinline__ uint64_t fold64(uint64_t x)
{
	const uint64_t l = x & 0x7F7F7F7F7F7F7F7Full;
	const uint64_t m = (l + 0x1F1F1F1F1F1F1F1Full) & ~(l + 0x0505050505050505ull) & ~x & 0x8080808080808080ull;
	return x ^ (m >> 2);
}

// the byte as the automaton sees it: folded when NOCASE
template <bool NOCASE>
__host__ __device__ __forceinline__ uint32_t fold_if(uint32_t b)
{
	return NOCASE ? fold_byte(b) : b;
}

}  // namespace acm
