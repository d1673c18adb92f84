// The ordering step of the passes that group records by a small key (sequence.hip: by part, rule.hip: by
// operand): stable 8-bit LSD radix passes over (key, value) cells on the record-pass grid, and the emit step
// behind them: a record per flagged cell, in input order.  Internal to the library, gfx950 only.  DESIGN.md 6i.
//
// One radix pass is three launches over n cells, digit = (key >> shift) & 255:
//   k_radix_hist      per-block digit counts (the LDS atomics only count)
//   k_radix_offsets   their exclusive scan in (digit, block) order: a block per digit over the blocks' counts;
//                     the scatter adds the digits in front
//   k_radix_scatter   the scatter, ranks from wave ballots: cell order is kept among equal digits
// The kernels have internal linkage: every translation unit that includes this header has its own copies.
#pragma once

#include "record_pass.h"

namespace acm_rp {

constexpr uint32_t kNoKey = 0xFFFFFFFFu;   // the key of a cell that takes no part: ordered behind every other
constexpr uint32_t kDigits = 256;
// the radix kernels keep one digit per thread: h[tid], run[tid], wcnt[.. + tid]
static_assert(kThreads == kDigits, "a radix pass has one thread per digit");

struct RadixArgs {
	uint32_t n;                                      // the cells that are ordered
	const uint32_t *key_in, *val_in;
	uint32_t *key_out, *val_out;
	uint32_t shift;
	uint32_t *hist;                                  // [gridDim.x][256]
	uint32_t *digit_total;                           // [256] cells of each digit, of the radix pass at hand
};

// number of cells of the sorted a[0, n) that are < key
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t *a, uint32_t n, uint32_t key)
{
	uint32_t lo = 0, hi = n;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (a[mid] < key)
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo;
}

static __global__ __launch_bounds__(kThreads) void k_radix_hist(RadixArgs g)
{
	__shared__ uint32_t h[kDigits];

	const uint32_t tid = threadIdx.x;
	h[tid] = 0;
	__syncthreads();
	const Share sh = share_of((g.n + kTile - 1) / kTile);
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++)
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t i = t * kTile + q * kThreads + tid;
			if (i < g.n)
				atomicAdd(&h[(g.key_in[i] >> g.shift) & (kDigits - 1)], 1u);   // (a count: no order depends on it)
		}
	__syncthreads();
	g.hist[blockIdx.x * kDigits + tid] = h[tid];
}

// A block per digit d (a grid of kDigits blocks): hist[b][d] becomes the cells of digit d in the blocks in front of
// b, and digit_total[d] the cells of digit d; k_radix_scatter adds the cells of the digits in front.  Every block
// reads and writes its own column only.  blocks: the grid of the other launches; a thread takes a run of them.
static __global__ __launch_bounds__(kThreads) void k_radix_offsets(RadixArgs g, uint32_t blocks)
{
	__shared__ uint32_t red[kWaves];

	const uint32_t d = blockIdx.x;
	const uint32_t per = (blocks + kThreads - 1) / kThreads;
	const uint32_t b0 = min(threadIdx.x * per, blocks), b1 = min(b0 + per, blocks);
	uint32_t sum = 0;
	for (uint32_t b = b0; b < b1; b++)
		sum += g.hist[b * kDigits + d];
	uint32_t total;
	uint32_t at = block_prefix(sum, red, total);
	for (uint32_t b = b0; b < b1; b++) {
		const uint32_t c = g.hist[b * kDigits + d];
		g.hist[b * kDigits + d] = at;
		at += c;
	}
	if (threadIdx.x == 0)
		g.digit_total[d] = total;
}

static __global__ __launch_bounds__(kThreads) void k_radix_scatter(RadixArgs g)
{
	__shared__ uint32_t run[kDigits];             // the next output cell of each digit
	__shared__ uint32_t wcnt[kWaves * kDigits];   // cells of each digit in each wave of the row at hand
	__shared__ uint32_t red[kWaves];

	const uint32_t tid = threadIdx.x, wave = tid / 64;
	uint32_t all;
	const uint32_t digits_before = block_prefix(g.digit_total[tid], red, all);   // cells of the digits in front of tid
	run[tid] = digits_before + g.hist[blockIdx.x * kDigits + tid];
	for (int w = 0; w < kWaves; w++)
		wcnt[w * kDigits + tid] = 0;
	__syncthreads();
	const Share sh = share_of((g.n + kTile - 1) / kTile);
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++)
		for (int q = 0; q < kPer; q++) {   // a row of kThreads cells: cell order is (row, thread)
			const uint32_t i = t * kTile + q * kThreads + tid;
			const bool valid = i < g.n;
			const uint32_t key = valid ? g.key_in[i] : 0, val = valid ? g.val_in[i] : 0;
			const uint32_t digit = (key >> g.shift) & (kDigits - 1);
			uint64_t same = __ballot(valid);   // the lanes of this wave with this lane's digit
#pragma unroll
			for (int b = 0; b < 8; b++) {
				const bool bit = (digit >> b) & 1;
				const uint64_t v = __ballot(bit);
				same &= bit ? v : ~v;
			}
			const uint32_t rank = mbcnt64(same);
			if (valid && rank == 0)
				wcnt[wave * kDigits + digit] = (uint32_t)__popcll(same);
			__syncthreads();
			if (valid) {
				uint32_t dst = run[digit] + rank;
				for (uint32_t w = 0; w < wave; w++)
					dst += wcnt[w * kDigits + digit];
				if (dst < g.n) {   // (always: the counts are those of k_radix_hist)
					g.key_out[dst] = key;
					g.val_out[dst] = val;
				}
			}
			__syncthreads();
			uint32_t c = 0;
			for (int w = 0; w < kWaves; w++) {
				c += wcnt[w * kDigits + tid];
				wcnt[w * kDigits + tid] = 0;
			}
			run[tid] += c;
			__syncthreads();
		}
}

// ---- the flagged cells, in input order ----

// The count launch (WRITE false) and the write launch (WRITE true) of a pass that keeps the cells i < m with
// emit[i] != 0, in order: the count leaves every block's cells in counts[blockIdx.x]; the write calls
// ends(total) in thread 0 of block 0 (the header and trailer cells, the info) and put(i, d) for kept cell i,
// the d-th of all, where d + 2 < cap.  Called by every thread of the block.  wave_cnt: kPer * kWaves cells of
// LDS, red: 2 * kWaves.
template <bool WRITE, class Ends, class Put>
__device__ __forceinline__ void emit_flagged(const uint32_t *emit, uint32_t m, int32_t *counts, uint32_t cap, uint32_t *wave_cnt,
    uint32_t *red, Ends ends, Put put)
{
	const uint32_t tid = threadIdx.x;
	const Share sh = share_of((m + kTile - 1) / kTile);
	uint32_t base = 0;
	if (WRITE) {
		uint32_t total;
		base = blocks_before(counts, red, total);
		if (blockIdx.x == 0 && tid == 0)
			ends(total);
	}
	uint32_t kept = 0;
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++) {
		uint32_t flag[kPer], incl[kPer], wave_total[kPer];
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t i = t * kTile + q * kThreads + tid;
			flag[q] = i < m ? (emit[i] != 0) : 0u;
			kept += flag[q];
		}
		if (!WRITE)
			continue;
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			incl[q] = wave_inclusive(flag[q]);
			wave_total[q] = (uint32_t)__shfl((int)incl[q], 63, 64);
		}
		tile_publish(wave_total, wave_cnt);
		uint32_t tile_total = 0;
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t i = t * kTile + q * kThreads + tid;
			const uint32_t d = base + tile_row(wave_cnt, q, tile_total) + incl[q] - flag[q];
			if (flag[q] && d + 2 < cap)
				put(i, d);
		}
		base += tile_total;
	}
	if (!WRITE) {
		kept = block_sum(kept, red);
		if (tid == 0)
			counts[blockIdx.x] = (int32_t)kept;
	}
}

// ---- host side ----

// 8-bit passes that order keys in [0, keys] (keys: the key count; kNoKey orders through its low digits, which are
// the last in every pass)
inline uint32_t radix_passes(uint32_t keys)
{
	uint32_t passes = 1;
	while (passes < 4 && ((uint64_t)keys >> (8 * passes)) != 0)
		passes++;
	return passes;
}

inline size_t radix_hist_bytes(uint32_t blocks) { return round256((size_t)blocks * kDigits * sizeof(uint32_t)); }
inline size_t radix_digit_total_bytes() { return round256(kDigits * sizeof(uint32_t)); }

// Enqueues the passes that order the n cells of (key[0], val[0]) by key, ping-ponging with (key[1], val[1]);
// returns the buffer pair that holds the ordered cells.  grid: the record-pass grid of n.  3 * passes launches.
inline hipError_t radix_order(uint32_t n, uint32_t *const key[2], uint32_t *const val[2], uint32_t *hist, uint32_t *digit_total,
    uint32_t passes, uint32_t blocks, hipStream_t s, int &cur)
{
	RadixArgs r{};
	r.n = n;
	r.hist = hist;
	r.digit_total = digit_total;
	cur = 0;
	for (uint32_t k = 0; k < passes; k++) {
		r.key_in = key[cur];
		r.val_in = val[cur];
		r.key_out = key[cur ^ 1];
		r.val_out = val[cur ^ 1];
		r.shift = 8 * k;
		hipLaunchKernelGGL(k_radix_hist, dim3(blocks), dim3(kThreads), 0, s, r);
		if (hipError_t e = hipGetLastError())
			return e;
		hipLaunchKernelGGL(k_radix_offsets, dim3(kDigits), dim3(kThreads), 0, s, r, blocks);
		if (hipError_t e = hipGetLastError())
			return e;
		hipLaunchKernelGGL(k_radix_scatter, dim3(blocks), dim3(kThreads), 0, s, r);
		if (hipError_t e = hipGetLastError())
			return e;
		cur ^= 1;
	}
	return hipSuccess;
}

}  // namespace acm_rp
