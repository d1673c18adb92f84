// The record-pass core: what the passes that run behind a scan (segment.hip, tally.hip, lines.hip, sequence.hip,
// rule.hip, select.hip, rewrite.hip, through range_pack.h extract.hip and format.hip, expand in post.hip, and through entry_pass.h word.hip, case.hip, position.hip, wildcard.hip and approx.hip) share.  Internal to the
// library, gfx950 only.  DESIGN.md 6f.
//
// A pass runs a fixed grid of at most kMaxBlocks blocks of kThreads threads.  Every block owns a
// contiguous run of tiles (share_of); a tile of records is kPer rows of kThreads, row q holding records
// r0 + q * kThreads + tid.  A pass that writes in position order takes two launches: the first leaves
// every block's count in block_counts[blockIdx.x], the second sums the counts of the blocks in front of
// its own (blocks_before), ranks its cells inside each tile (tile_publish and tile_row, or block_prefix)
// and writes; block 0 writes the header and trailer cells (write_ends).  No atomics for ordering.
// The LDS arrays the helpers use are declared by the kernels and passed in, so that a kernel's LDS
// footprint stays visible where it is budgeted.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace acm_rp {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPer = 4;                      // records per thread per tile
constexpr uint32_t kTile = kThreads * kPer;  // 1024
constexpr uint32_t kSliceMax = 2048;         // segment starts staged in LDS per tile (8 KiB)
constexpr uint32_t kMaxBlocks = 1024;        // 4 blocks of 256 threads on each of 256 CUs

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0)); }

// bits of m below this lane
__device__ __forceinline__ uint32_t mbcnt64(uint64_t m)
{
	return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

// number of cells of the sorted a[0, n) that are <= key.  K: int32_t, or int64_t for a key that may lie
// outside the cells' range; the cells are compared in K.
template <typename K>
__device__ __forceinline__ uint32_t upper_bound_i32(const int32_t *a, uint32_t n, K key)
{
	uint32_t lo = 0, hi = n;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if ((K)a[mid] <= key)
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo;
}

// The same, found by the whole wave: 64 samples per step, each step shrinks the range 64-fold (three
// steps for 240 k segments).  Every lane passes the same key and gets the same answer, in [0, n].
__device__ inline uint32_t wave_upper_bound(const int32_t *a, uint32_t n, int64_t key)
{
	const uint32_t lane = lane_id();
	uint32_t lo = 0, hi = n;   // the answer lies in [lo, hi]
	while (lo < hi) {
		const uint32_t step = (hi - lo + 63) / 64;
		const uint32_t idx = lo + lane * step;
		const bool le = idx < hi && (int64_t)a[idx] <= key;
		const uint32_t c = (uint32_t)__popcll(__ballot(le));   // a prefix of the lanes: a is sorted
		if (step == 1)
			return lo + c;
		if (c == 0)
			return lo;
		const uint32_t nlo = lo + (c - 1) * step + 1, nhi = min(hi, lo + c * step);
		lo = nlo;
		hi = nhi;
	}
	return lo;
}

// ---- block primitives (called by every thread of the block; red: cells of LDS) ----

// sum over the block of one value per wave (v is uniform over the wave).  Every thread gets the sum.
// red: kWaves cells.
__device__ __forceinline__ uint32_t block_sum_of_waves(uint32_t v, uint32_t *red)
{
	__syncthreads();   // (red of an earlier call is no longer read)
	if (lane_id() == 0)
		red[threadIdx.x / 64] = v;
	__syncthreads();
	uint32_t s = 0;
	for (int w = 0; w < kWaves; w++)
		s += red[w];
	return s;
}

// sum over the block of v.  Every thread gets the sum.  red: kWaves cells.
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *red)
{
	for (int o = 32; o > 0; o >>= 1)
		v += __shfl_xor(v, o, 64);
	return block_sum_of_waves(v, red);
}

// inclusive prefix of v over the lanes of the wave
__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v)
{
	const uint32_t lane = lane_id();
	for (int o = 1; o < 64; o <<= 1) {
		const uint32_t up = __shfl_up(v, o, 64);
		v += lane >= (uint32_t)o ? up : 0;
	}
	return v;
}

// exclusive prefix of v over the block in thread order, and the block's total.  red: kWaves cells.
__device__ __forceinline__ uint32_t block_prefix(uint32_t v, uint32_t *red, uint32_t &total)
{
	const uint32_t lane = lane_id(), wave = threadIdx.x / 64;
	const uint32_t inc = wave_inclusive(v);
	__syncthreads();
	if (lane == 63)
		red[wave] = inc;
	__syncthreads();
	uint32_t before = 0;
	total = 0;
	for (uint32_t w = 0; w < (uint32_t)kWaves; w++) {
		before += w < wave ? red[w] : 0;
		total += red[w];
	}
	return before + inc - v;
}

// counts of the blocks in front of this one, and of all blocks: both sums in one pass.  red: 2 * kWaves
// cells.
__device__ __forceinline__ uint32_t blocks_before(const int32_t *block_counts, uint32_t *red, uint32_t &all)
{
	const uint32_t wave = threadIdx.x / 64;
	uint32_t before = 0, sum = 0;
	for (uint32_t j = threadIdx.x; j < gridDim.x; j += kThreads) {
		const uint32_t c = (uint32_t)block_counts[j];
		sum += c;
		before += j < blockIdx.x ? c : 0;
	}
	for (int o = 32; o > 0; o >>= 1) {
		before += __shfl_xor(before, o, 64);
		sum += __shfl_xor(sum, o, 64);
	}
	__syncthreads();   // (red of an earlier call is no longer read)
	if (lane_id() == 0) {
		red[wave] = before;
		red[kWaves + wave] = sum;
	}
	__syncthreads();
	before = all = 0;
	for (int w = 0; w < kWaves; w++) {
		before += red[w];
		all += red[kWaves + w];
	}
	return before;
}

// ---- tile ownership ----

struct Share {
	uint32_t t_begin, t_end;   // the block's tiles
};

__device__ __forceinline__ Share share_of(uint32_t tiles)
{
	const uint32_t per = (tiles + gridDim.x - 1) / gridDim.x;
	const uint32_t t_begin = min(blockIdx.x * per, tiles);
	return Share{ t_begin, min(t_begin + per, tiles) };
}

// ---- the segment starts a tile spans ----

struct Slice {
	uint32_t ub0, ub1;   // starts <= the offset of the tile's first and of its last record
	uint32_t k0, len;    // starts [k0, k0 + len) are in LDS when in_lds (len <= kSliceMax)
	bool in_lds;
};

// Finds the slice of seg_start that the records [r0, r1) of a tile fall in (records and starts are both
// in offset order) and stages it in slice[kSliceMax] when it fits; bounds: 2 cells of LDS.  Called by
// every thread of the block.  When in_lds (uniform over the block) the slice may be read after the
// caller's next barrier.
__device__ __forceinline__ Slice stage_slice(const int32_t *off_plane, uint32_t r0, uint32_t r1, const int32_t *seg_start,
    uint32_t segments, int32_t *slice, uint32_t *bounds)
{
	const uint32_t wave = threadIdx.x / 64;
	__syncthreads();   // (the slice of the previous tile is no longer read)
	if (wave < 2) {
		const uint32_t ub = wave_upper_bound(seg_start, segments, (int64_t)off_plane[1 + (wave == 0 ? r0 : r1 - 1)]);
		if (lane_id() == 0)
			bounds[wave] = ub;
	}
	__syncthreads();
	Slice s;
	s.ub0 = bounds[0];
	s.ub1 = bounds[1];
	s.k0 = s.ub0 > 0 ? s.ub0 - 1 : 0;
	s.len = s.ub1 - s.k0;
	s.in_lds = s.len <= kSliceMax;
	if (s.in_lds)
		for (uint32_t j = threadIdx.x; j < s.len; j += kThreads)
			slice[j] = seg_start[s.k0 + j];
	return s;
}

// number of starts <= o (the segment of o is that minus one): in the staged slice, else (a tile whose
// slice is larger than the LDS budget: many empty segments) in global memory
__device__ __forceinline__ uint32_t starts_le(const Slice &s, const int32_t *slice, const int32_t *seg_start, uint32_t segments,
    int32_t o)
{
	return s.in_lds ? s.k0 + upper_bound_i32(slice, s.len, o) : upper_bound_i32(seg_start, segments, o);
}

// The text [lo, hi) a record lies in, from ub = the number of starts <= its offset (in [0, segments]):
// lo is start ub - 1 and hi is start ub; where there is no such start the bound is left as it was.
// start_at(k): start number k < segments, from wherever the caller keeps it.
template <class StartAt>
__device__ __forceinline__ void text_bounds(uint32_t ub, uint32_t segments, StartAt start_at, int64_t &lo, int64_t &hi)
{
	if (ub > 0)
		lo = start_at(ub - 1);
	if (ub < segments)
		hi = start_at(ub);
}

// ---- ordered rank inside a tile ----

// A tile's cells are ranked row by row (the first cells of all kPer rows at once cost k_word<true> 12
// VGPRs and a step of occupancy):
//   tile_publish   wave_total[q]: the cells of row q that this wave writes, uniform over the wave
//   tile_row       for q = 0 .. kPer - 1 in order: the cells of the tile in front of this wave's of row q
//                  (every row q' < q, then the waves w' < wave of row q); adds row q to tile_total
// The rank inside the wave is the caller's: mbcnt64 of a ballot for counts of 0 or 1, else wave_inclusive.
// wave_cnt: kPer * kWaves cells of LDS.  Both are called by every thread of the block.
__device__ __forceinline__ void tile_publish(const uint32_t (&wave_total)[kPer], uint32_t *wave_cnt)
{
	__syncthreads();   // (wave_cnt of the previous tile is no longer read)
	if (lane_id() == 0)
#pragma unroll
		for (int q = 0; q < kPer; q++)
			wave_cnt[q * kWaves + threadIdx.x / 64] = wave_total[q];
	__syncthreads();
}

__device__ __forceinline__ uint32_t tile_row(const uint32_t *wave_cnt, int q, uint32_t &tile_total)
{
	const uint32_t wave = threadIdx.x / 64;
	uint32_t before = tile_total;
	for (uint32_t w = 0; w < (uint32_t)kWaves; w++) {
		before += w < wave ? wave_cnt[q * kWaves + w] : 0;
		tile_total += wave_cnt[q * kWaves + w];
	}
	return before;
}

// ---- the span of a record ----

// What a record (p, o) of a pattern plane covers in the text, for the passes that need where a match begins and ends
// (select.hip, rewrite.hip; the contract is acm_select_matches_async's): [s, e] = [o - L + 1 - pre, o + post], int64,
// L the pattern's length and pre, post its wildcard context (both 0 without one).  ok: p is a pattern index and
// L >= 1.  pat_len: [patterns]; wild_ent: [patterns] {cell index, pre, post, length}, or null for a set without contexts.
struct Span {
	int64_t s, e;
	bool ok;
};

__device__ __forceinline__ Span span_of(const uint32_t *pat_len, const int4 *wild_ent, uint32_t num_patterns, uint32_t p, int32_t o)
{
	Span sp{ 0, 0, false };
	if (p >= num_patterns)   // (a cell may hold anything)
		return sp;
	int64_t L, pre = 0, post = 0;
	if (wild_ent) {
		const int4 w = wild_ent[p];
		pre = w.y;
		post = w.z;
		L = w.w;
	} else {
		L = pat_len[p];
	}
	sp.ok = L >= 1;
	sp.s = (int64_t)o - L + 1 - pre;
	sp.e = (int64_t)o + post;
	return sp;
}

// ---- output planes ----

// The header and trailer cells of an output plane of cap >= 2 cells, as the scan writes them: the count,
// and `last` behind the records (in the last cell when there are more records than cap - 2).
__device__ __forceinline__ void write_ends(int32_t *plane, uint32_t cap, uint32_t total, int32_t last)
{
	plane[0] = (int32_t)total;
	plane[min(total + 1, cap - 1)] = last;
}

// ---- host side ----

inline size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

// blocks of the fixed grid of a pass over at most max_records records
inline uint32_t grid_for(size_t max_records)
{
	const size_t tiles = (max_records + kTile - 1) / kTile;
	return (uint32_t)std::max<size_t>(1, std::min<size_t>(tiles, kMaxBlocks));
}

// the workspace of a two-launch pass: block_counts
inline size_t block_counts_bytes(uint32_t blocks) { return round256((size_t)blocks * sizeof(int32_t)); }

// out_capacity as the kernels take it
inline uint32_t clamp_cap(size_t out_capacity) { return (uint32_t)std::min<size_t>(out_capacity, 0xFFFFFFFFul); }

}  // namespace acm_rp
