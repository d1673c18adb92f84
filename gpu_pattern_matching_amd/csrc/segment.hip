// Segmented scans: many independent texts in one scan.  gfx950 only.
//
// Let s(p) be the state of the serial walk after byte p and b the bytes of p's segment up to and
// including p.  The state a walk restarted at the segment's start would be in is the first state on
// the fail chain s, fail(s), fail(fail(s)), ... whose trie depth is <= b: s(p) is the longest suffix
// of all bytes scanned so far that is a trie node, its fail chain lists every such suffix longest
// first, and the per-segment state is the longest of them that lies inside the segment.  Match lists
// inherit along fail links, so where the per-segment state is final s(p) is final too: the records
// of an ordinary ACM_REPORT_STATE scan, each clamped by depth, less those whose clamped state has an
// empty match list, are the segmented scan's records.  The scan kernels stay as they are; this pass
// costs per record, not per text byte, and the clamp only does work within max_pattern_len bytes of
// a segment start.
//
// Two launches over a fixed grid (every block owns a contiguous run of 1024-record tiles):
//   k_segment<false>  clamps every record and writes the number its block keeps
//   k_segment<true>   clamps again, sums the counts of the blocks in front of its own, and writes
//                     the kept records in position order: ranks inside a wave from a 64-bit ballot
//                     and mbcnt, across the block's waves from LDS, no atomics for ordering
// The segment of a record is found in the slice of the start array that its tile spans, staged in
// LDS (a wave-wide 64-ary search finds the slice's bounds); a tile whose slice is larger than the
// LDS budget (many empty segments) searches the start array in global memory instead.
#include <hip/hip_runtime.h>

#include "acm_internal.h"
#include "device_dfa.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPer = 4;                      // records per thread per tile
constexpr uint32_t kTile = kThreads * kPer;  // 1024
constexpr uint32_t kSliceMax = 2048;         // segment starts staged in LDS per tile (8 KiB)
constexpr uint32_t kMaxBlocks = 1024;

struct SegArgs {
	const int32_t *state_plane, *off_plane;
	uint32_t max_records;
	const int32_t *seg_start;
	uint32_t segments;
	int64_t text_end;
	const uint2 *fail_depth;     // [ref state] {fail, depth}
	const uint32_t *list_begin, *list_len;
	const int32_t *list_pool;
	uint32_t num_states, max_depth;
	int report;
	int32_t *pat_out, *off_out, *seg_out;
	uint32_t cap;
	int32_t *seg_counts;
	int32_t *block_counts;       // [gridDim.x]
};

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0)); }

__device__ __forceinline__ uint32_t mbcnt64(uint64_t m)
{
	return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

// Number of starts <= key (so the segment is that minus one), found by the whole wave: 64 samples per
// step, each step shrinks the range 64-fold (three steps for 240 k segments).  Every lane passes the
// same key and gets the same answer.
__device__ uint32_t wave_upper_bound(const int32_t *a, uint32_t n, int64_t key)
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

__device__ __forceinline__ uint32_t upper_bound_i32(const int32_t *a, uint32_t n, int32_t key)
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

// the first state on s's fail chain whose depth is <= b
__device__ __forceinline__ uint32_t clamp_state(const SegArgs &g, uint32_t s, int64_t b)
{
	if (b >= (int64_t)g.max_depth)   // the common case: no state is that deep
		return s;
	uint2 fd = g.fail_depth[s];
	while ((int64_t)fd.y > b) {
		s = fd.x;
		fd = g.fail_depth[s];
	}
	return s;
}

struct Staged {
	uint32_t k0, len;   // starts [k0, k0 + len) of the tile are in LDS (len <= kSliceMax), else global
	bool in_lds;
};

// One record: its segment, its clamped state, whether it survives and the value it reports.
__device__ __forceinline__ bool one_record(const SegArgs &g, int32_t o, uint32_t s, const int32_t *slice,
    const Staged &st, int32_t &val, int32_t &seg)
{
	if (s >= g.num_states)   // not the planes of a STATE scan: nothing to report
		return false;
	const uint32_t s_in = s;
	int32_t k = -1;
	if (g.segments) {
		const uint32_t ub = st.in_lds ? st.k0 + upper_bound_i32(slice, st.len, o)
		                              : upper_bound_i32(g.seg_start, g.segments, o);
		k = (int32_t)ub - 1;
		if (k >= 0)
			s = clamp_state(g, s, (int64_t)o - g.seg_start[k] + 1);
	}
	seg = k;
	if (s != s_in && g.list_len[s] == 0)
		return false;
	val = g.report == ACM_REPORT_HEAD ? g.list_pool[g.list_begin[s]] : (int32_t)s;
	return true;
}

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void k_segment(SegArgs g)
{
	__shared__ int32_t slice[kSliceMax];
	__shared__ uint32_t bounds[2];
	__shared__ uint32_t wave_cnt[kPer * kWaves];
	__shared__ uint32_t red[kWaves * 2];

	const uint32_t tid = threadIdx.x, wave = tid / 64, lane = lane_id();
	const uint32_t m = min((uint32_t)g.state_plane[0], g.max_records);
	const uint32_t tiles = (m + kTile - 1) / kTile, per = (tiles + gridDim.x - 1) / gridDim.x;
	const uint32_t t_begin = min(blockIdx.x * per, tiles), t_end = min(t_begin + per, tiles);

	if (WRITE && t_begin == t_end && blockIdx.x != 0)   // nothing to write (a batch with few records)
		return;
	uint32_t base = 0;   // WRITE: records kept by the blocks in front of this one
	if (WRITE) {
		uint32_t before = 0, all = 0;
		for (uint32_t j = tid; j < gridDim.x; j += kThreads) {
			const uint32_t c = (uint32_t)g.block_counts[j];
			all += c;
			before += j < blockIdx.x ? c : 0;
		}
		for (int o = 32; o > 0; o >>= 1) {
			before += __shfl_xor(before, o, 64);
			all += __shfl_xor(all, o, 64);
		}
		if (lane == 0) {
			red[wave] = before;
			red[kWaves + wave] = all;
		}
		__syncthreads();
		uint32_t total = 0;
		for (int w = 0; w < kWaves; w++) {
			base += red[w];
			total += red[kWaves + w];
		}
		if (blockIdx.x == 0 && wave == 0) {   // header and trailer cells, as the scan writes them
			uint32_t last = (uint32_t)g.state_plane[1 + m];
			if (g.segments && last < g.num_states) {
				const uint32_t ub = wave_upper_bound(g.seg_start, g.segments, g.text_end);
				if (ub > 0)
					last = clamp_state(g, last, g.text_end - g.seg_start[ub - 1]);
			}
			if (lane == 0) {
				const uint32_t tail = min(total + 1, g.cap - 1);
				g.pat_out[0] = (int32_t)total;
				g.off_out[0] = (int32_t)total;
				g.pat_out[tail] = (int32_t)last;
				g.off_out[tail] = (int32_t)last;
				if (g.seg_out) {
					g.seg_out[0] = (int32_t)total;
					g.seg_out[tail] = (int32_t)last;
				}
			}
		}
	}

	uint32_t kept = 0;
	for (uint32_t t = t_begin; t < t_end; t++) {
		const uint32_t r0 = t * kTile, r1 = min(r0 + kTile, m);
		int32_t off[kPer];
		uint32_t state[kPer];
#pragma unroll
		for (int q = 0; q < kPer; q++) {   // loaded first: in flight while the slice is found and staged
			const uint32_t i = r0 + q * kThreads + tid;
			off[q] = i < r1 ? g.off_plane[1 + i] : 0;
			state[q] = i < r1 ? (uint32_t)g.state_plane[1 + i] : 0;
		}
		Staged st{ 0, 0, false };
		if (g.segments) {
			__syncthreads();   // (the slice of the previous tile is no longer read)
			if (wave < 2) {
				const uint32_t ub = wave_upper_bound(g.seg_start, g.segments,
				    (int64_t)g.off_plane[1 + (wave == 0 ? r0 : r1 - 1)]);
				if (lane == 0)
					bounds[wave] = ub;
			}
			__syncthreads();
			st.k0 = bounds[0] > 0 ? bounds[0] - 1 : 0;
			st.len = bounds[1] - st.k0;
			st.in_lds = st.len <= kSliceMax;
			if (st.in_lds) {
				for (uint32_t j = tid; j < st.len; j += kThreads)
					slice[j] = g.seg_start[st.k0 + j];
				__syncthreads();
			}
		}
		bool keep[kPer];
		int32_t val[kPer], seg[kPer];
		uint64_t mask[kPer];
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t i = r0 + q * kThreads + tid;
			val[q] = 0;
			seg[q] = -1;
			keep[q] = i < r1 && one_record(g, off[q], state[q], slice, st, val[q], seg[q]);
			mask[q] = __ballot(keep[q]);
		}
		if (!WRITE) {
#pragma unroll
			for (int q = 0; q < kPer; q++)
				kept += (uint32_t)__popcll(mask[q]);
			continue;
		}
		if (lane == 0)
#pragma unroll
			for (int q = 0; q < kPer; q++)
				wave_cnt[q * kWaves + wave] = (uint32_t)__popcll(mask[q]);
		__syncthreads();
		uint32_t tile_total = 0;
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			// record r0 + q * 256 + tid: behind every record of rows q' < q, then of waves w' < wave of row q
			uint32_t before = base + tile_total;
			for (uint32_t w = 0; w < (uint32_t)kWaves; w++)
				before += w < wave ? wave_cnt[q * kWaves + w] : 0;
			for (uint32_t w = 0; w < (uint32_t)kWaves; w++)
				tile_total += wave_cnt[q * kWaves + w];
			const uint32_t d = before + mbcnt64(mask[q]);
			if (keep[q] && d + 2 < g.cap) {
				g.pat_out[1 + d] = val[q];
				g.off_out[1 + d] = off[q];
				if (g.seg_out)
					g.seg_out[1 + d] = seg[q];
			}
			if (g.seg_counts) {
				// records kept per segment: one atomic per run of a segment within the wave (records are
				// in position order, so a segment's records are consecutive among the kept lanes)
				const uint64_t lt = (1ull << lane) - 1;
				const uint64_t prior = mask[q] & lt;
				const int prev = prior ? 63 - __clzll((long long)prior) : (int)lane;
				const int32_t pseg = __shfl(seg[q], prev, 64);
				const bool head = keep[q] && seg[q] >= 0 && (!prior || pseg != seg[q]);
				const uint64_t heads = __ballot(head);
				if (head) {
					const uint64_t above = heads & ~(lt | (1ull << lane));
					const uint64_t upto = above ? ((1ull << (__ffsll((long long)above) - 1)) - 1) : ~0ull;
					atomicAdd(&g.seg_counts[seg[q]], (int32_t)__popcll(mask[q] & upto & ~lt));
				}
			}
		}
		base += tile_total;
		__syncthreads();   // (wave_cnt is rewritten by the next tile)
	}
	if (!WRITE) {
		if (lane == 0)
			red[wave] = kept;
		__syncthreads();
		if (tid == 0) {
			uint32_t sum = 0;
			for (int w = 0; w < kWaves; w++)
				sum += red[w];
			g.block_counts[blockIdx.x] = (int32_t)sum;
		}
	}
}

uint32_t grid_for(size_t max_records)
{
	const size_t tiles = (max_records + kTile - 1) / kTile;
	return (uint32_t)std::max<size_t>(1, std::min<size_t>(tiles, kMaxBlocks));
}

}  // namespace

extern "C" size_t acm_segment_workspace_bytes(size_t max_records)
{
	return ((size_t)grid_for(max_records) * sizeof(int32_t) + 255) & ~(size_t)255;
}

extern "C" int acm_segment_matches_async(const acm_dfa *d, const int32_t *d_state_plane, const int32_t *d_off_plane,
    size_t max_records, const int32_t *d_seg_start, size_t segments, long text_end, int report, int32_t *d_pat_out,
    int32_t *d_off_out, int32_t *d_seg_out, size_t out_capacity, int32_t *d_seg_counts, void *d_workspace,
    size_t workspace_bytes, void *stream)
{
	if (!d || !d_state_plane || !d_off_plane || !d_pat_out || !d_off_out || out_capacity < 2 ||
	    max_records > 0x7FFFFFFEul || (segments && !d_seg_start) || segments > 0x7FFFFFFFul ||
	    (report != ACM_REPORT_HEAD && report != ACM_REPORT_STATE))
		return acm::fail(ACM_ERR_ARG, "acm_segment_matches_async: bad arguments");
	if (!d->d_fail_depth)
		return acm::fail(ACM_ERR_ARG, "acm_segment_matches_async: automaton has no fail/depth table");
	if (!d_workspace || workspace_bytes < acm_segment_workspace_bytes(max_records))
		return acm::fail(ACM_ERR_ARG, "acm_segment_matches_async: workspace %zu B < required %zu B", workspace_bytes,
		    acm_segment_workspace_bytes(max_records));
	hipStream_t s = (hipStream_t)stream;
	ACM_HIP_TRY(hipSetDevice(d->device));
	SegArgs g;
	g.state_plane = d_state_plane;
	g.off_plane = d_off_plane;
	g.max_records = (uint32_t)max_records;
	g.seg_start = d_seg_start;
	g.segments = (uint32_t)segments;
	g.text_end = (int64_t)text_end;
	g.fail_depth = (const uint2 *)d->d_fail_depth;
	g.list_begin = d->d_list_begin;
	g.list_len = d->d_list_len;
	g.list_pool = d->d_list_pool;
	g.num_states = d->num_states;
	g.max_depth = d->max_pattern_len;
	g.report = report;
	g.pat_out = d_pat_out;
	g.off_out = d_off_out;
	g.seg_out = d_seg_out;
	g.cap = (uint32_t)(out_capacity > 0xFFFFFFFFul ? 0xFFFFFFFFul : out_capacity);
	g.seg_counts = segments ? d_seg_counts : nullptr;
	g.block_counts = (int32_t *)d_workspace;
	const uint32_t blocks = grid_for(max_records);
	if (g.seg_counts)
		ACM_HIP_TRY(hipMemsetAsync(g.seg_counts, 0, segments * sizeof(int32_t), s));
	hipLaunchKernelGGL(k_segment<false>, dim3(blocks), dim3(kThreads), 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_segment<true>, dim3(blocks), dim3(kThreads), 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}
