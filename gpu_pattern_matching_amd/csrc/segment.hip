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
// The pass is a two-launch ordered write over a fixed grid (record_pass.h):
//   k_segment<false>  clamps every record and writes the number its block keeps
//   k_segment<true>   clamps again and writes the kept records in position order, ranks inside a wave
//                     from a 64-bit ballot
// The segment of a record is found in the slice of the start array that its tile spans (stage_slice).
#include <hip/hip_runtime.h>

#include "acm_internal.h"
#include "device_dfa.h"
#include "record_pass.h"

namespace {

using namespace acm_rp;

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

// One record: its segment, its clamped state, whether it survives and the value it reports.
__device__ __forceinline__ bool one_record(const SegArgs &g, int32_t o, uint32_t s, const int32_t *slice,
    const Slice &st, int32_t &val, int32_t &seg)
{
	if (s >= g.num_states)   // not the planes of a STATE scan: nothing to report
		return false;
	const uint32_t s_in = s;
	int32_t k = -1;
	if (g.segments) {
		k = (int32_t)starts_le(st, slice, g.seg_start, g.segments, o) - 1;
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
	__shared__ uint32_t red[2 * kWaves];

	const uint32_t tid = threadIdx.x, lane = lane_id();
	const uint32_t m = min((uint32_t)g.state_plane[0], g.max_records);
	const Share sh = share_of((m + kTile - 1) / kTile);

	if (WRITE && sh.t_begin == sh.t_end && blockIdx.x != 0)   // nothing to write (a batch with few records)
		return;
	uint32_t base = 0;   // WRITE: records kept by the blocks in front of this one
	if (WRITE) {
		uint32_t total;
		base = blocks_before(g.block_counts, red, total);
		if (blockIdx.x == 0 && tid < 64) {   // the trailer: the input's, clamped at the text's end
			uint32_t last = (uint32_t)g.state_plane[1 + m];
			if (g.segments && last < g.num_states) {
				const uint32_t ub = wave_upper_bound(g.seg_start, g.segments, g.text_end);
				if (ub > 0)
					last = clamp_state(g, last, g.text_end - g.seg_start[ub - 1]);
			}
			if (lane == 0) {
				write_ends(g.pat_out, g.cap, total, (int32_t)last);
				write_ends(g.off_out, g.cap, total, (int32_t)last);
				if (g.seg_out)
					write_ends(g.seg_out, g.cap, total, (int32_t)last);
			}
		}
	}

	uint32_t kept = 0;
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++) {
		const uint32_t r0 = t * kTile, r1 = min(r0 + kTile, m);
		int32_t off[kPer];
		uint32_t state[kPer];
#pragma unroll
		for (int q = 0; q < kPer; q++) {   // loaded first: in flight while the slice is found and staged
			const uint32_t i = r0 + q * kThreads + tid;
			off[q] = i < r1 ? g.off_plane[1 + i] : 0;
			state[q] = i < r1 ? (uint32_t)g.state_plane[1 + i] : 0;
		}
		Slice st{};
		if (g.segments) {
			st = stage_slice(g.off_plane, r0, r1, g.seg_start, g.segments, slice, bounds);
			if (st.in_lds)
				__syncthreads();
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
			kept += (uint32_t)__popcll(mask[q]);   // (of the wave)
		}
		if (!WRITE)
			continue;
		uint32_t wave_total[kPer];
#pragma unroll
		for (int q = 0; q < kPer; q++)
			wave_total[q] = (uint32_t)__popcll(mask[q]);
		tile_publish(wave_total, wave_cnt);
		uint32_t tile_total = 0;
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t d = base + tile_row(wave_cnt, q, tile_total) + mbcnt64(mask[q]);
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
	}
	if (!WRITE) {
		kept = block_sum_of_waves(kept, red);
		if (tid == 0)
			g.block_counts[blockIdx.x] = (int32_t)kept;
	}
}

}  // namespace

extern "C" size_t acm_segment_workspace_bytes(size_t max_records)
{
	return block_counts_bytes(grid_for(max_records));
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
	g.cap = clamp_cap(out_capacity);
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
