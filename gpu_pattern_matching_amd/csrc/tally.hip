// Match tallies: counts per class and per (segment, class) of the records of any pass.  gfx950 only.
//
// A counted entry is a record's pattern (HEAD planes), the head of a record's match list (STATE planes)
// or every entry of that list (ACM_TALLY_ALL_PATTERNS).  Its class is class_of[pattern] (the pattern
// itself without a map), its segment the last start <= its offset.  Sums are integers and a tally keeps
// no order, so one launch over the records does it (segment.hip and word.hip need two: count, write):
//   k_tally   the fixed grid of record_pass.h, every block owns a contiguous run of 1024-record tiles
// in front of it hipMemsetAsync zeroes the outputs that are written whole; everything the kernel adds to
// global memory is an atomic add, so blocks and tiles need no order among themselves.
//
// Class totals: num_classes <= kLdsClasses: one uint32 bin per class in LDS per block (ds atomics), one
// 64-bit global atomic per non-zero bin when the block is done.  Above that: a global atomic per entry,
// lanes of a wave that share a class merged into one add first.
// Segment rows: the slice of the start array a tile spans is found and staged (record_pass.h); the
// rows a tile touches are contiguous (records and starts are both in offset order), so when rows x
// classes <= kRowCells they are summed in LDS and added to global memory once per tile (rows at a tile's
// edges are shared with its neighbours: atomics only).  Otherwise a global atomic per entry, merged per
// (row, class) inside a wave.
//
// LDS budget: 160 KiB per CU over the 4 blocks of 256 threads a CU gets from the largest grid (1024
// blocks, 256 CUs) = 40 KiB per block: 8 KiB slice + 8 KiB rows + 22 KiB bins (5632 classes) + 8 B.
//
// Every class, pattern index, state and segment is range-checked before it addresses anything: no write
// leaves the output arrays whatever the planes and the class map hold.
#include <hip/hip_runtime.h>

#include "acm_internal.h"
#include "device_dfa.h"
#include "record_pass.h"

namespace {

using namespace acm_rp;

constexpr uint32_t kRowCells = 2048;         // (segment, class) cells of a tile summed in LDS (8 KiB)
constexpr uint32_t kLdsClasses = 5632;       // class bins per block in LDS (22 KiB)
constexpr size_t kWorkspace = 256;           // the pass needs no scratch; the query keeps its siblings' shape

struct TallyArgs {
	const int32_t *pat_plane, *off_plane;
	uint32_t max_records;
	int report, all;
	const int32_t *class_of;     // [num_patterns] or null: the identity
	uint32_t num_classes, num_patterns, num_states;
	const uint32_t *list_begin, *list_len;
	const int32_t *list_pool;
	const int32_t *seg_start;
	uint32_t segments;
	unsigned long long *class_total;
	int32_t *seg_class, *lead;
	uint32_t flush_tiles;        // tiles a block may sum into its uint32 bins before it must flush them
};

// One add per distinct key among the active lanes of the wave: the first lane that holds a key adds the
// number of lanes that hold it.  Called by every lane of the wave (active or not).
template <typename F>
__device__ __forceinline__ void wave_merged_add(bool active, int64_t key, F add)
{
	uint64_t todo = __ballot(active);
	const uint32_t lane = lane_id();
	while (todo) {
		const int leader = __ffsll((long long)todo) - 1;
		const uint32_t klo = (uint32_t)__shfl((int)(uint32_t)key, leader, 64);
		const uint32_t khi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)key >> 32), leader, 64);
		const bool same = active && (uint32_t)key == klo && (uint32_t)((uint64_t)key >> 32) == khi;
		const uint64_t group = __ballot(same);
		if (lane == (uint32_t)leader)
			add((uint32_t)__popcll(group));
		todo &= ~group;
	}
}

__global__ __launch_bounds__(kThreads) void k_tally(TallyArgs g)
{
	__shared__ int32_t slice[kSliceMax];
	__shared__ uint32_t rows[kRowCells];
	__shared__ uint32_t bins[kLdsClasses];
	__shared__ uint32_t bounds[2];

	const uint32_t tid = threadIdx.x;
	const uint32_t m = min((uint32_t)g.pat_plane[0], g.max_records);
	const Share sh = share_of((m + kTile - 1) / kTile);
	if (sh.t_begin == sh.t_end)   // a batch with few records: most of the grid has nothing to do
		return;
	const uint32_t C = g.num_classes;
	const bool lds_bins = C <= kLdsClasses;
	const bool want_rows = g.segments && (g.seg_class || g.lead);
	if (lds_bins) {
		for (uint32_t j = tid; j < C; j += kThreads)
			bins[j] = 0;
		__syncthreads();
	}
	auto flush_bins = [&]() {   // between two barriers
		for (uint32_t j = tid; j < C; j += kThreads) {
			const uint32_t v = bins[j];
			if (v) {
				atomicAdd(&g.class_total[j], (unsigned long long)v);
				bins[j] = 0;
			}
		}
	};

	uint32_t since_flush = 0;
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++) {
		const uint32_t r0 = t * kTile, r1 = min(r0 + kTile, m);
		int32_t off[kPer];
		uint32_t cell[kPer];
#pragma unroll
		for (int q = 0; q < kPer; q++) {   // loaded first: in flight while the slice is found and staged
			const uint32_t i = r0 + q * kThreads + tid;
			off[q] = i < r1 ? g.off_plane[1 + i] : 0;
			cell[q] = i < r1 ? (uint32_t)g.pat_plane[1 + i] : 0;
		}
		Slice st{};
		uint32_t n_rows = 0, row_cells = 0;
		int32_t k_first = 0;
		bool rows_in_lds = false;
		if (want_rows) {
			// (behind stage_slice's first barrier the rows of the previous tile are no longer read either)
			st = stage_slice(g.off_plane, r0, r1, g.seg_start, g.segments, slice, bounds);
			// rows k_first .. st.ub1 - 1 (row -1: the lead)
			k_first = (int32_t)st.ub0 - 1;
			if (st.ub1 >= st.ub0) {
				n_rows = st.ub1 - st.ub0 + 1;
				rows_in_lds = (uint64_t)n_rows * C <= kRowCells;
			}
			row_cells = rows_in_lds ? n_rows * C : 0;
			for (uint32_t j = tid; j < row_cells; j += kThreads)
				rows[j] = 0;
			__syncthreads();
		}
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t i = r0 + q * kThreads + tid;
			// the entries of this record: pool[begin .. begin + cnt), or the one pattern `single`
			uint32_t begin = 0, cnt = 0;
			int32_t single = -1;
			if (i < r1) {
				if (g.report == ACM_REPORT_HEAD) {
					if (cell[q] < g.num_patterns) {
						single = (int32_t)cell[q];
						cnt = 1;
					}
				} else if (cell[q] < g.num_states) {
					const uint32_t n = g.list_len[cell[q]];
					begin = g.list_begin[cell[q]];
					cnt = g.all ? n : min(n, 1u);
				}
			}
			int32_t k = -1;
			if (want_rows && cnt)   // in [-1, segments - 1] whatever the offset is
				k = (int32_t)starts_le(st, slice, g.seg_start, g.segments, off[q]) - 1;
			for (uint32_t j = 0; __ballot(j < cnt); j++) {
				bool ok = j < cnt;
				uint32_t cls = 0;
				if (ok) {
					const uint32_t p = single >= 0 ? (uint32_t)single : (uint32_t)g.list_pool[begin + j];
					ok = p < g.num_patterns;
					if (ok)
						cls = g.class_of ? (uint32_t)g.class_of[p] : p;
					ok = ok && cls < C;
				}
				if (lds_bins) {
					if (ok)
						atomicAdd(&bins[cls], 1u);
				} else {
					wave_merged_add(ok, (int64_t)cls,
					    [&](uint32_t n) { atomicAdd(&g.class_total[cls], (unsigned long long)n); });
				}
				if (!want_rows)
					continue;
				const uint32_t r = (uint32_t)(k - k_first);
				const bool here = ok && rows_in_lds && r < n_rows;
				if (here)
					atomicAdd(&rows[r * C + cls], 1u);
				// what LDS does not hold: a tile that spans too many rows.  (Planes that are not in offset
				// order are outside the contract: such a record may fall outside the rows its tile's ends
				// name, or below the staged slice, where it is attributed to row k0 - 1; the add stays inside
				// the arrays either way.)
				const bool far = ok && !here && (k >= 0 ? g.seg_class != nullptr : g.lead != nullptr);
				if (rows_in_lds) {
					if (far)
						atomicAdd(k >= 0 ? &g.seg_class[(size_t)k * C + cls] : &g.lead[cls], 1);
				} else {
					wave_merged_add(far, (int64_t)k * (int64_t)C + (int64_t)cls, [&](uint32_t n) {
						atomicAdd(k >= 0 ? &g.seg_class[(size_t)k * C + cls] : &g.lead[cls], (int32_t)n);
					});
				}
			}
		}
		if (row_cells) {
			__syncthreads();
			for (uint32_t j = tid; j < row_cells; j += kThreads) {
				const uint32_t v = rows[j];
				if (!v)
					continue;
				const int32_t k = k_first + (int32_t)(j / C);
				const uint32_t cls = j % C;
				if (k >= 0) {
					if (g.seg_class)
						atomicAdd(&g.seg_class[(size_t)k * C + cls], (int32_t)v);
				} else if (g.lead) {
					atomicAdd(&g.lead[cls], (int32_t)v);
				}
			}
		}
		if (lds_bins && ++since_flush >= g.flush_tiles && t + 1 < sh.t_end) {   // (uniform over the block)
			__syncthreads();
			flush_bins();
			__syncthreads();
			since_flush = 0;
		}
	}
	if (lds_bins) {
		__syncthreads();
		flush_bins();
	}
}

}  // namespace

extern "C" size_t acm_tally_workspace_bytes(size_t max_records, size_t num_classes)
{
	(void)max_records;
	(void)num_classes;
	return kWorkspace;
}

extern "C" int acm_tally_matches_async(const acm_dfa *d, const int32_t *d_pat_plane, const int32_t *d_off_plane,
    size_t max_records, int report, int flags, const int32_t *d_class_of, size_t num_classes,
    const int32_t *d_seg_start, size_t segments, uint64_t *d_class_total, int32_t *d_seg_class, int32_t *d_lead,
    void *d_workspace, size_t workspace_bytes, void *stream)
{
	const bool all = (flags & ACM_TALLY_ALL_PATTERNS) != 0;
	if (!d || !d_pat_plane || !d_off_plane || !d_class_total || max_records > 0x7FFFFFFEul ||
	    (report != ACM_REPORT_HEAD && report != ACM_REPORT_STATE) ||
	    (flags & ~(ACM_TALLY_ACCUMULATE | ACM_TALLY_ALL_PATTERNS)) || (all && report == ACM_REPORT_HEAD) ||
	    num_classes == 0 || num_classes > 0x7FFFFFFFul || (segments && !d_seg_start) || segments > 0x7FFFFFFFul ||
	    (d_seg_class && !segments))
		return acm::fail(ACM_ERR_ARG, "acm_tally_matches_async: bad arguments");
	if (!d_class_of && num_classes != d->num_patterns)
		return acm::fail(ACM_ERR_ARG, "acm_tally_matches_async: no class map and num_classes %zu != %u patterns",
		    num_classes, d->num_patterns);
	if (report == ACM_REPORT_STATE && (!d->d_list_begin || !d->d_list_len || !d->d_list_pool))
		return acm::fail(ACM_ERR_ARG, "acm_tally_matches_async: automaton has no match lists");
	if (d_seg_class && (uint64_t)segments * (uint64_t)num_classes > 0x7FFFFFFFull)
		return acm::fail(ACM_ERR_LIMIT, "acm_tally_matches_async: %zu segments x %zu classes exceed 2^31 - 1 cells",
		    segments, num_classes);
	if (!d_workspace || workspace_bytes < acm_tally_workspace_bytes(max_records, num_classes))
		return acm::fail(ACM_ERR_ARG, "acm_tally_matches_async: workspace %zu B < required %zu B", workspace_bytes,
		    acm_tally_workspace_bytes(max_records, num_classes));
	hipStream_t s = (hipStream_t)stream;
	ACM_HIP_TRY(hipSetDevice(d->device));
	TallyArgs g;
	g.pat_plane = d_pat_plane;
	g.off_plane = d_off_plane;
	g.max_records = (uint32_t)max_records;
	g.report = report;
	g.all = all ? 1 : 0;
	g.class_of = d_class_of;
	g.num_classes = (uint32_t)num_classes;
	g.num_patterns = d->num_patterns;
	g.num_states = d->num_states;
	g.list_begin = d->d_list_begin;
	g.list_len = d->d_list_len;
	g.list_pool = d->d_list_pool;
	g.seg_start = d_seg_start;
	g.segments = (uint32_t)segments;
	g.class_total = (unsigned long long *)d_class_total;
	g.seg_class = d_seg_class;
	g.lead = d_lead;
	// a record adds at most one entry per pattern: a block's uint32 bins cannot wrap within this many tiles
	const uint64_t per_tile = (uint64_t)kTile * (all ? std::max<uint32_t>(d->num_patterns, 1) : 1);
	g.flush_tiles = (uint32_t)std::max<uint64_t>(1, 0x7FFFFFFFull / per_tile);
	if (!(flags & ACM_TALLY_ACCUMULATE))
		ACM_HIP_TRY(hipMemsetAsync(d_class_total, 0, num_classes * sizeof(uint64_t), s));
	if (d_seg_class)
		ACM_HIP_TRY(hipMemsetAsync(d_seg_class, 0, segments * num_classes * sizeof(int32_t), s));
	if (d_lead)
		ACM_HIP_TRY(hipMemsetAsync(d_lead, 0, num_classes * sizeof(int32_t), s));
	hipLaunchKernelGGL(k_tally, dim3(grid_for(max_records)), dim3(kThreads), 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}
