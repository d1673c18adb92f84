// Ordered multi-part signatures: the gap-constrained join of the parts' records.  gfx950 only.
//
// A sequence (acm_automaton_add_sequence, include/acmatch.h) is parts p_0 .. p_{k-1} with a gap (lo, hi) in
// front of every part but the first.  The rule, level by level: a record of pattern p (length L) at offset e
// starts at a = e - L + 1 and lies in the text that begins at T0.  A level-0 record is ALIVE iff a >= T0; a
// level-j record is alive iff some alive level-(j-1) record of its sequence ends in
// [max(a - 1 - hi, T0), a - 1 - lo] (hi unbounded: [T0, a - 1 - lo]).  An alive record of a last part is a
// match.  int64 throughout.  Not here: parts in different calls, overlapping parts, where a match begins.
//
// Tables (device_dfa.hip, only for a set with sequences): a SLOT is a part of a sequence, numbered level-major
// (all level-0 parts, then all level-1 parts, ...).  d_seq_ent[p] = {slot or -1, lo, hi, length}, one 16-byte
// load; d_seq_slot[s] = {slot in front or -1, sequence or -1: not a last part}.
//
// The input is pattern-form planes in offset order.  Ordered stably by slot, the records of every slot are a
// contiguous list still in offset order, and every level a contiguous range.  "Some alive record of the slot in
// front ends in [x, y]" is then two binary searches in that slot's ends and a difference of the level's
// inclusive alive-prefix.  Launches, on the record-pass grid (record_pass.h) over n = max_records cells:
//   k_seq_key            per cell: sort key (slot, or all-ones: no part, or behind the count), its index, T0
//                        (the tile's starts staged in LDS, as the position pass) and emit[] = 0
//   k_radix_hist / k_radix_offsets / k_radix_scatter   (radix_pass.h, shared with rule.hip)
//                        one stable LSD radix pass of 8 bits: per-block digit counts, their exclusive scan in
//                        (digit, block) order (a block per digit over the blocks' counts; the scatter adds the
//                        digits in front), the scatter with ranks from wave ballots.  1 to 4 passes:
//                        ceil(bits(slots) / 8); the all-ones key has the last digit in every pass
//   k_seq_bounds         slot_begin[s] by binary search in the ordered keys; the ends gathered in order
//   k_seq_level<first>   per level: the alive flag of the level's range, a block count, emit[index] = 1 for an
//                        alive record of a last part
//   k_seq_prefix         per level: blocks_before, then the flags become the level's inclusive alive-prefix
//   k_seq_emit<write>    the core's count and write launches over the input order (emit_flagged, radix_pass.h): a
//                        record per emit[] cell set
// 4 + 3 * passes + 2 * levels launches, whatever the planes hold.  No atomics decide an order (the LDS atomics of
// k_radix_hist only count).  Every index that is read from memory is bounded before it is used.
#include <hip/hip_runtime.h>

#include "acm_internal.h"
#include "device_dfa.h"
#include "radix_pass.h"
#include "record_pass.h"

namespace {

using namespace acm_rp;

constexpr uint32_t kNoSlot = kNoKey;

struct SeqArgs {
	const int32_t *pat_plane, *off_plane;   // the input: [0] the count, then the records, then the trailer
	uint32_t n;                             // max_records: the cells that are keyed and ordered
	const int32_t *seg_start;
	uint32_t segments;
	int64_t lead_begin;
	const int4 *ent;                        // [patterns] {slot or -1, lo, hi, length}
	const int2 *slot_tab;                   // [slots] {slot in front or -1, sequence or -1}
	uint32_t num_patterns, slots, levels;
	// workspace
	int64_t *t0;                            // [n] by input index: where the record's text begins
	uint32_t *key_in, *val_in;              // the cells as keyed; keys/vals: the ordered cells
	const uint32_t *keys, *vals;
	int32_t *ends;                          // [n] in slot order: the record's offset
	uint32_t *prefix;                       // [n] in slot order: alive flag, then the level's inclusive alive-prefix
	uint32_t *emit;                         // [n] by input index: 1: an alive record of a last part
	uint32_t *slot_begin;                   // [slots + 1] first ordered cell of each slot; [slots]: the cells with a slot
	int32_t *counts;                        // [gridDim.x] block counts of a two-launch step
	uint32_t *level_total;                  // [ACM_SEQ_MAX_PARTS] alive records of each level
	uint32_t level, lv_begin, lv_end, prev_begin;    // the level of this launch: its slots and the first of the level in front
	// output
	int32_t *seq_out, *off_out;
	uint32_t cap;
	int32_t *info;
};

__device__ __forceinline__ uint32_t records_of(const SeqArgs &g) { return min((uint32_t)g.pat_plane[0], g.n); }

__global__ __launch_bounds__(kThreads) void k_seq_key(SeqArgs g)
{
	__shared__ int32_t slice[kSliceMax];
	__shared__ uint32_t bounds[2];

	const uint32_t tid = threadIdx.x;
	const uint32_t m = records_of(g);
	const Share sh = share_of((g.n + kTile - 1) / kTile);
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++) {
		const uint32_t r0 = t * kTile, r1 = min(r0 + kTile, m);   // (r1 <= r0: a tile behind the records)
		const bool want_text = g.segments && r1 > r0;
		Slice st{};
		if (want_text) {
			st = stage_slice(g.off_plane, r0, r1, g.seg_start, g.segments, slice, bounds);
			__syncthreads();
		}
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t i = r0 + q * kThreads + tid;
			if (i >= g.n)
				continue;
			uint32_t key = kNoSlot;
			int64_t T0 = g.lead_begin;
			if (i < r1) {
				const uint32_t p = (uint32_t)g.pat_plane[1 + i];
				const int32_t slot = p < g.num_patterns ? g.ent[p].x : -1;
				if (slot >= 0 && (uint32_t)slot < g.slots) {
					key = (uint32_t)slot;
					if (want_text) {
						const uint32_t ub = starts_le(st, slice, g.seg_start, g.segments, g.off_plane[1 + i]);
						if (ub > 0 && ub <= g.segments) {
							const uint32_t k = ub - 1;
							T0 = (st.in_lds && k >= st.k0 && k - st.k0 < st.len) ? slice[k - st.k0] : g.seg_start[k];
						}
					}
				}
			}
			g.key_in[i] = key;
			g.val_in[i] = i;
			g.t0[i] = T0;
			g.emit[i] = 0;
		}
	}
}

// ---- the ordered cells: where every slot begins, and the ends in order ----

__global__ __launch_bounds__(kThreads) void k_seq_bounds(SeqArgs g)
{
	const uint32_t tid = threadIdx.x;
	for (uint32_t s = blockIdx.x * kThreads + tid; s <= g.slots; s += gridDim.x * kThreads)
		g.slot_begin[s] = lower_bound_u32(g.keys, g.n, s);
	const uint32_t m = records_of(g);
	const Share sh = share_of((g.n + kTile - 1) / kTile);
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++)
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t i = t * kTile + q * kThreads + tid;
			if (i >= g.n)
				continue;
			const uint32_t at = g.vals[i];
			g.ends[i] = (g.keys[i] != kNoSlot && at < m) ? g.off_plane[1 + at] : 0;
		}
}

// ---- a level ----

struct LevelRange {
	uint32_t first, count;   // ordered cells [first, first + count)
};

__device__ __forceinline__ LevelRange level_range(const SeqArgs &g)
{
	const uint32_t a = min(g.slot_begin[g.lv_begin], g.n), b = min(g.slot_begin[g.lv_end], g.n);
	return LevelRange{ a, b > a ? b - a : 0 };
}

template <bool FIRST>
__global__ __launch_bounds__(kThreads) void k_seq_level(SeqArgs g)
{
	__shared__ uint32_t red[kWaves];

	const uint32_t tid = threadIdx.x;
	const uint32_t m = records_of(g);
	const LevelRange lv = level_range(g);
	const uint32_t prev_first = FIRST ? 0 : min(g.slot_begin[g.prev_begin], g.n);
	const Share sh = share_of((lv.count + kTile - 1) / kTile);
	uint32_t alive_n = 0;
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++)
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t r = t * kTile + q * kThreads + tid;
			if (r >= lv.count)
				continue;
			const uint32_t i = lv.first + r;
			const uint32_t at = g.vals[i], slot = g.keys[i];
			bool alive = false;
			const uint32_t p = at < m ? (uint32_t)g.pat_plane[1 + at] : kNoSlot;
			if (p < g.num_patterns && slot >= g.lv_begin && slot < g.lv_end) {   // (always: the key came from this cell)
				const int4 e = g.ent[p];   // {slot, lo, hi, length}
				const int64_t a = (int64_t)g.ends[i] + 1 - (int64_t)e.w;
				const int64_t T0 = g.t0[at];
				const int2 sl = g.slot_tab[slot];   // {slot in front, sequence}
				if (FIRST) {
					alive = a >= T0;
				} else if ((uint32_t)sl.x < g.lv_begin) {   // (always; and >= 0)
					const uint32_t pb = min(g.slot_begin[sl.x], lv.first), pe = min(g.slot_begin[sl.x + 1], lv.first);
					if (pe > pb && pb >= prev_first) {
						const int64_t upper = a - 1 - (int64_t)e.y;
						// (no end lies below INT32_MIN: the clamp keeps lower - 1 in range whatever lead_begin is)
						const int64_t lower = max(e.z == INT32_MAX ? T0 : max(a - 1 - (int64_t)e.z, T0), (int64_t)INT32_MIN);
						const uint32_t x = pb + upper_bound_i32<int64_t>(g.ends + pb, pe - pb, lower - 1);
						const uint32_t y = pb + upper_bound_i32<int64_t>(g.ends + pb, pe - pb, upper);
						if (y > x)   // alive records among the ordered cells [x, y)
							alive = g.prefix[y - 1] - (x > prev_first ? g.prefix[x - 1] : 0u) > 0;
					}
				}
				if (alive && sl.y >= 0)
					g.emit[at] = 1;
			}
			g.prefix[i] = alive;
			alive_n += alive;
		}
	alive_n = block_sum(alive_n, red);
	if (tid == 0)
		g.counts[blockIdx.x] = (int32_t)alive_n;
}

__global__ __launch_bounds__(kThreads) void k_seq_prefix(SeqArgs g)
{
	__shared__ uint32_t wave_cnt[kPer * kWaves];
	__shared__ uint32_t red[2 * kWaves];

	const uint32_t tid = threadIdx.x;
	const LevelRange lv = level_range(g);
	const Share sh = share_of((lv.count + kTile - 1) / kTile);
	uint32_t all;
	uint32_t base = blocks_before(g.counts, red, all);
	if (blockIdx.x == 0 && tid == 0)
		g.level_total[g.level] = all;
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++) {
		uint32_t incl[kPer], wave_total[kPer];
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t r = t * kTile + q * kThreads + tid;
			incl[q] = wave_inclusive(r < lv.count ? g.prefix[lv.first + r] : 0u);
			wave_total[q] = (uint32_t)__shfl((int)incl[q], 63, 64);
		}
		tile_publish(wave_total, wave_cnt);
		uint32_t tile_total = 0;
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t r = t * kTile + q * kThreads + tid;
			const uint32_t before = base + tile_row(wave_cnt, q, tile_total);
			if (r < lv.count)
				g.prefix[lv.first + r] = before + incl[q];
		}
		base += tile_total;
	}
}

// ---- the matches, in input order ----

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void k_seq_emit(SeqArgs g)
{
	__shared__ uint32_t wave_cnt[kPer * kWaves];
	__shared__ uint32_t red[2 * kWaves];

	const uint32_t m = records_of(g);
	emit_flagged<WRITE>(
	    g.emit, m, g.counts, g.cap, wave_cnt, red,
	    [&](uint32_t total) {
		    const int32_t last = g.pat_plane[1 + m];   // the trailer is the input's
		    write_ends(g.seq_out, g.cap, total, last);
		    write_ends(g.off_out, g.cap, total, last);
		    uint32_t alive = 0;
		    for (uint32_t j = 0; j < g.levels; j++)
			    alive += g.level_total[j];
		    g.info[0] = (int32_t)g.slot_begin[g.slots];
		    g.info[1] = (int32_t)alive;
		    g.info[2] = g.info[3] = 0;
	    },
	    [&](uint32_t i, uint32_t d) {
		    const uint32_t p = (uint32_t)g.pat_plane[1 + i];
		    int32_t seq = -1;
		    if (p < g.num_patterns) {
			    const int32_t slot = g.ent[p].x;
			    if (slot >= 0 && (uint32_t)slot < g.slots)
				    seq = g.slot_tab[slot].y;
		    }
		    g.seq_out[1 + d] = seq;
		    g.off_out[1 + d] = g.off_plane[1 + i];
	    });
}

// a set without sequences: no record
__global__ void k_seq_none(SeqArgs g)
{
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		const int32_t last = g.pat_plane[1 + records_of(g)];
		write_ends(g.seq_out, g.cap, 0, last);
		write_ends(g.off_out, g.cap, 0, last);
		g.info[0] = g.info[1] = g.info[2] = g.info[3] = 0;
	}
}

// ---- host side ----

struct Layout {
	size_t t0, key[2], val[2], ends, prefix, emit, hist, digit_total, slot_begin, counts, level_total, total;
};

Layout layout_of(size_t n, uint32_t blocks, uint32_t slots)
{
	Layout l;
	size_t at = 0;
	auto take = [&](size_t bytes) {
		const size_t here = at;
		at += round256(bytes);
		return here;
	};
	l.t0 = take(n * sizeof(int64_t));
	for (int k = 0; k < 2; k++) {
		l.key[k] = take(n * sizeof(uint32_t));
		l.val[k] = take(n * sizeof(uint32_t));
	}
	l.ends = take(n * sizeof(int32_t));
	l.prefix = take(n * sizeof(uint32_t));
	l.emit = take(n * sizeof(uint32_t));
	l.hist = take(radix_hist_bytes(blocks));
	l.digit_total = take(radix_digit_total_bytes());
	l.slot_begin = take(((size_t)slots + 1) * sizeof(uint32_t));
	l.counts = take((size_t)blocks * sizeof(int32_t));
	l.level_total = take(ACM_SEQ_MAX_PARTS * sizeof(uint32_t));
	l.total = std::max<size_t>(at, 256);
	return l;
}

}  // namespace

extern "C" size_t acm_sequence_workspace_bytes(const acm_dfa *d, size_t max_records)
{
	return layout_of(max_records, grid_for(max_records), d ? d->seq_slots : 0).total;
}

extern "C" int acm_sequence_matches_async(const acm_dfa *d, const int32_t *d_pat_plane, const int32_t *d_off_plane,
    size_t max_records, const int32_t *d_seg_start, size_t segments, long lead_begin, long text_end, int32_t *d_seq_out,
    int32_t *d_off_out, size_t out_capacity, int32_t *d_info, void *d_workspace, size_t workspace_bytes, void *stream)
{
	(void)text_end;   // (where a text ends does not enter the rule)
	if (!d || !d_pat_plane || !d_off_plane || !d_seq_out || !d_off_out || !d_info || out_capacity < 2 ||
	    max_records > 0x7FFFFFFEul || (segments && !d_seg_start) || segments > 0x7FFFFFFFul)
		return acm::fail(ACM_ERR_ARG, "acm_sequence_matches_async: bad arguments");
	if (d->seq_slots && (!d->d_seq_ent || !d->d_seq_slot || d->seq_levels < 1 || d->seq_levels > ACM_SEQ_MAX_PARTS))
		return acm::fail(ACM_ERR_ARG, "acm_sequence_matches_async: automaton with sequences without their tables");
	const uint32_t blocks = grid_for(max_records);
	const Layout l = layout_of(max_records, blocks, d->seq_slots);
	if (!d_workspace || workspace_bytes < l.total)
		return acm::fail(ACM_ERR_ARG, "acm_sequence_matches_async: workspace %zu B < required %zu B", workspace_bytes, l.total);

	char *ws = (char *)d_workspace;
	SeqArgs g{};
	g.pat_plane = d_pat_plane;
	g.off_plane = d_off_plane;
	g.n = (uint32_t)max_records;
	g.seg_start = d_seg_start;
	g.segments = (uint32_t)segments;
	g.lead_begin = (int64_t)lead_begin;
	g.ent = (const int4 *)d->d_seq_ent;
	g.slot_tab = (const int2 *)d->d_seq_slot;
	g.num_patterns = d->num_patterns;
	g.slots = d->seq_slots;
	g.levels = d->seq_levels;
	g.t0 = (int64_t *)(ws + l.t0);
	g.ends = (int32_t *)(ws + l.ends);
	g.prefix = (uint32_t *)(ws + l.prefix);
	g.emit = (uint32_t *)(ws + l.emit);
	g.slot_begin = (uint32_t *)(ws + l.slot_begin);
	g.counts = (int32_t *)(ws + l.counts);
	g.level_total = (uint32_t *)(ws + l.level_total);
	g.seq_out = d_seq_out;
	g.off_out = d_off_out;
	g.cap = clamp_cap(out_capacity);
	g.info = d_info;

	ACM_HIP_TRY(hipSetDevice(d->device));
	hipStream_t s = (hipStream_t)stream;
	const dim3 grid(blocks), block(kThreads);
	if (!d->seq_slots) {
		hipLaunchKernelGGL(k_seq_none, dim3(1), dim3(64), 0, s, g);
		ACM_HIP_TRY(hipGetLastError());
		return ACM_OK;
	}
	uint32_t *const key[2] = { (uint32_t *)(ws + l.key[0]), (uint32_t *)(ws + l.key[1]) };
	uint32_t *const val[2] = { (uint32_t *)(ws + l.val[0]), (uint32_t *)(ws + l.val[1]) };
	g.key_in = key[0];
	g.val_in = val[0];
	hipLaunchKernelGGL(k_seq_key, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	int cur = 0;   // the buffers that hold the ordered cells
	ACM_HIP_TRY(radix_order(g.n, key, val, (uint32_t *)(ws + l.hist), (uint32_t *)(ws + l.digit_total),
	    radix_passes(d->seq_slots), blocks, s, cur));
	g.keys = (const uint32_t *)(ws + l.key[cur]);
	g.vals = (const uint32_t *)(ws + l.val[cur]);
	hipLaunchKernelGGL(k_seq_bounds, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	for (uint32_t j = 0; j < d->seq_levels; j++) {
		g.level = j;
		g.lv_begin = d->seq_level_base[j];
		g.lv_end = d->seq_level_base[j + 1];
		g.prev_begin = j ? d->seq_level_base[j - 1] : 0;
		if (j == 0)
			hipLaunchKernelGGL(k_seq_level<true>, grid, block, 0, s, g);
		else
			hipLaunchKernelGGL(k_seq_level<false>, grid, block, 0, s, g);
		ACM_HIP_TRY(hipGetLastError());
		hipLaunchKernelGGL(k_seq_prefix, grid, block, 0, s, g);
		ACM_HIP_TRY(hipGetLastError());
	}
	hipLaunchKernelGGL(k_seq_emit<false>, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_seq_emit<true>, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}
