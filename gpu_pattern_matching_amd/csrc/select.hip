// Leftmost-longest non-overlapping selection over the records of a pass.  gfx950 only.  DESIGN.md 6o.
//
// An entry (p, o) of pattern p (length L, wildcard context pre and post, both 0 without one) spans
// [s, e] = [o - L + 1 - pre, o + post], int64.  It is ELIGIBLE iff p is a pattern index, L >= 1 and s >= min_start.
// The rule (include/acmatch.h): cursor c = min_start; among the eligible entries with s >= c the smallest s, then
// the largest e, then the first in the input; emit it, c = e + 1, repeat.
//
// Ordered stably by s, the entries that begin at one byte are a contiguous RUN, still in input order, and "the entry
// chosen behind entry j" is a function of j alone: the best of the first run whose s is > e_j.  The chosen set is
// the path from the best of the first run through that function, and pointer doubling marks a path in a number of
// rounds that depends on the cell count alone.  Launches, on the record-pass grid (record_pass.h) over
// n = max_records cells:
//   k_sel_key            per cell: key s - min_start (or all-ones: not eligible, or behind the count), its index,
//                        mark[] = 0; per block the entries dropped for s < min_start
//   k_radix_hist / k_radix_offsets / k_radix_scatter   (radix_pass.h) four stable 8-bit passes: the whole key
//   k_sel_runs           the first cell of every run walks it: best[first] = the cell with the largest e, the earliest
//                        among equals; block 0 writes info[0..1]
//   k_sel_double<true>   round 0: succ(j) = best of the run found by a binary search for e_j + 1, computed on the
//                        fly; jump_1[j] = succ(succ(j)); the head and its successor are marked
//   k_sel_double<false>  rounds 1 .. R - 1, R = ceil(log2(n + 1)): a marked cell marks jump_k[j];
//                        jump_{k+1}[j] = jump_k[jump_k[j]], ping-ponged between two buffers
//   k_sel_emit<write>    the core's count and write launches over the input order (emit_flagged): a record per marked cell
// 16 + R launches, whatever the planes hold.  After round k the marks hold the first 2^(k+1) cells of the path and
// never a cell off it, so marking in place is sound: every writer stores the same 1, and a cell that sees a mark of
// its own round only marks a cell further along the path.  2^R >= n + 1 cells cover every path.  No atomics decide
// an order (the LDS atomics of k_radix_hist only count).  Every index that is read from memory is bounded before it
// is used.
#include <hip/hip_runtime.h>

#include "acm_internal.h"
#include "device_dfa.h"
#include "radix_pass.h"
#include "record_pass.h"

namespace {

using namespace acm_rp;

struct SelArgs {
	const int32_t *pat_plane, *off_plane;   // the input: [0] the count, then the records, then the trailer
	uint32_t n;                             // max_records: the cells that are keyed and ordered; cell n is END
	int64_t min_start;
	const uint32_t *pat_len;                // [patterns]
	const int4 *wild_ent;                   // [patterns] {cell index, pre, post, length}; null: a set without contexts
	uint32_t num_patterns;
	// workspace
	uint32_t *key_in, *val_in;              // the cells as keyed; keys/vals: the ordered cells
	const uint32_t *keys, *vals;
	uint32_t *best;                         // [n] in start order, at the first cell of a run: the run's best cell
	const uint32_t *jump_in;                // [n + 1] in start order: the cell 2^k choices on, or n: none
	uint32_t *jump_out;
	uint32_t *mark;                         // [n] by input index: 1: on the path
	int32_t *counts;                        // [gridDim.x] block counts of the emit step
	int32_t *dropped;                       // [gridDim.x] entries with s < min_start
	// output
	int32_t *pat_out, *off_out, *start_out;
	uint32_t cap;
	int32_t *info;
};

__device__ __forceinline__ uint32_t records_of(const SelArgs &g) { return min((uint32_t)g.pat_plane[0], g.n); }

__device__ __forceinline__ Span span_of(const SelArgs &g, uint32_t p, int32_t o)
{
	return acm_rp::span_of(g.pat_len, g.wild_ent, g.num_patterns, p, o);
}

// the span of input cell at < m
__device__ __forceinline__ Span span_at(const SelArgs &g, uint32_t at)
{
	return span_of(g, (uint32_t)g.pat_plane[1 + at], g.off_plane[1 + at]);
}

__global__ __launch_bounds__(kThreads) void k_sel_key(SelArgs g)
{
	__shared__ uint32_t red[kWaves];

	const uint32_t tid = threadIdx.x;
	const uint32_t m = records_of(g);
	const Share sh = share_of((g.n + kTile - 1) / kTile);
	uint32_t drop = 0;
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++)
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t i = t * kTile + q * kThreads + tid;
			if (i >= g.n)
				continue;
			uint32_t key = kNoKey;
			if (i < m) {
				const Span sp = span_at(g, i);
				if (sp.ok) {
					if (sp.s >= g.min_start)
						key = (uint32_t)(sp.s - g.min_start);   // (< kNoKey: s <= INT32_MAX, min_start > INT32_MIN)
					else
						drop++;
				}
			}
			g.key_in[i] = key;
			g.val_in[i] = i;
			g.mark[i] = 0;
		}
	drop = block_sum(drop, red);
	if (tid == 0)
		g.dropped[blockIdx.x] = (int32_t)drop;
}

// the span's end of ordered cell j < E; false where the cell is not what its key says (never: the key came from it)
__device__ __forceinline__ bool end_of(const SelArgs &g, uint32_t j, uint32_t m, int64_t &e)
{
	const uint32_t at = g.vals[j];
	if (at >= m)
		return false;
	const Span sp = span_at(g, at);
	e = sp.e;
	return sp.ok;
}

// ---- the best cell of every run of equal starts ----

__global__ __launch_bounds__(kThreads) void k_sel_runs(SelArgs g)
{
	__shared__ uint32_t red[kWaves];

	const uint32_t tid = threadIdx.x;
	const uint32_t m = records_of(g);
	const uint32_t E = lower_bound_u32(g.keys, g.n, kNoKey);   // the eligible cells
	const Share sh = share_of((g.n + kTile - 1) / kTile);
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++)
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t j = t * kTile + q * kThreads + tid;
			if (j >= g.n)
				continue;
			uint32_t b = j;
			if (j < E) {
				const uint32_t key = g.keys[j];
				if (j == 0 || g.keys[j - 1] != key) {   // the first of its run
					int64_t be = INT64_MIN;
					for (uint32_t k = j; k < E && g.keys[k] == key; k++) {
						int64_t e;
						if (end_of(g, k, m, e) && e > be) {   // (>: the earliest in the input among equals)
							be = e;
							b = k;
						}
					}
				}
			}
			g.best[j] = b;
		}
	if (blockIdx.x == 0) {
		uint32_t d = 0;
		for (uint32_t j = tid; j < gridDim.x; j += kThreads)
			d += (uint32_t)g.dropped[j];
		d = block_sum(d, red);
		if (tid == 0) {
			g.info[0] = (int32_t)E;
			g.info[1] = (int32_t)d;
		}
	}
}

// ---- the path ----

// the cell chosen behind ordered cell j < E, or n: none
__device__ __forceinline__ uint32_t succ(const SelArgs &g, uint32_t j, uint32_t m, uint32_t E)
{
	int64_t e;
	if (!end_of(g, j, m, e))
		return g.n;
	const int64_t t = e + 1 - g.min_start;   // the key of the first start behind the span
	if (t > (int64_t)(kNoKey - 1))
		return g.n;
	const uint32_t r = lower_bound_u32(g.keys, E, (uint32_t)max(t, (int64_t)0));
	if (r >= E)
		return g.n;
	const uint32_t b = g.best[r];
	return b < E ? b : g.n;
}

template <bool FIRST>
__global__ __launch_bounds__(kThreads) void k_sel_double(SelArgs g)
{
	const uint32_t tid = threadIdx.x;
	const uint32_t m = records_of(g);
	const uint32_t END = g.n;
	const uint32_t E = lower_bound_u32(g.keys, g.n, kNoKey);
	uint32_t head = END;
	if (FIRST && E > 0) {
		head = g.best[0];
		if (head >= E)
			head = END;
	}
	if (blockIdx.x == 0 && tid == 0)
		g.jump_out[END] = END;
	const Share sh = share_of((g.n + kTile - 1) / kTile);
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++)
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t j = t * kTile + q * kThreads + tid;
			if (j >= g.n)
				continue;
			uint32_t a = END, b = END;
			if (j < E) {
				a = FIRST ? succ(g, j, m, E) : min(g.jump_in[j], END);
				if (a < E)
					b = FIRST ? succ(g, a, m, E) : min(g.jump_in[a], END);
				else
					a = END;
				const uint32_t at = g.vals[j];
				const bool marked = FIRST ? j == head : (at < g.n && g.mark[at] != 0);
				if (marked) {
					if (FIRST && at < g.n)
						g.mark[at] = 1;
					if (a < E) {
						const uint32_t to = g.vals[a];
						if (to < g.n)
							g.mark[to] = 1;
					}
				}
			}
			g.jump_out[j] = b;
		}
}

// ---- the chosen entries, in input order ----

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void k_sel_emit(SelArgs g)
{
	__shared__ uint32_t wave_cnt[kPer * kWaves];
	__shared__ uint32_t red[2 * kWaves];

	const uint32_t m = records_of(g);
	uint32_t last_key = 0;   // the largest start's key: the entry whose span ends at or behind it is the path's last
	if (WRITE) {
		const uint32_t E = lower_bound_u32(g.keys, g.n, kNoKey);
		last_key = E > 0 ? g.keys[E - 1] : 0;
	}
	// (the capacity is tested in put: the last chosen entry leaves the cursor even where its record does not fit)
	emit_flagged<WRITE>(
	    g.mark, m, g.counts, 0xFFFFFFFFu, wave_cnt, red,
	    [&](uint32_t total) {
		    const int32_t last = g.pat_plane[1 + m];   // the trailer is the input's
		    write_ends(g.pat_out, g.cap, total, last);
		    write_ends(g.off_out, g.cap, total, last);
		    if (g.start_out)
			    write_ends(g.start_out, g.cap, total, 0);
		    if (total == 0) {
			    g.info[2] = (int32_t)(uint32_t)((uint64_t)g.min_start & 0xFFFFFFFFu);
			    g.info[3] = (int32_t)(g.min_start >> 32);
		    }
	    },
	    [&](uint32_t i, uint32_t d) {
		    const int32_t p = g.pat_plane[1 + i], o = g.off_plane[1 + i];
		    const Span sp = span_of(g, (uint32_t)p, o);
		    if ((uint64_t)d + 2 < g.cap) {
			    g.pat_out[1 + d] = p;
			    g.off_out[1 + d] = o;
			    if (g.start_out)
				    g.start_out[1 + d] = (int32_t)sp.s;
		    }
		    if (sp.e + 1 - g.min_start > (int64_t)last_key) {   // no start behind this span: one cell of the path
			    const int64_t c = sp.e + 1;
			    g.info[2] = (int32_t)(uint32_t)((uint64_t)c & 0xFFFFFFFFu);
			    g.info[3] = (int32_t)(c >> 32);
		    }
	    });
}

// ---- host side ----

struct Layout {
	size_t key[2], val[2], best, jump[2], mark, hist, digit_total, counts, dropped, total;
};

Layout layout_of(size_t n, uint32_t blocks)
{
	Layout l;
	size_t at = 0;
	auto take = [&](size_t bytes) {
		const size_t here = at;
		at += round256(bytes);
		return here;
	};
	for (int k = 0; k < 2; k++) {
		l.key[k] = take(n * sizeof(uint32_t));
		l.val[k] = take(n * sizeof(uint32_t));
	}
	l.best = take(n * sizeof(uint32_t));
	for (int k = 0; k < 2; k++)
		l.jump[k] = take((n + 1) * sizeof(uint32_t));
	l.mark = take(n * sizeof(uint32_t));
	l.hist = take(radix_hist_bytes(blocks));
	l.digit_total = take(radix_digit_total_bytes());
	l.counts = take((size_t)blocks * sizeof(int32_t));
	l.dropped = take((size_t)blocks * sizeof(int32_t));
	l.total = std::max<size_t>(at, 256);
	return l;
}

// rounds of doubling that cover a path of n cells and END: ceil(log2(n + 1))
uint32_t rounds_for(size_t n)
{
	uint32_t r = 0;
	while (((size_t)1 << r) < n + 1)
		r++;
	return r;
}

}  // namespace

extern "C" size_t acm_select_workspace_bytes(size_t max_records)
{
	return layout_of(max_records, grid_for(max_records)).total;
}

extern "C" int acm_select_matches_async(const acm_dfa *d, const int32_t *d_pat_plane, const int32_t *d_off_plane,
    size_t max_records, long min_start, unsigned flags, int32_t *d_pat_out, int32_t *d_off_out, int32_t *d_start_out,
    size_t out_capacity, int32_t *d_info, void *d_workspace, size_t workspace_bytes, void *stream)
{
	if (!d || !d_pat_plane || !d_off_plane || !d_pat_out || !d_off_out || !d_info || out_capacity < 2 ||
	    max_records > 0x7FFFFFFEul || flags != 0 || min_start < (long)INT32_MIN + 1 || min_start > (long)INT32_MAX)
		return acm::fail(ACM_ERR_ARG, "acm_select_matches_async: bad arguments");
	if ((d->num_patterns && !d->d_pat_len) || (d->wild && !d->d_wild_ent))
		return acm::fail(ACM_ERR_ARG, "acm_select_matches_async: automaton without its span tables");
	const uint32_t blocks = grid_for(max_records);
	const Layout l = layout_of(max_records, blocks);
	if (!d_workspace || workspace_bytes < l.total)
		return acm::fail(ACM_ERR_ARG, "acm_select_matches_async: workspace %zu B < required %zu B", workspace_bytes, l.total);

	char *ws = (char *)d_workspace;
	SelArgs g{};
	g.pat_plane = d_pat_plane;
	g.off_plane = d_off_plane;
	g.n = (uint32_t)max_records;
	g.min_start = (int64_t)min_start;
	g.pat_len = d->d_pat_len;
	g.wild_ent = d->wild ? (const int4 *)d->d_wild_ent : nullptr;
	g.num_patterns = d->num_patterns;
	g.best = (uint32_t *)(ws + l.best);
	g.mark = (uint32_t *)(ws + l.mark);
	g.counts = (int32_t *)(ws + l.counts);
	g.dropped = (int32_t *)(ws + l.dropped);
	g.pat_out = d_pat_out;
	g.off_out = d_off_out;
	g.start_out = d_start_out;
	g.cap = clamp_cap(out_capacity);
	g.info = d_info;

	ACM_HIP_TRY(hipSetDevice(d->device));
	hipStream_t s = (hipStream_t)stream;
	const dim3 grid(blocks), block(kThreads);
	uint32_t *const key[2] = { (uint32_t *)(ws + l.key[0]), (uint32_t *)(ws + l.key[1]) };
	uint32_t *const val[2] = { (uint32_t *)(ws + l.val[0]), (uint32_t *)(ws + l.val[1]) };
	uint32_t *const jump[2] = { (uint32_t *)(ws + l.jump[0]), (uint32_t *)(ws + l.jump[1]) };
	g.key_in = key[0];
	g.val_in = val[0];
	hipLaunchKernelGGL(k_sel_key, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	int cur = 0;   // the buffers that hold the ordered cells
	ACM_HIP_TRY(radix_order(g.n, key, val, (uint32_t *)(ws + l.hist), (uint32_t *)(ws + l.digit_total), 4, blocks, s, cur));
	g.keys = (const uint32_t *)(ws + l.key[cur]);
	g.vals = (const uint32_t *)(ws + l.val[cur]);
	hipLaunchKernelGGL(k_sel_runs, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	const uint32_t rounds = rounds_for(max_records);
	for (uint32_t k = 0; k < rounds; k++) {
		g.jump_in = jump[k & 1];   // (round 0 reads none)
		g.jump_out = jump[(k & 1) ^ 1];
		if (k == 0)
			hipLaunchKernelGGL(k_sel_double<true>, grid, block, 0, s, g);
		else
			hipLaunchKernelGGL(k_sel_double<false>, grid, block, 0, s, g);
		ACM_HIP_TRY(hipGetLastError());
	}
	hipLaunchKernelGGL(k_sel_emit<false>, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_sel_emit<true>, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}
