// Approximate patterns: up to k substituted bytes per pattern, counted where a piece matched.  gfx950 only.
//
// An approximate pattern (acm_automaton_add_approx) of n bytes and budget k is in the automaton as k + 1 pieces
// that tile it: piece i covers [b_i, b_{i + 1}), b_i = i * q + min(i, r) with q = n / (k + 1), r = n % (k + 1).
// An occurrence with at most k mismatches holds at least one piece exactly (pigeonhole), so the records of the
// pieces are its candidates and this pass makes them matches.  Entry (p, o) with L >= 1 in the text [T0, Tend)
// its record lies in (int64 throughout):
//   1. p is no piece: kept, distance 0
//   2. p is piece j of A: s = o - L + 1 - b_j, span [s, s + n).  The span leaves [T0, Tend): dropped
//   3. the span leaves the bytes given, [text_origin - before_len, text_end): undecided, dropped and counted
//   4. m_i = mismatches of piece i with the text under it (both sides folded if A folds): kept iff m_j == 0,
//      m_i > 0 for every i < j and sum m_i <= k
// Rule 4 reports an occurrence once, by its first exact piece, and stands on the text alone: no sort, no case
// pass in front, and a cell that names a piece where none matched is dropped.
//
// Tables (device_dfa.hip, only for a set with approximate patterns): d_approx_ent[p] = {word index of A's bytes
// in d_approx_pool or -1, n, k | j << 8 | folds << 16, mode}, one 16-byte load per entry (mode 1: an edit pattern,
// which only edit.hip verifies: this pass refuses a set that holds one); d_approx_pool, the whole
// patterns (stored folded for one that folds), each from a word on, one spare word behind the last.  A set
// without them has neither: the pass then reads d_pat_len, keeps every entry of length >= 1 with distance 0 and
// looks up no text.
//
// The compare walks the span from its first byte: bytes in `before` and up to the first aligned text word, then
// aligned text words against the pool at a byte shift (two pool words and v_alignbyte, as case.hip), then the
// last bytes.  A word's mismatches are the popcount of the per-byte "any bit" mask of the XOR; the mask is cut
// where a piece ends.  A lane leaves as soon as the sum passes k, a piece in front of j closes without a
// mismatch or piece j closes with one: on random data within a few words, so the lanes of a wave that loop on
// are few and the divergence is short.
//
// The pass is an entry filter (entry_pass.h): k_approx<false> counts the cells and the
// undecided entries of every block, k_approx<true> writes the three planes; two launches.
#include <hip/hip_runtime.h>

#include "approx_verdict.h"
#include "case_fold.h"
#include "entry_pass.h"

namespace {

using namespace acm_rp;

struct ApproxArgs {
	EntryArgs e;                 // all: set.  block_counts: [2][gridDim.x]: cells written, undecided entries
	int states;                  // the cells are states (ACM_REPORT_STATE), else pattern indices
	TextWindow w;                // (tail_out: null)
	const int32_t *seg_start;
	uint32_t segments;
	int64_t lead_begin, open_end;   // open_end: kEndUnknown when the caller passed -1
	const int4 *ent;             // null: the set has no approximate pattern, every entry of length >= 1 is kept
	const uint32_t *pool;
	int32_t *dist_out;           // null: no distance plane
	int32_t *info;               // [4]
};

struct ApproxPass : EntryPass {
	const ApproxArgs &g;
	int32_t *slice;     // kSliceMax cells of LDS
	uint32_t *bounds;   // 2 cells of LDS
	Slice st{};         // the starts the tile spans
	uint32_t r1 = 0;    // the end of the tile's records
	uint32_t und = 0;   // undecided entries this thread dropped
	struct Row {
		int64_t T0, Tend;   // the text of the record (Tend: kEndUnknown)
		uint32_t kept;      // bit j: entry j of the record's list is kept (j < 32)
		uint32_t dist;      // the distance of the record's first kept entry
	};

	__device__ __forceinline__ ApproxPass(const ApproxArgs &g, int32_t *slice, uint32_t *bounds) : g(g), slice(slice), bounds(bounds) {}
	__device__ __forceinline__ bool head_form() const { return false; }   // (record<true> writes: the distance plane is its own)
	__device__ __forceinline__ bool want_text() const { return g.ent && g.segments; }   // (without pieces no entry asks)

	__device__ __forceinline__ void tile(uint32_t r0, uint32_t r1)
	{
		this->r1 = r1;
		if (want_text()) {
			st = stage_slice(g.e.off_plane, r0, r1, g.seg_start, g.segments, slice, bounds);
			__syncthreads();
		}
	}

	__device__ __forceinline__ void put(uint32_t d, int32_t p, int32_t o, uint32_t dist) const
	{
		emit(g.e, d, p, o);
		if (g.dist_out && d + 2 < g.e.cap)
			g.dist_out[1 + d] = (int32_t)dist;
	}

	// !WRITE: finds the record's text and adds its undecided entries to und
	template <bool WRITE>
	__device__ __forceinline__ uint32_t record(Row &row, uint32_t i, int32_t o, uint32_t c, uint32_t d, int32_t &)
	{
		if (!WRITE) {
			row = Row{ g.lead_begin, g.open_end, 0, 0 };
			if (i >= r1)   // (no record: no search for its text)
				return 0;
			if (want_text()) {
				int64_t next = INT64_MAX;
				// start number k, from the staged slice where it holds it
				text_bounds(starts_le(st, slice, g.seg_start, g.segments, o), g.segments, [&](uint32_t k) -> int64_t {
					return (st.in_lds && k >= st.k0 && k - st.k0 < st.len) ? slice[k - st.k0] : g.seg_start[k];
				}, row.T0, next);
				if (next <= g.w.text_end)
					row.Tend = next;
			}
		}
		if (!g.states) {   // a pattern cell: one entry
			if (WRITE) {   // (called for a kept entry only)
				put(d, (int32_t)c, o, row.dist);
				return 1;
			}
			const int v = verdict(g, c, o, row.T0, row.Tend, row.dist);
			und += v == kUndecided;
			return v == kKeep;
		}
		// the write walk asks about the same entries as the count walk in front of it: it takes the first 32
		// answers, and the first kept entry's distance, from the row
		const uint32_t len = list_len_of(g.e, c);
		if (len == 0)
			return 0;
		const uint32_t from = g.e.list_begin[c];
		uint32_t n = 0;
		for (uint32_t j = 0; j < len; j++) {
			const int32_t p = g.e.list_pool[from + j];
			if ((uint32_t)p >= g.e.num_patterns)
				continue;
			const uint32_t bit = j < 32 ? 1u << j : 0u;
			uint32_t dist;
			if (WRITE) {
				if (bit && !(row.kept & bit))
					continue;
				if (bit && (n == 0 || !g.dist_out))
					dist = row.dist;
				else if (verdict(g, (uint32_t)p, o, row.T0, row.Tend, dist) != kKeep)
					continue;
				put(d + n, p, o, dist);
			} else {
				const int v = verdict(g, (uint32_t)p, o, row.T0, row.Tend, dist);
				und += v == kUndecided;
				if (v != kKeep)
					continue;
				row.kept |= bit;
				if (n == 0)
					row.dist = dist;
			}
			n++;
		}
		return n;
	}

	__device__ __forceinline__ void block0(uint32_t *red)
	{
		uint32_t u = 0, total = 0;
		for (uint32_t j = threadIdx.x; j < gridDim.x; j += kThreads) {
			total += (uint32_t)g.e.block_counts[j];
			u += (uint32_t)g.e.block_counts[gridDim.x + j];
		}
		u = block_sum(u, red);
		total = block_sum(total, red);
		if (threadIdx.x == 0) {
			g.info[0] = (int32_t)u;
			g.info[1] = g.info[2] = g.info[3] = 0;
			if (g.dist_out) {   // header and trailer as in the other planes
				const uint32_t m = min((uint32_t)g.e.cell_plane[0], g.e.max_records);
				write_ends(g.dist_out, g.e.cap, total, g.e.cell_plane[1 + m]);
			}
		}
	}
	__device__ __forceinline__ void counted(uint32_t *red)
	{
		und = block_sum(und, red);
		if (threadIdx.x == 0)
			g.e.block_counts[gridDim.x + blockIdx.x] = (int32_t)und;
	}
};

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void k_approx(ApproxArgs g)
{
	__shared__ int32_t slice[kSliceMax];
	__shared__ uint32_t bounds[2];
	__shared__ uint32_t wave_cnt[kPer * kWaves];
	__shared__ uint32_t red[2 * kWaves];

	ApproxPass pass(g, slice, bounds);
	entry_pass<WRITE>(g.e, pass, wave_cnt, red);
}

}  // namespace

extern "C" size_t acm_approx_workspace_bytes(size_t max_records)
{
	return round256(2 * (size_t)grid_for(max_records) * sizeof(int32_t));
}

extern "C" int acm_approx_matches_async(const acm_dfa *d, const int32_t *d_pat_plane, const int32_t *d_off_plane,
    size_t max_records, int report, const void *d_text, long text_origin, long text_end, const void *d_before,
    size_t before_len, const int32_t *d_seg_start, size_t segments, long lead_begin, long open_end, int32_t *d_pat_out,
    int32_t *d_off_out, int32_t *d_dist_out, size_t out_capacity, int32_t *d_info, void *d_workspace, size_t workspace_bytes,
    void *stream)
{
	ApproxArgs g;
	const bool own_ok = d_info && (report == ACM_REPORT_STATE || report == ACM_REPORT_HEAD) &&
	                    window_ok(d_text, text_origin, text_end, d_before, before_len) && (!segments || d_seg_start) &&
	                    segments <= 0x7FFFFFFFul && (open_end == -1 || open_end >= text_end);
	const char *tables = tables_error(d, [&](const acm_dfa &a) -> const char * {
		if (report == ACM_REPORT_STATE && (!a.d_list_begin || !a.d_list_len || !a.d_list_pool))
			return "automaton has no match lists";
		return a.approx && (!a.d_approx_ent || !a.d_approx_pool) ? "automaton with approximate patterns without their tables" : nullptr;
	});
	if (int rc = entry_args(g.e, "acm_approx_matches_async",
	        EntryCall{ d, d_pat_plane, d_off_plane, max_records, 1, d_pat_out, d_off_out, out_capacity, d_workspace, workspace_bytes },
	        own_ok, tables, acm_approx_workspace_bytes(max_records)))
		return rc;
	if (d->edit)
		return acm::fail(ACM_ERR_ARG, "acm_approx_matches_async: the set holds edit patterns, which acm_edit_matches_async verifies");
	g.states = report == ACM_REPORT_STATE;
	g.w = window_of(d, d_text, text_origin, text_end, d_before, before_len, nullptr);
	g.seg_start = d_seg_start;
	g.segments = (uint32_t)segments;
	g.lead_begin = (int64_t)lead_begin;
	g.open_end = open_end == -1 ? kEndUnknown : (int64_t)open_end;
	g.ent = d->approx ? (const int4 *)d->d_approx_ent : nullptr;
	g.pool = d->d_approx_pool;
	g.dist_out = d_dist_out;
	g.info = d_info;
	return launch_passes(k_approx<false>, k_approx<true>, d, max_records, g, stream);
}
