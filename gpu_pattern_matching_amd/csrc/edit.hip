// Edit patterns: up to k substituted, inserted or deleted bytes per pattern, verified where a piece matched.
// gfx950 only.  DESIGN.md 6t.
//
// An edit pattern (acm_automaton_add_edit) of n bytes and budget k <= 4 has the pieces of an approximate pattern
// (approx.hip): an occurrence within edit distance k holds one of the k + 1 pieces exactly, so the records of the
// pieces are its candidates.  The rule is in include/acmatch.h (acm_edit_matches_async); in short, for entry (p, o),
// p piece j of A: s0 = o - L + 1 - b_j, e0 = s0 + n, and among the ends e with |e - e0| <= k the one with the
// smallest D(e) = min over s of ed(A, T[s:e]) (Sellers), then the nearest to e0, then the smaller, is reported with
// the shortest span that has that distance.  The output is a set: ordered by (offset, pattern), equal records once.
//
// Stage 1, the candidates, is an entry filter (entry_pass.h): one lane per entry, k_edit<false> counts, k_edit<true>
// writes (pattern, offset, distance | length << 8) in input order into planes of the workspace.  A plain pattern and
// a Hamming pattern (approx_verdict.h) give their normalised record.  For an edit pattern a lane keeps one BAND of the
// Sellers matrix in registers: cell c of 4k + 1 is diagonal c - 2k, text bytes consumed minus pattern bytes
// consumed.  A path of at most k errors that ends within k of e0 never leaves these diagonals, so the band holds
// min(D, k + 1) exactly.  The band advances one pattern byte a step, all indices fixed at compile time (two
// instantiations: 9 cells for k <= 2, 17 for k <= 4; a band wider than 4k + 1 holds the same values), beside a
// window of the text bytes under it that shifts by one byte a step.  A lane
// leaves at the first step whose band is all > k (Ukkonen); on text that does not match, a few steps.  The length is
// a second run of the same routine from e* backwards, reversed pattern against reversed text, with the start fixed;
// only kept entries get there.  No read leaves [max(T0, s0 - 2k), min(Tend, e0 + k)), which the rule has checked.
//
// Stage 2 orders the candidates by (offset, pattern) with the stable radix passes of radix_pass.h: first by pattern
// (as many 8-bit passes as the pattern count needs), then by offset - (text_origin - before_len) (as many as the bytes
// given need); a cell is a record iff it differs from the cell in front, and emit_flagged writes the records.
// The cells ordered are C = max_records * (longest match list) for STATE input, max_records for HEAD input.
//
// Launches: k_edit<false>, k_edit<true>, k_edit_cells<0> (keys by pattern), 3 per pattern digit, k_edit_cells<1>
// (keys by offset), 3 per offset digit, k_edit_cells<2> (flags), k_edit_emit<false>, k_edit_emit<true>:
// 7 + 3 * (pattern digits + offset digits), whatever the planes hold.  No atomics decide an order.  Every index
// read from memory is bounded before it is used.
#include <hip/hip_runtime.h>

#include "approx_verdict.h"
#include "case_fold.h"
#include "entry_pass.h"
#include "radix_pass.h"

namespace {

using namespace acm_rp;

struct EditArgs {
	EntryArgs e;                 // all: set.  pat_out, off_out, cap: the candidate planes.  block_counts: [2][gridDim.x]
	int states;
	TextWindow w;
	const int32_t *seg_start;
	uint32_t segments;
	int64_t lead_begin, open_end;   // open_end: kEndUnknown when the caller passed -1
	const int4 *ent;             // null: the set has no approximate pattern
	const uint32_t *pool;
	int64_t key_lo;              // text_origin - before_len: offset o has the key o - key_lo
	uint32_t key_range;          // the keys are < key_range
	uint32_t *cand_dl;           // [1 + C] beside the candidate planes: distance | length << 8
	int32_t *info;               // [4]
};

struct Cand {
	int32_t pat, off;
	uint32_t dl;
};

// One band of 2 H + 1 cells over the n pattern bytes at pb.  Cell c of the step behind i pattern bytes has consumed
// u = i + c - H text bytes; it exists iff ulo <= u <= uhi, every other cell holds inf.  fwd: the text runs up from
// `base`, byte u is at base + u - 1, and the start is free (step 0 is all 0); else it runs down from `base`, byte u
// is at base - u, and step 0 holds u.  Byte u is read iff ulo < u <= uhi.  False: the band passed inf everywhere.
template <int H>
__device__ __forceinline__ bool band_run(const TextWindow &w, const uint8_t *pb, int32_t n, bool folds, uint32_t inf, bool fwd,
    int64_t base, int32_t ulo, int32_t uhi, uint32_t (&b)[2 * H + 1])
{
	constexpr int W = 2 * H + 1;
	auto byte_at = [&](int32_t u) -> uint32_t {
		if (u <= ulo || u > uhi)
			return 0x100u;   // (no byte: its cells hold inf or start from one that does)
		const uint32_t t = window_byte(w, fwd ? base + u - 1 : base - u);
		return folds ? acm::fold_byte(t) : t;
	};
	uint32_t t[W];
#pragma unroll
	for (int c = 0; c < W; c++) {
		const int32_t u = c - H;
		t[c] = byte_at(u);
		b[c] = (u < ulo || u > uhi) ? inf : fwd ? 0u : min((uint32_t)u, inf);
	}
	for (int32_t i = 1; i <= n; i++) {
		const uint32_t pc = pb[fwd ? i - 1 : n - i];
#pragma unroll
		for (int c = 0; c + 1 < W; c++)
			t[c] = t[c + 1];
		t[W - 1] = byte_at(i + H);
		uint32_t left = inf, low = inf;
#pragma unroll
		for (int c = 0; c < W; c++) {
			const int32_t u = i + c - H;
			const uint32_t diag = b[c] + (t[c] != pc ? 1u : 0u);
			const uint32_t up = c + 1 < W ? b[c + 1] + 1u : inf;
			uint32_t v = min(min(diag, up), min(left + 1u, inf));
			v = (u < ulo || u > uhi) ? inf : v;
			b[c] = v;
			left = v;
			low = min(low, v);
		}
		if (low >= inf)
			return false;
	}
	return true;
}

// rule 3 for piece j of an edit pattern of budget K <= H / 2: e = {pool word, n, k | j << 8 | folds << 16, 1}.  The
// band has 2 H + 1 cells: at least the 4 K + 1 the rule needs (a wider band holds the same values).
template <int H>
__device__ __forceinline__ int edit_verdict(const EditArgs &g, const int4 e, int32_t o, int64_t T0, int64_t Tend, Cand &c)
{
	const int32_t n = e.y, K = e.z & 0xFF, j = (e.z >> 8) & 0xFF;
	const bool folds = (e.z >> 16) & 1;
	const int32_t q = n / (K + 1), r = n % (K + 1);
	const int32_t bj = j * q + min(j, r), ej = (j + 1) * q + min(j + 1, r);
	const int64_t a = (int64_t)o + 1 - (int64_t)(ej - bj);   // the piece is [a, o + 1)
	if (a < T0 || (Tend != kEndUnknown && (int64_t)o + 1 > Tend))
		return kDrop;
	const int64_t s0 = a - bj, e0 = s0 + n;
	if (Tend == kEndUnknown && e0 + K > g.w.text_end)
		return kUndecided;
	const int64_t lo = max(T0, s0 - 2 * K), hi = Tend == kEndUnknown ? e0 + K : min(Tend, e0 + K);
	if (lo < g.w.text_origin - g.w.before_len || hi > g.w.text_end)
		return kUndecided;
	const uint8_t *pb = (const uint8_t *)(g.pool + e.x);
	const uint32_t inf = (uint32_t)K + 1;
	// run 0, forward: u counts from s0 and the cells are the text positions [lo, hi].  Run 1, backward from the end
	// found: the shortest span with that distance, no longer than n + K and not in front of T0.
	int64_t base = s0;
	int32_t ulo = (int32_t)(lo - s0), uhi = (int32_t)(hi - s0);
	uint32_t best = inf, len = (uint32_t)n;
#pragma nounroll
	for (int run = 0; run < 2; run++) {
		uint32_t b[2 * H + 1];
		if (!band_run<H>(g.w, pb, n, folds, inf, run == 0, base, ulo, uhi, b))
			return kDrop;   // (run 1 never: its band holds the path run 0 found)
		if (run == 0) {
			// the end: the smallest distance, then the nearest to e0, then the smaller
			int32_t delta = 0;
#pragma unroll
			for (int t = 0; t <= H; t++) {
				const int d = (t + 1) / 2 * ((t & 1) ? -1 : 1);   // 0, -1, 1, -2, 2, ..
				const int32_t u = n + d;
				if ((t + 1) / 2 <= K && u > ulo && u <= uhi && b[H + d] < best) {   // (an end lies behind T0)
					best = b[H + d];
					delta = d;
				}
			}
			if (best > (uint32_t)K)
				return kDrop;
			base = e0 + delta;
			ulo = 0;
			uhi = (int32_t)min(base - T0, (int64_t)(n + K));
		} else {
			bool found = false;
#pragma unroll
			for (int d = -H / 2; d <= H / 2; d++) {
				const int32_t u = n + d;
				if (!found && d >= -K && d <= K && u <= uhi && b[H + d] == best) {
					found = true;
					len = (uint32_t)u;
				}
			}
		}
	}
	c.off = (int32_t)(base - 1);
	c.dl = best | len << 8;
	return kKeep;
}

// entry (p, o) in the text [T0, Tend) (Tend: kEndUnknown); c: its candidate where it is kept
__device__ __forceinline__ int candidate(const EditArgs &g, uint32_t p, int32_t o, int64_t T0, int64_t Tend, Cand &c)
{
	if (p >= g.e.num_patterns)   // (a cell of a HEAD plane may hold anything)
		return kDrop;
	const uint32_t L = g.e.pat_len[p];
	if (L == 0)
		return kDrop;
	c = Cand{ (int32_t)p, o, L << 8 };
	int v = kKeep;
	if (g.ent) {
		const int4 e = g.ent[p];   // {pool word, n, k | j << 8 | folds << 16, mode}
		if (e.x >= 0) {
			const int32_t k = e.z & 0xFF, j = (e.z >> 8) & 0xFF;
			c.pat = (int32_t)p - j;
			if (e.w == 0) {   // Hamming: the record of the whole pattern
				uint32_t dist;
				v = verdict(g, p, o, T0, Tend, dist);
				const int32_t q = e.y / (k + 1), r = e.y % (k + 1);
				const int64_t end = (int64_t)o + (e.y - ((j + 1) * q + min(j + 1, r)));
				c.off = (int32_t)end;
				c.dl = dist | (uint32_t)e.y << 8;
			} else {
				if (k <= 2)   // two instantiations of the band: 9 cells for k <= 2, 17 for k <= 4
					v = edit_verdict<4>(g, e, o, T0, Tend, c);
				else if (k <= ACM_EDIT_MAX_K)
					v = edit_verdict<8>(g, e, o, T0, Tend, c);
				else
					v = kDrop;
			}
		}
	}
	if (v != kKeep)
		return v;
	// a record of this text ends inside the bytes given; any other offset (a cell may hold anything) has no key
	const int64_t key = (int64_t)c.off - g.key_lo;
	return key >= 0 && key < (int64_t)g.key_range ? kKeep : kDrop;
}

struct EditPass : EntryPass {
	const EditArgs &g;
	int32_t *slice;     // kSliceMax cells of LDS
	uint32_t *bounds;   // 2 cells of LDS
	Slice st{};         // the starts the tile spans
	uint32_t r1 = 0;    // the end of the tile's records
	uint32_t und = 0;   // undecided entries this thread dropped
	struct Row {
		int64_t T0, Tend;   // the text of the record (Tend: kEndUnknown)
		uint32_t kept;      // bit j: entry j of the record's list is kept (j < 32)
		Cand first;         // the candidate of the record's first kept entry
	};

	__device__ __forceinline__ EditPass(const EditArgs &g, int32_t *slice, uint32_t *bounds) : g(g), slice(slice), bounds(bounds) {}
	__device__ __forceinline__ bool head_form() const { return false; }
	__device__ __forceinline__ bool want_text() const { return g.ent && g.segments; }   // (without pieces no entry asks)

	__device__ __forceinline__ void tile(uint32_t r0, uint32_t r1)
	{
		this->r1 = r1;
		if (want_text()) {
			st = stage_slice(g.e.off_plane, r0, r1, g.seg_start, g.segments, slice, bounds);
			__syncthreads();
		}
	}

	__device__ __forceinline__ void put(uint32_t d, const Cand &c) const
	{
		emit(g.e, d, c.pat, c.off);
		if (d + 2 < g.e.cap)
			g.cand_dl[1 + d] = c.dl;
	}

	template <bool WRITE>
	__device__ __forceinline__ uint32_t record(Row &row, uint32_t i, int32_t o, uint32_t c, uint32_t d, int32_t &)
	{
		if (!WRITE) {
			row = Row{ g.lead_begin, g.open_end, 0, Cand{ 0, 0, 0 } };
			if (i >= r1)   // (no record: no search for its text)
				return 0;
			if (want_text()) {
				int64_t next = INT64_MAX;
				text_bounds(starts_le(st, slice, g.seg_start, g.segments, o), g.segments, [&](uint32_t k) -> int64_t {
					return (st.in_lds && k >= st.k0 && k - st.k0 < st.len) ? slice[k - st.k0] : g.seg_start[k];
				}, row.T0, next);
				if (next <= g.w.text_end)
					row.Tend = next;
			}
		}
		// a pattern cell is a list of its own.  The write walk asks about the same entries as the count walk in
		// front of it: it takes the first 32 answers, and the first kept entry's candidate, from the row
		const uint32_t len = g.states ? list_len_of(g.e, c) : 1u;
		if (len == 0)
			return 0;
		const uint32_t from = g.states ? g.e.list_begin[c] : 0u;
		uint32_t n = 0;
		for (uint32_t j = 0; j < len; j++) {
			const int32_t p = g.states ? g.e.list_pool[from + j] : (int32_t)c;
			if ((uint32_t)p >= g.e.num_patterns)
				continue;
			const uint32_t bit = j < 32 ? 1u << j : 0u;
			Cand cd;
			if (WRITE && bit && !(row.kept & bit))
				continue;
			if (WRITE && bit && n == 0) {
				cd = row.first;
			} else {
				const int v = candidate(g, (uint32_t)p, o, row.T0, row.Tend, cd);
				if (!WRITE)
					und += v == kUndecided;
				if (v != kKeep)
					continue;
			}
			if (WRITE) {
				put(d + n, cd);
			} else {
				row.kept |= bit;
				if (n == 0)
					row.first = cd;
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
			g.info[1] = (int32_t)total;
			g.info[2] = g.info[3] = 0;
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
__global__ __launch_bounds__(kThreads) void k_edit(EditArgs g)
{
	__shared__ int32_t slice[kSliceMax];
	__shared__ uint32_t bounds[2];
	__shared__ uint32_t wave_cnt[kPer * kWaves];
	__shared__ uint32_t red[2 * kWaves];

	EditPass pass(g, slice, bounds);
	entry_pass<WRITE>(g.e, pass, wave_cnt, red);
}

// ---- order and unique ----

struct OrderArgs {
	uint32_t n;                                   // C: the cells that are ordered
	const int32_t *cand_pat, *cand_off;           // [1 + C + 1] the candidates, [0] their count
	const uint32_t *cand_dl;
	int64_t key_lo;
	uint32_t *key, *val;                          // the cells at hand
	uint32_t *flag;                               // [C] in order: 1: differs from the cell in front
	int32_t *counts;                              // [gridDim.x] block counts of the emit step
	const int32_t *cell_plane;                    // the input, for its trailer
	uint32_t max_records;
	int32_t *pat_out, *off_out, *dist_out, *len_out;
	uint32_t cap;
};

__device__ __forceinline__ uint32_t cands_of(const OrderArgs &g) { return min((uint32_t)g.cand_pat[0], g.n); }

// STAGE 0: cell i = candidate i, keyed by pattern.  1: the cells as ordered so far, keyed by offset.  2: the flags.
template <int STAGE>
__global__ __launch_bounds__(kThreads) void k_edit_cells(OrderArgs g)
{
	const uint32_t m = cands_of(g);
	const Share sh = share_of((g.n + kTile - 1) / kTile);
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++)
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t i = t * kTile + q * kThreads + threadIdx.x;
			if (i >= g.n)
				continue;
			if (STAGE == 0) {
				g.key[i] = i < m ? (uint32_t)g.cand_pat[1 + i] : kNoKey;
				g.val[i] = i;
			} else if (STAGE == 1) {
				const uint32_t v = g.val[i];
				g.key[i] = v < m ? (uint32_t)((int64_t)g.cand_off[1 + v] - g.key_lo) : kNoKey;
			} else {
				const uint32_t v = g.val[i];
				uint32_t f = 0;
				if (i < m && v < m) {   // (the candidates are the first m cells: every other key is kNoKey)
					f = 1;
					if (i > 0) {
						const uint32_t u = g.val[i - 1];
						if (u < m && g.key[i - 1] == g.key[i] && g.cand_pat[1 + u] == g.cand_pat[1 + v])
							f = 0;
					}
				}
				g.flag[i] = f;
			}
		}
}

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void k_edit_emit(OrderArgs g)
{
	__shared__ uint32_t wave_cnt[kPer * kWaves];
	__shared__ uint32_t red[2 * kWaves];

	const uint32_t m = cands_of(g);
	emit_flagged<WRITE>(
	    g.flag, m, g.counts, g.cap, wave_cnt, red,
	    [&](uint32_t total) {
		    const int32_t last = g.cell_plane[1 + min((uint32_t)g.cell_plane[0], g.max_records)];   // the trailer is the input's
		    write_ends(g.pat_out, g.cap, total, last);
		    write_ends(g.off_out, g.cap, total, last);
		    if (g.dist_out)
			    write_ends(g.dist_out, g.cap, total, last);
		    if (g.len_out)
			    write_ends(g.len_out, g.cap, total, last);
	    },
	    [&](uint32_t i, uint32_t d) {
		    const uint32_t v = g.val[i];
		    if (v >= m)   // (never: the flag came from it)
			    return;
		    g.pat_out[1 + d] = g.cand_pat[1 + v];
		    g.off_out[1 + d] = g.cand_off[1 + v];
		    const uint32_t dl = g.cand_dl[1 + v];
		    if (g.dist_out)
			    g.dist_out[1 + d] = (int32_t)(dl & 0xFFu);
		    if (g.len_out)
			    g.len_out[1 + d] = (int32_t)(dl >> 8);
	    });
}

// ---- host side ----

struct Layout {
	size_t block_counts, cand_pat, cand_off, cand_dl, key[2], val[2], flag, hist, digit_total, counts, total;
};

// cells: the candidates there is room for
Layout layout_of(size_t max_records, size_t cells)
{
	Layout l;
	size_t at = 0;
	auto take = [&](size_t bytes) {
		const size_t here = at;
		at += round256(bytes);
		return here;
	};
	const uint32_t blocks = std::max(grid_for(max_records), grid_for(cells));
	l.block_counts = take(2 * (size_t)blocks * sizeof(int32_t));
	l.cand_pat = take((cells + 2) * sizeof(int32_t));
	l.cand_off = take((cells + 2) * sizeof(int32_t));
	l.cand_dl = take((cells + 2) * sizeof(uint32_t));
	for (int k = 0; k < 2; k++) {
		l.key[k] = take(cells * sizeof(uint32_t));
		l.val[k] = take(cells * sizeof(uint32_t));
	}
	l.flag = take(cells * sizeof(uint32_t));
	l.hist = take(radix_hist_bytes(blocks));
	l.digit_total = take(radix_digit_total_bytes());
	l.counts = take((size_t)blocks * sizeof(int32_t));
	l.total = std::max<size_t>(at, 256);
	return l;
}

// the candidates max_records records of a STATE plane can give
size_t state_cells(const acm_dfa *d, size_t max_records)
{
	return max_records * (size_t)std::max<uint32_t>(1, d ? d->max_list_len : 1);
}

}  // namespace

extern "C" size_t acm_edit_workspace_bytes(const acm_dfa *d, size_t max_records)
{
	return layout_of(max_records, state_cells(d, max_records)).total;
}

extern "C" int acm_edit_matches_async(const acm_dfa *d, const int32_t *d_pat_plane, const int32_t *d_off_plane, size_t max_records,
    int report, const void *d_text, long text_origin, long text_end, const void *d_before, size_t before_len,
    const int32_t *d_seg_start, size_t segments, long lead_begin, long open_end, int32_t *d_pat_out, int32_t *d_off_out,
    int32_t *d_dist_out, int32_t *d_len_out, size_t out_capacity, int32_t *d_info, void *d_workspace, size_t workspace_bytes,
    void *stream)
{
	EditArgs g;
	const bool own_ok = d_info && (report == ACM_REPORT_STATE || report == ACM_REPORT_HEAD) &&
	                    window_ok(d_text, text_origin, text_end, d_before, before_len) && (!segments || d_seg_start) &&
	                    segments <= 0x7FFFFFFFul && (open_end == -1 || open_end >= text_end);
	const char *tables = tables_error(d, [&](const acm_dfa &a) -> const char * {
		if (report == ACM_REPORT_STATE && (!a.d_list_begin || !a.d_list_len || !a.d_list_pool))
			return "automaton has no match lists";
		return a.approx && (!a.d_approx_ent || !a.d_approx_pool) ? "automaton with approximate patterns without their tables" : nullptr;
	});
	const size_t need = acm_edit_workspace_bytes(d, max_records);
	if (int rc = entry_args(g.e, "acm_edit_matches_async",
	        EntryCall{ d, d_pat_plane, d_off_plane, max_records, 1, d_pat_out, d_off_out, out_capacity, d_workspace, workspace_bytes },
	        own_ok, tables, need))
		return rc;
	const size_t cells = report == ACM_REPORT_STATE ? state_cells(d, max_records) : max_records;
	if (cells > 0x7FFFFFF0ul)
		return acm::fail(ACM_ERR_ARG, "acm_edit_matches_async: %zu records of up to %u entries are too many candidates", max_records,
		    d->max_list_len);
	const Layout l = layout_of(max_records, cells);   // (no larger than the layout of the query)
	char *ws = (char *)d_workspace;
	const uint32_t C = (uint32_t)cells;

	g.e.block_counts = (int32_t *)(ws + l.block_counts);
	g.e.pat_out = (int32_t *)(ws + l.cand_pat);
	g.e.off_out = (int32_t *)(ws + l.cand_off);
	g.e.cap = C + 2;
	g.states = report == ACM_REPORT_STATE;
	g.w = window_of(d, d_text, text_origin, text_end, d_before, before_len, nullptr);
	g.seg_start = d_seg_start;
	g.segments = (uint32_t)segments;
	g.lead_begin = (int64_t)lead_begin;
	g.open_end = open_end == -1 ? kEndUnknown : (int64_t)open_end;
	g.ent = d->approx ? (const int4 *)d->d_approx_ent : nullptr;
	g.pool = d->d_approx_pool;
	g.key_lo = (int64_t)text_origin - (int64_t)before_len;
	g.key_range = (uint32_t)std::min<int64_t>((int64_t)text_end - g.key_lo, 0xFFFFFFFEl);
	g.cand_dl = (uint32_t *)(ws + l.cand_dl);
	g.info = d_info;
	if (int rc = launch_passes(k_edit<false>, k_edit<true>, d, max_records, g, stream))
		return rc;

	OrderArgs r{};
	r.n = C;
	r.cand_pat = g.e.pat_out;
	r.cand_off = g.e.off_out;
	r.cand_dl = g.cand_dl;
	r.key_lo = g.key_lo;
	r.flag = (uint32_t *)(ws + l.flag);
	r.counts = (int32_t *)(ws + l.counts);
	r.cell_plane = d_pat_plane;
	r.max_records = (uint32_t)max_records;
	r.pat_out = d_pat_out;
	r.off_out = d_off_out;
	r.dist_out = d_dist_out;
	r.len_out = d_len_out;
	r.cap = clamp_cap(out_capacity);

	hipStream_t s = (hipStream_t)stream;
	const uint32_t blocks = grid_for(C);
	const dim3 grid(blocks), block(kThreads);
	uint32_t *const key[2] = { (uint32_t *)(ws + l.key[0]), (uint32_t *)(ws + l.key[1]) };
	uint32_t *const val[2] = { (uint32_t *)(ws + l.val[0]), (uint32_t *)(ws + l.val[1]) };
	uint32_t *hist = (uint32_t *)(ws + l.hist), *digit_total = (uint32_t *)(ws + l.digit_total);
	r.key = key[0];
	r.val = val[0];
	hipLaunchKernelGGL(k_edit_cells<0>, grid, block, 0, s, r);
	ACM_HIP_TRY(hipGetLastError());
	int cur = 0;
	ACM_HIP_TRY(radix_order(C, key, val, hist, digit_total, radix_passes(d->num_patterns), blocks, s, cur));
	// the cells ordered by pattern become the input of the order by offset
	uint32_t *const key2[2] = { key[cur], key[cur ^ 1] };
	uint32_t *const val2[2] = { val[cur], val[cur ^ 1] };
	r.key = key2[0];
	r.val = val2[0];
	hipLaunchKernelGGL(k_edit_cells<1>, grid, block, 0, s, r);
	ACM_HIP_TRY(hipGetLastError());
	ACM_HIP_TRY(radix_order(C, key2, val2, hist, digit_total, radix_passes(g.key_range), blocks, s, cur));
	r.key = key2[cur];
	r.val = val2[cur];
	hipLaunchKernelGGL(k_edit_cells<2>, grid, block, 0, s, r);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_edit_emit<false>, grid, block, 0, s, r);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_edit_emit<true>, grid, block, 0, s, r);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}
