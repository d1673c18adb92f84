// Position constraints per pattern: where in its text an entry may start.  gfx950 only.
//
// A window (acm_automaton_set_position) keeps pattern p of length L >= 1 that ends at offset o, so starts
// at a = o - L + 1, iff lo <= a - T0 <= hi (from the start of its text [T0, Tend)) or, with
// ACM_POS_FROM_END, lo <= Tend - a <= hi.  The predicate needs no text: the pattern's length, the offset
// and the bounds of the text the record lies in.  So the pass takes either form of plane:
//   ACM_REPORT_STATE  final states: the entries of a record are its state's match list (as word.hip,
//                     case.hip)
//   ACM_REPORT_HEAD   pattern indices, one entry per record: a HEAD scan, or what the word, case and
//                     expand passes write in their all-patterns form.  A run of records with equal offset
//                     is one offset.
// The text of a record is found as the tally finds its row: the starts a tile spans are staged in LDS
// (record_pass.h) and searched once per record; the start behind it, if it is <= text_end, is the text's
// end.  Otherwise the text is open: its end is open_end, or unknown (-1), and then an end-anchored entry
// is undecided: dropped and counted.
//
// Tables (device_dfa.hip, positioned automata only): d_pos_ent[p] = {lo, hi, flags, length}, one 16-byte
// load per entry.  An automaton without constraints has none; the pass then reads d_pat_len, keeps every
// entry of length >= 1 and looks up no segment.
//
// The pass is an entry filter (entry_pass.h): k_position<false> counts the cells every block
// writes and the undecided entries it drops, k_position<true> writes; block 0 also writes d_info (the sum of
// the blocks' undecided counts: integers, the same on every run).
// First-entry form over HEAD input: a record that is kept (or undecided) is the first of its run iff no
// record in front of it with the same offset is kept; it finds that by looking back through the input
// plane and evaluating the predicate again (same offset, so same text).  No state is shared between
// threads, so tile and block cuts do not matter.
#include <hip/hip_runtime.h>

#include "entry_pass.h"

namespace {

using namespace acm_rp;

constexpr int64_t kEndUnknown = INT64_MIN;

struct PosArgs {
	EntryArgs e;                 // block_counts: [2][gridDim.x]: cells written, undecided entries
	int states;                  // the cells are states (ACM_REPORT_STATE), else pattern indices
	const int32_t *seg_start;
	uint32_t segments;
	int64_t lead_begin, text_end, open_end;   // open_end: kEndUnknown when the caller passed -1
	const int4 *pos_ent;         // null: the automaton is not positioned, every entry of length >= 1 is kept
	int32_t *info;               // [4]
};

enum { kDrop = 0, kKeep = 1, kUndecided = 2 };

// the window of pattern p at offset o of the text [T0, Tend) (Tend: kEndUnknown)
__device__ __forceinline__ int verdict(const PosArgs &g, uint32_t p, int32_t o, int64_t T0, int64_t Tend)
{
	if (p >= g.e.num_patterns)   // (a cell of a HEAD plane may hold anything)
		return kDrop;
	if (!g.pos_ent)
		return g.e.pat_len[p] != 0 ? kKeep : kDrop;
	const int4 e = g.pos_ent[p];   // {lo, hi, flags, length}
	if (e.w == 0)
		return kDrop;
	if (e.x == 0 && e.y == INT32_MAX && e.z == 0)
		return kKeep;
	const int64_t a = (int64_t)o + 1 - (int64_t)e.w;
	int64_t v;
	if (e.z & ACM_POS_FROM_END) {
		if (Tend == kEndUnknown)
			return kUndecided;
		v = Tend - a;
	} else {
		v = a - T0;
	}
	return (v >= (int64_t)e.x && (e.y == INT32_MAX || v <= (int64_t)e.y)) ? kKeep : kDrop;
}

struct PosPass : EntryPass {
	const PosArgs &g;
	int32_t *slice;     // kSliceMax cells of LDS
	uint32_t *bounds;   // 2 cells of LDS
	Slice st{};         // the starts the tile spans
	uint32_t r1 = 0;    // the end of the tile's records
	uint32_t und = 0;   // undecided entries this thread dropped
	struct Row {
		int64_t T0, Tend;   // the text of the record (Tend: kEndUnknown)
	};

	__device__ __forceinline__ PosPass(const PosArgs &g, int32_t *slice, uint32_t *bounds) : g(g), slice(slice), bounds(bounds) {}
	__device__ __forceinline__ bool head_form() const { return !g.e.all || !g.states; }
	__device__ __forceinline__ bool want_text() const { return g.pos_ent && g.segments; }   // (without windows no entry asks)

	__device__ __forceinline__ void tile(uint32_t r0, uint32_t r1)
	{
		this->r1 = r1;
		if (want_text()) {
			st = stage_slice(g.e.off_plane, r0, r1, g.seg_start, g.segments, slice, bounds);
			__syncthreads();
		}
	}

	// !WRITE: finds the record's text and adds its undecided entries to und.  First form over HEAD input: a
	// record that is kept or undecided counts only as the first such of its run.
	template <bool WRITE>
	__device__ __forceinline__ uint32_t record(Row &row, uint32_t i, int32_t o, uint32_t c, uint32_t d, int32_t &head)
	{
		if (!WRITE) {
			row = Row{ g.lead_begin, g.open_end };
			if (i >= r1)   // (no record: no search for its text)
				return 0;
			if (want_text()) {
				int64_t next = INT64_MAX;
				// start number k, from the staged slice where it holds it
				text_bounds(starts_le(st, slice, g.seg_start, g.segments, o), g.segments, [&](uint32_t k) -> int64_t {
					return (st.in_lds && k >= st.k0 && k - st.k0 < st.len) ? slice[k - st.k0] : g.seg_start[k];
				}, row.T0, next);
				if (next <= g.text_end)
					row.Tend = next;
			}
		}
		if (g.states)
			return walk_list<WRITE>(g.e, o, c, d, head, [&](uint32_t p, int32_t o) {
				const int v = verdict(g, p, o, row.T0, row.Tend);
				if (!WRITE)
					und += v == kUndecided;
				return v == kKeep;
			});
		const int v = verdict(g, c, o, row.T0, row.Tend);
		if (v == kDrop)
			return 0;
		if (!g.e.all)   // first of its run?  The records in front with this offset lie in the same text.
			for (uint32_t j = i; j > 0; j--) {
				if (g.e.off_plane[j] != o)   // (cell j holds record j - 1)
					break;
				if (verdict(g, (uint32_t)g.e.cell_plane[j], o, row.T0, row.Tend) == kKeep)
					return 0;
			}
		if (v == kUndecided) {
			und++;
			return 0;
		}
		head = (int32_t)c;
		return 1;
	}

	__device__ __forceinline__ void block0(uint32_t *red)
	{
		uint32_t u = 0;
		for (uint32_t j = threadIdx.x; j < gridDim.x; j += kThreads)
			u += (uint32_t)g.e.block_counts[gridDim.x + j];
		u = block_sum(u, red);
		if (threadIdx.x == 0) {
			g.info[0] = (int32_t)u;
			g.info[1] = g.info[2] = g.info[3] = 0;
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
__global__ __launch_bounds__(kThreads) void k_position(PosArgs g)
{
	__shared__ int32_t slice[kSliceMax];
	__shared__ uint32_t bounds[2];
	__shared__ uint32_t wave_cnt[kPer * kWaves];
	__shared__ uint32_t red[2 * kWaves];

	PosPass pass(g, slice, bounds);
	entry_pass<WRITE>(g.e, pass, wave_cnt, red);
}

}  // namespace

extern "C" size_t acm_position_workspace_bytes(size_t max_records)
{
	return round256(2 * (size_t)grid_for(max_records) * sizeof(int32_t));
}

extern "C" int acm_position_matches_async(const acm_dfa *d, const int32_t *d_pat_plane, const int32_t *d_off_plane,
    size_t max_records, int report, const int32_t *d_seg_start, size_t segments, long lead_begin, long text_end,
    long open_end, int all_patterns, int32_t *d_pat_out, int32_t *d_off_out, size_t out_capacity, int32_t *d_info,
    void *d_workspace, size_t workspace_bytes, void *stream)
{
	PosArgs g;
	const bool own_ok = d_info && (report == ACM_REPORT_HEAD || report == ACM_REPORT_STATE) && (!segments || d_seg_start) &&
	                    segments <= 0x7FFFFFFFul && (open_end == -1 || open_end >= text_end);
	const char *tables = tables_error(d, [&](const acm_dfa &a) -> const char * {
		if (report == ACM_REPORT_STATE && (!a.d_list_begin || !a.d_list_len || !a.d_list_pool))
			return "automaton has no match lists";
		return a.positioned && !a.d_pos_ent ? "positioned automaton without its window table" : nullptr;
	});
	if (int rc = entry_args(g.e, "acm_position_matches_async",
	        EntryCall{ d, d_pat_plane, d_off_plane, max_records, all_patterns, d_pat_out, d_off_out, out_capacity, d_workspace,
	            workspace_bytes },
	        own_ok, tables, acm_position_workspace_bytes(max_records)))
		return rc;
	g.states = report == ACM_REPORT_STATE;
	g.seg_start = d_seg_start;
	g.segments = (uint32_t)segments;
	g.lead_begin = (int64_t)lead_begin;
	g.text_end = (int64_t)text_end;
	g.open_end = open_end == -1 ? kEndUnknown : (int64_t)open_end;
	g.pos_ent = d->positioned ? (const int4 *)d->d_pos_ent : nullptr;
	g.info = d_info;
	return launch_passes(k_position<false>, k_position<true>, d, max_records, g, stream);
}
