// Wildcard patterns: the bytes around an anchor checked against byte sets.  gfx950 only.
//
// A wildcard pattern (acm_automaton_add_wildcard) is in the automaton with its anchor alone, the longest run
// of exact bytes; the pre positions in front of the anchor and the post positions behind it are its context,
// each a set of byte values.  This pass makes the anchors' records matches.  Entry (p, o) with L >= 1,
// a = o - L + 1 and span [a - pre, o + post], in the text [T0, Tend) its record lies in (int64 throughout):
//   1. no context: kept, whatever its text is
//   2. the span leaves [T0, Tend): dropped (Tend unknown: no end is in the way)
//   3. the span leaves the bytes given, [text_origin - before_len, text_end): undecided, dropped and counted
//   4. kept iff every context byte is in its set and every group holds
// It has the case pass's shape (the text under and around a record is read: TextWindow) and the position
// pass's (the record's text is found in the staged slice of starts; STATE cells or pattern cells; undecided
// entries are counted per block and summed by block 0 into d_info).  Cost per record and per context byte.
//
// Tables (device_dfa.hip, only for a set with contexts): d_wild_ent[p] = {cell index, pre, post, L}, one 16-byte
// load per entry; d_wild_pool, a 16-bit cell per context position, pre cells then post cells, an exact byte or
// 0x100 | class; d_wild_sets[class][8], the interned sets of two or more bytes, at most 256 of them (8 KiB),
// staged in LDS in ready(): a set test is one LDS read.  A set without contexts has none of these; the pass
// then reads d_pat_len, keeps every entry of length >= 1, looks up no text and stages nothing.
//
// Groups (acm_automaton_add_wildcard_groups; tables only for a set that has some): d_grp_ent[p] = {first group,
// groups}; d_grp[g] = {first byte counted from the span's, width w, count | negated << 31, word index of its
// strings in d_grp_pool}, one 16-byte load; d_grp_pool, the strings, each zero-padded to whole words.  A group
// holds iff the w text bytes equal one of its strings (negated: none).  The positions a group covers carry the
// full set, so context_ok passes over them and groups_ok decides, for the few lanes that get that far.  The
// kernels are instantiated a second time for such a set, over WildGroupArgs (141 and 178 VGPRs, nothing in
// scratch): a set without groups runs the code it ran before there were any.  DESIGN.md 6m.
//
// LDS: the slice (8 KiB), the sets (at most 8 KiB, kSetWords) and the ranks' few cells: 16.1 KiB a block.  Eight
// blocks of 256 threads would fill a CU's 32 wave slots with 129 KiB of its 160 KiB: LDS does not bound the
// occupancy.  Registers do: 84 VGPRs (count) and 119 (write) give 5 and 4 waves per SIMD where the position pass
// (61 and 73) has 7 and 6.  DESIGN.md 6j says what that costs.
//
// The pass is an entry filter (entry_pass.h): k_wildcard<false> counts the cells and the
// undecided entries of every block, k_wildcard<true> writes; two launches.
#include <hip/hip_runtime.h>

#include "entry_pass.h"

namespace {

using namespace acm_rp;

constexpr int64_t kEndUnknown = INT64_MIN;
constexpr uint32_t kSetWords = 256 * 8;   // the interned sets, 8 words each

struct WildArgs {
	EntryArgs e;                 // block_counts: [2][gridDim.x]: cells written, undecided entries
	int states;                  // the cells are states (ACM_REPORT_STATE), else pattern indices
	TextWindow w;                // (tail_out: null)
	const int32_t *seg_start;
	uint32_t segments;
	int64_t lead_begin, open_end;   // open_end: kEndUnknown when the caller passed -1
	const int4 *wild_ent;        // null: the set has no contexts, every entry of length >= 1 is kept
	const uint16_t *pool;
	const uint32_t *sets;
	uint32_t classes;
	int32_t *info;               // [4]
	static constexpr bool kGroups = false;
};

// the arguments of the GROUPS kernels: a set without groups is launched with WildArgs as it was, so that its
// kernels are the instructions they were
struct WildGroupArgs : WildArgs {
	const int2 *grp_ent;
	const int4 *grp;
	const uint32_t *grp_pool;
	static constexpr bool kGroups = true;
};

constexpr int kGroupWords = ACM_GROUP_MAX_WIDTH / 4;

enum { kDrop = 0, kKeep = 1, kUndecided = 2 };

// is byte b what context cell c asks for?  sets: the staged sets (LDS).  No branch: the set word is read
// whatever the cell is (its index lies inside the array), so that the tests of a step can be issued together.
__device__ __forceinline__ uint32_t cell_has(const uint32_t *sets, uint32_t c, uint32_t b)
{
	const uint32_t in_set = (sets[(c & 0xFFu) * 8 + (b >> 5)] >> (b & 31)) & 1u;
	return c < 0x100u ? (uint32_t)(c == b) : in_set;
}

// Are the n bytes from stream offset `at` on (all inside before ++ text) what the cells c[0, n) ask for?  Four
// positions a step: their eight loads do not depend on each other, and only the step's verdict branches (a
// long context is a chain of dependent steps for one lane while its wave waits).
__device__ __forceinline__ bool context_ok(const TextWindow &w, const uint32_t *sets, const uint16_t *c, int32_t n, int64_t at)
{
	int32_t i = 0;
	for (; i + 4 <= n; i += 4) {
		const uint32_t b0 = window_byte(w, at + i), b1 = window_byte(w, at + i + 1), b2 = window_byte(w, at + i + 2),
		               b3 = window_byte(w, at + i + 3);
		const uint32_t c0 = c[i], c1 = c[i + 1], c2 = c[i + 2], c3 = c[i + 3];
		if (!(cell_has(sets, c0, b0) & cell_has(sets, c1, b1) & cell_has(sets, c2, b2) & cell_has(sets, c3, b3)))
			return false;
	}
	for (; i < n; i++)
		if (!cell_has(sets, c[i], window_byte(w, at + i)))
			return false;
	return true;
}

// Do the groups of pattern p hold where its span begins at stream offset `first`?  The span lies inside
// before ++ text and a group inside the span.  The w text bytes of a group are packed once into words as the
// pool holds a string (little-endian, zeros behind byte w), then compared word by word with every string until
// one is equal.  The words are indexed by unrolled loops only: they stay in registers.
__device__ __forceinline__ bool groups_ok(const WildGroupArgs &g, uint32_t p, int64_t first)
{
	const int2 ge = g.grp_ent[p];   // {first group, groups}
	for (int32_t k = 0; k < ge.y; k++) {
		const int4 e = g.grp[ge.x + k];   // {rel, width, count | negated << 31, word index}
		const int64_t at = first + e.x;
		const int32_t w = e.y, words = (w + 3) >> 2;
		uint32_t t[kGroupWords];
#pragma unroll
		for (int j = 0; j < kGroupWords; j++) {
			uint32_t v = 0;
#pragma unroll
			for (int b = 0; b < 4; b++)
				if (4 * j + b < w)
					v |= window_byte(g.w, at + 4 * j + b) << (8 * b);
			t[j] = v;
		}
		const uint32_t count = (uint32_t)e.z & 0x7FFFFFFFu;
		const uint32_t *str = g.grp_pool + e.w;
		bool any = false;
		// four strings a step: their first words are four loads that do not wait for each other, and only a
		// string whose first word is the text's has its other words read (early exit per string)
		for (uint32_t c = 0; c < count && !any; c += 4, str += 4 * words) {
			uint32_t hit = 0;
#pragma unroll
			for (uint32_t u = 0; u < 4; u++)
				if (c + u < count)
					hit |= (uint32_t)(str[u * words] == t[0]) << u;
			for (; hit && !any; hit &= hit - 1) {
				const uint32_t *s = str + (uint32_t)(__ffs((int)hit) - 1) * words;
				bool eq = true;
#pragma unroll
				for (int j = 1; j < kGroupWords; j++) {
					if (j >= words || !eq)
						break;
					eq = s[j] == t[j];
				}
				any = eq;
			}
		}
		if (any == (e.z < 0))   // one is equal and negated, or none and not negated
			return false;
	}
	return true;
}

// entry (p, o) in the text [T0, Tend) (Tend: kEndUnknown).  Reads text only inside before ++ text.
template <class Args>
__device__ __forceinline__ int verdict(const Args &g, const uint32_t *sets, uint32_t p, int32_t o, int64_t T0, int64_t Tend)
{
	if (p >= g.e.num_patterns)   // (a cell of a HEAD plane may hold anything)
		return kDrop;
	if (!g.wild_ent)
		return g.e.pat_len[p] != 0 ? kKeep : kDrop;
	const int4 e = g.wild_ent[p];   // {cell index, pre, post, length}
	if (e.w == 0)
		return kDrop;
	if ((e.y | e.z) == 0)
		return kKeep;
	const int64_t last = (int64_t)o + (int64_t)e.z;                          // the span's last byte
	const int64_t first = (int64_t)o + 1 - (int64_t)e.w - (int64_t)e.y;     // and its first
	if (first < T0 || (Tend != kEndUnknown && last >= Tend))
		return kDrop;
	if (first < g.w.text_origin - g.w.before_len || last >= g.w.text_end)
		return kUndecided;
	const uint16_t *c = g.pool + e.x;
	if constexpr (Args::kGroups)   // (behind both contexts: only lanes whose every position held get there)
		return context_ok(g.w, sets, c, e.y, first) && context_ok(g.w, sets, c + e.y, e.z, (int64_t)o + 1) && groups_ok(g, p, first)
		           ? kKeep
		           : kDrop;
	else
		return context_ok(g.w, sets, c, e.y, first) && context_ok(g.w, sets, c + e.y, e.z, (int64_t)o + 1) ? kKeep : kDrop;
}

template <class Args>
struct WildPass : EntryPass {
	const Args &g;
	int32_t *slice;     // kSliceMax cells of LDS
	uint32_t *bounds;   // 2 cells of LDS
	uint32_t *sets;     // kSetWords cells of LDS
	Slice st{};         // the starts the tile spans
	uint32_t r1 = 0;    // the end of the tile's records
	uint32_t und = 0;   // undecided entries this thread dropped
	struct Row {
		int64_t T0, Tend;   // the text of the record (Tend: kEndUnknown)
		uint32_t kept;      // bit k: the k-th entry of the record's list that the walk asks about is kept (k < 32)
	};

	__device__ __forceinline__ WildPass(const Args &g, int32_t *slice, uint32_t *bounds, uint32_t *sets)
	    : g(g), slice(slice), bounds(bounds), sets(sets)
	{
	}
	__device__ __forceinline__ bool head_form() const { return !g.e.all || !g.states; }
	__device__ __forceinline__ bool want_text() const { return g.wild_ent && g.segments; }   // (without contexts no entry asks)

	__device__ __forceinline__ void ready()
	{
		if (g.wild_ent) {   // (uniform over the grid)
			for (uint32_t j = threadIdx.x; j < min(g.classes * 8, kSetWords); j += kThreads)
				sets[j] = g.sets[j];
			__syncthreads();
		}
	}

	__device__ __forceinline__ void tile(uint32_t r0, uint32_t r1)
	{
		this->r1 = r1;
		if (want_text()) {
			st = stage_slice(g.e.off_plane, r0, r1, g.seg_start, g.segments, slice, bounds);
			__syncthreads();
		}
	}

	// !WRITE: finds the record's text and adds its undecided entries to und
	template <bool WRITE>
	__device__ __forceinline__ uint32_t record(Row &row, uint32_t i, int32_t o, uint32_t c, uint32_t d, int32_t &head)
	{
		if (!WRITE) {
			row = Row{ g.lead_begin, g.open_end, 0 };
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
		if (g.states) {
			// the write walk asks about the same entries in the same order as the count walk in front of it: it
			// takes the first 32 answers from the row and reads no text again
			uint32_t k = 0;
			return walk_list<WRITE>(g.e, o, c, d, head, [&](uint32_t p, int32_t o) {
				const uint32_t bit = k < 32 ? 1u << k : 0u;
				k++;
				if (WRITE && bit)
					return (row.kept & bit) != 0;
				const int v = verdict(g, sets, p, o, row.T0, row.Tend);
				if (!WRITE) {
					und += v == kUndecided;
					row.kept |= v == kKeep ? bit : 0u;
				}
				return v == kKeep;
			});
		}
		const int v = verdict(g, sets, c, o, row.T0, row.Tend);   // (pattern cells come in the all form only)
		und += v == kUndecided;
		head = (int32_t)c;
		return v == kKeep;
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

template <bool WRITE, class Args>
__global__ __launch_bounds__(kThreads) void k_wildcard(Args g)
{
	__shared__ int32_t slice[kSliceMax];
	__shared__ uint32_t sets[kSetWords];
	__shared__ uint32_t bounds[2];
	__shared__ uint32_t wave_cnt[kPer * kWaves];
	__shared__ uint32_t red[2 * kWaves];

	WildPass<Args> pass(g, slice, bounds, sets);
	entry_pass<WRITE>(g.e, pass, wave_cnt, red);
}

}  // namespace

extern "C" size_t acm_wildcard_workspace_bytes(size_t max_records)
{
	return round256(2 * (size_t)grid_for(max_records) * sizeof(int32_t));
}

extern "C" int acm_wildcard_matches_async(const acm_dfa *d, const int32_t *d_pat_plane, const int32_t *d_off_plane,
    size_t max_records, int report, const void *d_text, long text_origin, long text_end, const void *d_before,
    size_t before_len, const int32_t *d_seg_start, size_t segments, long lead_begin, long open_end, int all_patterns,
    int32_t *d_pat_out, int32_t *d_off_out, size_t out_capacity, int32_t *d_info, void *d_workspace, size_t workspace_bytes,
    void *stream)
{
	WildGroupArgs g;
	const bool own_ok = d_info && (report == ACM_REPORT_STATE || (report == ACM_REPORT_HEAD && all_patterns)) &&
	                    window_ok(d_text, text_origin, text_end, d_before, before_len) && (!segments || d_seg_start) &&
	                    segments <= 0x7FFFFFFFul && (open_end == -1 || open_end >= text_end);
	const char *tables = tables_error(d, [&](const acm_dfa &a) -> const char * {
		if (report == ACM_REPORT_STATE && (!a.d_list_begin || !a.d_list_len || !a.d_list_pool))
			return "automaton has no match lists";
		if (a.wild && (!a.d_wild_ent || !a.d_wild_pool || !a.d_wild_sets || a.wild_classes > 256))
			return "automaton with wildcard contexts without their tables";
		return a.groups && (!a.wild || !a.d_grp_ent || !a.d_grp || !a.d_grp_pool) ? "automaton with groups without their tables"
		                                                                         : nullptr;
	});
	if (int rc = entry_args(g.e, "acm_wildcard_matches_async",
	        EntryCall{ d, d_pat_plane, d_off_plane, max_records, all_patterns, d_pat_out, d_off_out, out_capacity, d_workspace,
	            workspace_bytes },
	        own_ok, tables, acm_wildcard_workspace_bytes(max_records)))
		return rc;
	g.states = report == ACM_REPORT_STATE;
	g.w = window_of(d, d_text, text_origin, text_end, d_before, before_len, nullptr);
	g.seg_start = d_seg_start;
	g.segments = (uint32_t)segments;
	g.lead_begin = (int64_t)lead_begin;
	g.open_end = open_end == -1 ? kEndUnknown : (int64_t)open_end;
	g.wild_ent = d->wild ? (const int4 *)d->d_wild_ent : nullptr;
	g.pool = d->d_wild_pool;
	g.sets = d->d_wild_sets;
	g.classes = d->wild_classes;
	g.info = d_info;
	g.grp_ent = (const int2 *)d->d_grp_ent;
	g.grp = (const int4 *)d->d_grp;
	g.grp_pool = d->d_grp_pool;
	if (d->groups)
		return launch_passes(k_wildcard<false, WildGroupArgs>, k_wildcard<true, WildGroupArgs>, d, max_records, g, stream);
	return launch_passes(k_wildcard<false, WildArgs>, k_wildcard<true, WildArgs>, d, max_records, (const WildArgs &)g, stream);
}
