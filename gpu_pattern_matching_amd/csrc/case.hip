// Case sensitivity per pattern: the candidates of a mixed automaton made exact.  gfx950 only.
//
// A mixed automaton (acm_automaton_add_ex: some patterns ignore ASCII case, some do not) is built and
// scanned as the nocase automaton of the same patterns, so a record's match list names every pattern P
// with fold(text under P) == fold(P).  An entry that ignores case is a match as it stands; an exact
// entry is one iff the text under it equals P's bytes as added.  As the word pass this is a pass over
// the records of an ACM_REPORT_STATE scan (or of the segment pass in STATE form): the list of the
// record's state is walked, the pattern lengths give every entry's start, and a predicate on the text
// keeps or drops the entry.  Cost per record and per pattern byte under it, not per text byte, and the
// scan kernels stay as they are.
//
// Tables (device_dfa.hip, mixed automata only): d_case_ent[p] = {where, length}, one 8-byte load per
// entry.  where = kCaseAny: the pattern ignores case, nothing else is read.  Else it is the word index
// of the pattern's bytes as added in d_case_pool, where every exact pattern starts on a word and one
// spare word lies behind the last.  The compare walks the text: bytes up to the text's first aligned
// word (and the bytes that lie in `before`, a streaming caller's previous tail), then whole aligned text
// words against the pattern's bytes at that shift (two pool words and v_alignbyte), then the last bytes.
// The pool is the patterns back to back, a few hundred KiB at most for the sets this project scans: the
// gathers into it are uncoalesced by nature (one pattern per lane) and live in L2.
//
// The pass is an entry filter (entry_pass.h): k_case<false> counts, k_case<true> writes.  Block
// 0 also writes the tail bytes a streaming caller hands to its next call.
#include <hip/hip_runtime.h>

#include "entry_pass.h"

namespace {

using namespace acm_rp;

struct CaseArgs {
	EntryArgs e;                 // the cells are states
	TextWindow w;
	const uint2 *case_ent;       // null: the automaton is not mixed, every entry is kept
	const uint32_t *case_pool;
};

// Does the text at [o - L + 1, o] equal the L >= 1 bytes at word `where` of the pool?  A byte outside
// before ++ text equals nothing.  Never reads outside [0, text_end - text_origin) of the text,
// [0, before_len) of before, or the pool words of this pattern and the one behind them.
__device__ __forceinline__ bool same_bytes(const TextWindow &w, const uint32_t *case_pool, int64_t o, uint32_t L, uint32_t where)
{
	const int64_t a = o + 1 - (int64_t)L;
	if (o >= w.text_end || a < w.text_origin - w.before_len)
		return false;
	const uint32_t *pw = case_pool + where;
	const uint8_t *pb = (const uint8_t *)pw;
	uint32_t i = 0;
	// bytes in `before`, then text bytes up to the first aligned text word
	for (; i < L && a + i < w.text_origin; i++)
		if (w.before[a + i - (w.text_origin - w.before_len)] != pb[i])
			return false;
	if (i == L)
		return true;
	const uint8_t *tp = w.text + (a + i - w.text_origin);
	for (; i < L && ((uintptr_t)tp & 3); i++, tp++)
		if (*tp != pb[i])
			return false;
	if (i + 4 <= L) {
		uint32_t k = i >> 2;
		const uint32_t shift = i & 3;
		uint32_t lo = pw[k];
		for (; i + 4 <= L; i += 4, tp += 4) {
			const uint32_t hi = pw[++k];   // (at most the spare word behind the pattern's own)
			if (*(const uint32_t *)tp != __builtin_amdgcn_alignbyte(hi, lo, shift))
				return false;
			lo = hi;
		}
	}
	for (; i < L; i++, tp++)
		if (*tp != pb[i])
			return false;
	return true;
}

struct CasePass : EntryPass {
	const CaseArgs &g;

	__device__ __forceinline__ explicit CasePass(const CaseArgs &g) : g(g) {}
	__device__ __forceinline__ bool head_form() const { return !g.e.all; }

	template <bool WRITE>
	__device__ __forceinline__ uint32_t record(Row &, uint32_t, int32_t o, uint32_t s, uint32_t d, int32_t &head) const
	{
		return walk_list<WRITE>(g.e, o, s, d, head, [&](uint32_t p, int32_t o) {
			if (g.case_ent) {
				const uint2 e = g.case_ent[p];
				return e.x == acm::kCaseAny || (e.x != acm::kCaseNever && same_bytes(g.w, g.case_pool, (int64_t)o, e.y, e.x));
			}
			return g.e.pat_len[p] != 0;
		});
	}
	__device__ __forceinline__ void block0(uint32_t *) const { write_tail(g.w); }
};

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void k_case(CaseArgs g)
{
	__shared__ uint32_t wave_cnt[kPer * kWaves];
	__shared__ uint32_t red[2 * kWaves];

	CasePass pass(g);
	entry_pass<WRITE>(g.e, pass, wave_cnt, red);
}

}  // namespace

extern "C" size_t acm_case_workspace_bytes(size_t max_records)
{
	return block_counts_bytes(grid_for(max_records));
}

extern "C" int acm_case_matches_async(const acm_dfa *d, const int32_t *d_state_plane, const int32_t *d_off_plane,
    size_t max_records, const void *d_text, long text_origin, long text_end, const void *d_before, size_t before_len,
    int all_patterns, int32_t *d_pat_out, int32_t *d_off_out, size_t out_capacity, void *d_tail_out, void *d_workspace,
    size_t workspace_bytes, void *stream)
{
	CaseArgs g;
	const char *tables = tables_error(d, [](const acm_dfa &a) {
		return a.mixed && (!a.d_case_ent || !a.d_case_pool) ? "mixed automaton without its case tables" : nullptr;
	});
	if (int rc = entry_args(g.e, "acm_case_matches_async",
	        EntryCall{ d, d_state_plane, d_off_plane, max_records, all_patterns, d_pat_out, d_off_out, out_capacity,
	            d_workspace, workspace_bytes },
	        window_ok(d_text, text_origin, text_end, d_before, before_len), tables, acm_case_workspace_bytes(max_records)))
		return rc;
	g.w = window_of(d, d_text, text_origin, text_end, d_before, before_len, d_tail_out);
	g.case_ent = d->mixed ? (const uint2 *)d->d_case_ent : nullptr;
	g.case_pool = d->d_case_pool;
	return launch_passes(k_case<false>, k_case<true>, d, max_records, g, stream);
}
