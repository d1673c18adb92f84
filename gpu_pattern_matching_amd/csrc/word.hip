// Whole-word matching (grep -w): keep a pattern only where it stands as a whole word.  gfx950 only.
//
// A word byte is a byte of the caller's set W (default [0-9A-Za-z_]).  Pattern P of length L >= 1
// ending at offset o (starting at a = o - L + 1) is word-bounded when the byte at a - 1 is not in W
// or a is a text start, and the byte at o + 1 is not in W or o + 1 is a text end.  Only the bytes
// outside the match are looked at, as grep -w does.  The records of an ACM_REPORT_STATE scan (or of
// the segment pass in STATE form) carry the final state; its match list names every pattern that
// ends there, and the pattern lengths (acm_dfa.d_pat_len) give every entry's start.  So, as the
// segment pass, this is a pass over records: cost per record, not per text byte, and the scan
// kernels stay as they are.
//
// Per record: the byte after the match is the same for every pattern of the list, so it is tested
// once and a record that runs on into a word is dropped after one byte read.  Then the list is walked
// (one length load and one text-byte gather per entry) as far as the head form needs, the first
// word-bounded entry, or whole for the all form.
//
// The pass is an entry filter (entry_pass.h): k_word<false> counts, k_word<true> writes.  Block
// 0 also writes the tail bytes a streaming caller hands to its next call.
#include <hip/hip_runtime.h>

#include "entry_pass.h"

namespace {

using namespace acm_rp;

struct WordArgs {
	EntryArgs e;                 // the cells are states
	TextWindow w;
	int32_t next_byte;           // byte at text_end, or -1 (the text ends there)
	const int32_t *seg_start;
	uint32_t segments;
	uint32_t wset[8];            // bit b: byte b is a word byte
};

// the byte at stream offset p, or -1 where there is none: in front of the bytes the caller gave (a
// text start), at text_end when next_byte is -1, and beyond text_end.  Never reads outside
// [text_origin, text_end) of the text or [0, before_len) of before.
__device__ __forceinline__ int byte_at(const WordArgs &g, int64_t p)
{
	if (p >= g.w.text_origin && p < g.w.text_end)
		return g.w.text[p - g.w.text_origin];
	if (p == g.w.text_end)
		return g.next_byte;
	if (p < g.w.text_origin && p >= g.w.text_origin - g.w.before_len)
		return g.w.before[p - (g.w.text_origin - g.w.before_len)];
	return -1;
}

__device__ __forceinline__ bool is_word(const uint32_t *wset, int c)
{
	return c >= 0 && ((wset[c >> 5] >> (c & 31)) & 1u);
}

struct WordPass : EntryPass {
	const WordArgs &g;
	const uint32_t *wset;   // g.wset in LDS

	__device__ __forceinline__ WordPass(const WordArgs &g, const uint32_t *wset) : g(g), wset(wset) {}
	__device__ __forceinline__ bool head_form() const { return !g.e.all; }

	template <bool WRITE>
	__device__ __forceinline__ uint32_t record(Row &, uint32_t, int32_t o, uint32_t s, uint32_t d, int32_t &head) const
	{
		if (list_len_of(g.e, s) == 0)   // (walk_list asks again: here it saves the byte read of a record without a list)
			return 0;
		// the text this record lies in: [lo, hi) from the segment starts, else the whole stream
		int64_t lo = INT64_MIN, hi = INT64_MAX;
		if (g.segments)
			text_bounds(upper_bound_i32(g.seg_start, g.segments, o), g.segments,
			    [&](uint32_t k) -> int64_t { return g.seg_start[k]; }, lo, hi);
		const int64_t end = (int64_t)o + 1;
		if (end != hi && is_word(wset, byte_at(g, end)))   // runs on into a word: no entry is bounded
			return 0;
		return walk_list<WRITE>(g.e, o, s, d, head, [&](uint32_t p, int32_t) {
			const uint32_t L = g.e.pat_len[p];
			if (L == 0)
				return false;
			const int64_t a = end - (int64_t)L;
			return !(a > lo && is_word(wset, byte_at(g, a - 1)));
		});
	}
	__device__ __forceinline__ void ready() const { __syncthreads(); }
	__device__ __forceinline__ void block0(uint32_t *) const { write_tail(g.w); }
};

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void k_word(WordArgs g)
{
	__shared__ uint32_t wset[8];
	__shared__ uint32_t wave_cnt[kPer * kWaves];
	__shared__ uint32_t red[2 * kWaves];

	if (threadIdx.x < 8)
		wset[threadIdx.x] = g.wset[threadIdx.x];   // (readable behind the barrier of ready())
	WordPass pass(g, wset);
	entry_pass<WRITE>(g.e, pass, wave_cnt, red);
}

}  // namespace

extern "C" size_t acm_word_workspace_bytes(size_t max_records)
{
	return block_counts_bytes(grid_for(max_records));
}

extern "C" int acm_word_matches_async(const acm_dfa *d, const int32_t *d_state_plane, const int32_t *d_off_plane,
    size_t max_records, const void *d_text, long text_origin, long text_end, const void *d_before, size_t before_len,
    int next_byte, const int32_t *d_seg_start, size_t segments, const uint8_t *word_set, int all_patterns,
    int32_t *d_pat_out, int32_t *d_off_out, size_t out_capacity, void *d_tail_out, void *d_workspace,
    size_t workspace_bytes, void *stream)
{
	WordArgs g;
	const bool own_ok = window_ok(d_text, text_origin, text_end, d_before, before_len) && next_byte >= -1 &&
	                    next_byte <= 255 && (!segments || d_seg_start) && segments <= 0x7FFFFFFFul;
	if (int rc = entry_args(g.e, "acm_word_matches_async",
	        EntryCall{ d, d_state_plane, d_off_plane, max_records, all_patterns, d_pat_out, d_off_out, out_capacity,
	            d_workspace, workspace_bytes },
	        own_ok, nullptr, acm_word_workspace_bytes(max_records)))
		return rc;
	g.w = window_of(d, d_text, text_origin, text_end, d_before, before_len, d_tail_out);
	g.next_byte = next_byte;
	g.seg_start = d_seg_start;
	g.segments = (uint32_t)segments;
	for (int k = 0; k < 8; k++) {
		uint32_t v = 0;
		for (int b = 0; b < 32; b++) {
			const int c = 32 * k + b;
			const bool w = word_set ? ((word_set[c >> 3] >> (c & 7)) & 1) != 0
			                        : ((c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || c == '_');
			v |= (uint32_t)w << b;
		}
		g.wset[k] = v;
	}
	return launch_passes(k_word<false>, k_word<true>, d, max_records, g, stream);
}
