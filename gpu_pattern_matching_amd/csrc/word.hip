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
// The pass is a two-launch ordered write over a fixed grid (record_pass.h):
//   k_word<false>  counts the cells every block writes (head: 0 or 1 per input record; all: the
//                  word-bounded entries of the list)
//   k_word<true>   counts again and writes in position order.  Block 0 also writes the tail bytes a
//                  streaming caller hands to its next call.
#include <hip/hip_runtime.h>

#include "acm_internal.h"
#include "device_dfa.h"
#include "record_pass.h"

namespace {

using namespace acm_rp;

struct WordArgs {
	const int32_t *state_plane, *off_plane;
	uint32_t max_records;
	const uint8_t *text;         // byte at offset text_origin + i
	int64_t text_origin, text_end;
	const uint8_t *before;       // bytes at [text_origin - before_len, text_origin)
	int64_t before_len;
	int32_t next_byte;           // byte at text_end, or -1 (the text ends there)
	const int32_t *seg_start;
	uint32_t segments;
	uint32_t wset[8];            // bit b: byte b is a word byte
	int all;
	const uint32_t *list_begin, *list_len;
	const int32_t *list_pool;
	const uint32_t *pat_len;
	uint32_t num_states, num_patterns;
	int32_t *pat_out, *off_out;
	uint32_t cap;
	uint8_t *tail_out;
	uint32_t tail_len;
	int32_t *block_counts;       // [gridDim.x]
};

// the byte at stream offset p, or -1 where there is none: in front of the bytes the caller gave (a
// text start), at text_end when next_byte is -1, and beyond text_end.  Never reads outside
// [text_origin, text_end) of the text or [0, before_len) of before.
__device__ __forceinline__ int byte_at(const WordArgs &g, int64_t p)
{
	if (p >= g.text_origin && p < g.text_end)
		return g.text[p - g.text_origin];
	if (p == g.text_end)
		return g.next_byte;
	if (p < g.text_origin && p >= g.text_origin - g.before_len)
		return g.before[p - (g.text_origin - g.before_len)];
	return -1;
}

__device__ __forceinline__ bool is_word(const uint32_t *wset, int c)
{
	return c >= 0 && ((wset[c >> 5] >> (c & 31)) & 1u);
}

// One record: the number of entries it writes (head: 0 or 1) and, for the head form, the pattern.
// WRITE && all: the entries are written from cell 1 + d on.
template <bool WRITE>
__device__ __forceinline__ uint32_t one_record(const WordArgs &g, const uint32_t *wset, int32_t o, uint32_t s,
    uint32_t d, int32_t &head)
{
	if (s >= g.num_states)   // not the planes of a STATE scan: nothing to report
		return 0;
	const uint32_t len = g.list_len[s];
	if (len == 0)
		return 0;
	// the text this record lies in: [lo, hi) from the segment starts, else the whole stream
	int64_t lo = INT64_MIN, hi = INT64_MAX;
	if (g.segments) {
		const uint32_t ub = upper_bound_i32(g.seg_start, g.segments, o);
		if (ub > 0)
			lo = g.seg_start[ub - 1];
		if (ub < g.segments)
			hi = g.seg_start[ub];
	}
	const int64_t end = (int64_t)o + 1;
	if (end != hi && is_word(wset, byte_at(g, end)))   // runs on into a word: no entry is bounded
		return 0;
	const uint32_t from = g.list_begin[s];
	uint32_t n = 0;
	for (uint32_t j = 0; j < len; j++) {
		const int32_t p = g.list_pool[from + j];
		const uint32_t L = (uint32_t)p < g.num_patterns ? g.pat_len[p] : 0u;
		if (L == 0)
			continue;
		const int64_t a = end - (int64_t)L;
		if (a > lo && is_word(wset, byte_at(g, a - 1)))
			continue;
		if (!g.all) {
			head = p;
			return 1;
		}
		if (WRITE && d + n + 2 < g.cap) {
			g.pat_out[1 + d + n] = p;
			g.off_out[1 + d + n] = o;
		}
		n++;
	}
	return n;
}

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void k_word(WordArgs g)
{
	__shared__ uint32_t wset[8];
	__shared__ uint32_t wave_cnt[kPer * kWaves];
	__shared__ uint32_t red[2 * kWaves];

	const uint32_t tid = threadIdx.x;
	if (tid < 8)
		wset[tid] = g.wset[tid];
	const uint32_t m = min((uint32_t)g.state_plane[0], g.max_records);
	const Share sh = share_of((m + kTile - 1) / kTile);
	__syncthreads();

	if (WRITE && sh.t_begin == sh.t_end && blockIdx.x != 0)   // nothing to write (a batch with few records)
		return;
	uint32_t base = 0;   // WRITE: cells written by the blocks in front of this one
	if (WRITE) {
		uint32_t total;
		base = blocks_before(g.block_counts, red, total);
		if (blockIdx.x == 0) {
			if (tid == 0) {
				const int32_t last = g.state_plane[1 + m];   // the trailer is the input's
				write_ends(g.pat_out, g.cap, total, last);
				write_ends(g.off_out, g.cap, total, last);
			}
			if (g.tail_out)   // the last tail_len bytes of before ++ text, for the next piece's before
				for (uint32_t j = tid; j < g.tail_len; j += kThreads)
					g.tail_out[j] = (uint8_t)byte_at(g, g.text_end - (int64_t)g.tail_len + j);
		}
	}

	uint32_t kept = 0;
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++) {
		const uint32_t r0 = t * kTile, r1 = min(r0 + kTile, m);
		int32_t off[kPer];
		uint32_t state[kPer];
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t i = r0 + q * kThreads + tid;
			off[q] = i < r1 ? g.off_plane[1 + i] : 0;
			state[q] = i < r1 ? (uint32_t)g.state_plane[1 + i] : 0xFFFFFFFFu;
		}
		uint32_t cnt[kPer];
		int32_t head[kPer];
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			head[q] = 0;
			cnt[q] = one_record<false>(g, wset, off[q], state[q], 0, head[q]);
			kept += cnt[q];
		}
		if (!WRITE)
			continue;
		uint32_t incl[kPer], wave_total[kPer];
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			incl[q] = wave_inclusive(cnt[q]);
			wave_total[q] = (uint32_t)__shfl((int)incl[q], 63, 64);
		}
		tile_publish(wave_total, wave_cnt);
		uint32_t tile_total = 0;
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t d = base + tile_row(wave_cnt, q, tile_total) + incl[q] - cnt[q];
			if (cnt[q]) {
				if (!g.all) {
					if (d + 2 < g.cap) {
						g.pat_out[1 + d] = head[q];
						g.off_out[1 + d] = off[q];
					}
				} else {
					int32_t unused;
					(void)one_record<true>(g, wset, off[q], state[q], d, unused);
				}
			}
		}
		base += tile_total;
	}
	if (!WRITE) {
		kept = block_sum(kept, red);
		if (tid == 0)
			g.block_counts[blockIdx.x] = (int32_t)kept;
	}
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
	if (!d || !d_state_plane || !d_off_plane || !d_pat_out || !d_off_out || out_capacity < 2 ||
	    max_records > 0x7FFFFFFEul || text_end < text_origin || (text_end > text_origin && !d_text) ||
	    (before_len && !d_before) || before_len > 0x7FFFFFFFul || next_byte < -1 || next_byte > 255 ||
	    (segments && !d_seg_start) || segments > 0x7FFFFFFFul)
		return acm::fail(ACM_ERR_ARG, "acm_word_matches_async: bad arguments");
	if (!d->d_pat_len && d->num_patterns)
		return acm::fail(ACM_ERR_ARG, "acm_word_matches_async: automaton has no pattern-length table");
	if (!d_workspace || workspace_bytes < acm_word_workspace_bytes(max_records))
		return acm::fail(ACM_ERR_ARG, "acm_word_matches_async: workspace %zu B < required %zu B", workspace_bytes,
		    acm_word_workspace_bytes(max_records));
	hipStream_t s = (hipStream_t)stream;
	ACM_HIP_TRY(hipSetDevice(d->device));
	WordArgs g;
	g.state_plane = d_state_plane;
	g.off_plane = d_off_plane;
	g.max_records = (uint32_t)max_records;
	g.text = (const uint8_t *)d_text;
	g.text_origin = (int64_t)text_origin;
	g.text_end = (int64_t)text_end;
	g.before = (const uint8_t *)d_before;
	g.before_len = (int64_t)before_len;
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
	g.all = all_patterns != 0;
	g.list_begin = d->d_list_begin;
	g.list_len = d->d_list_len;
	g.list_pool = d->d_list_pool;
	g.pat_len = d->d_pat_len;
	g.num_states = d->num_states;
	g.num_patterns = d->num_patterns;
	g.pat_out = d_pat_out;
	g.off_out = d_off_out;
	g.cap = clamp_cap(out_capacity);
	g.tail_out = (uint8_t *)d_tail_out;
	g.tail_len = (uint32_t)std::min<int64_t>((int64_t)d->max_pattern_len, (int64_t)before_len + (text_end - text_origin));
	g.block_counts = (int32_t *)d_workspace;
	const uint32_t blocks = grid_for(max_records);
	hipLaunchKernelGGL(k_word<false>, dim3(blocks), dim3(kThreads), 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_word<true>, dim3(blocks), dim3(kThreads), 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}
