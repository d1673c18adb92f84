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
// The pass is a two-launch ordered write over a fixed grid (record_pass.h):
//   k_case<false>  counts the cells every block writes (head: 0 or 1 per input record; all: the kept
//                  entries of the list)
//   k_case<true>   counts again and writes in position order.  Block 0 also writes the tail bytes a
//                  streaming caller hands to its next call.
#include <hip/hip_runtime.h>

#include "acm_internal.h"
#include "device_dfa.h"
#include "record_pass.h"

namespace {

using namespace acm_rp;

struct CaseArgs {
	const int32_t *state_plane, *off_plane;
	uint32_t max_records;
	const uint8_t *text;         // byte at offset text_origin + i
	int64_t text_origin, text_end;
	const uint8_t *before;       // bytes at [text_origin - before_len, text_origin)
	int64_t before_len;
	int all;
	const uint32_t *list_begin, *list_len;
	const int32_t *list_pool;
	const uint32_t *pat_len;
	const uint2 *case_ent;       // null: the automaton is not mixed, every entry is kept
	const uint32_t *case_pool;
	uint32_t num_states, num_patterns;
	int32_t *pat_out, *off_out;
	uint32_t cap;
	uint8_t *tail_out;
	uint32_t tail_len;
	int32_t *block_counts;       // [gridDim.x]
};

// the byte at stream offset p of before ++ text.  The caller has checked that p lies in it.
__device__ __forceinline__ uint32_t byte_at(const CaseArgs &g, int64_t p)
{
	return p >= g.text_origin ? g.text[p - g.text_origin] : g.before[p - (g.text_origin - g.before_len)];
}

// Does the text at [o - L + 1, o] equal the L >= 1 bytes at word `where` of the pool?  A byte outside
// before ++ text equals nothing.  Never reads outside [0, text_end - text_origin) of the text,
// [0, before_len) of before, or the pool words of this pattern and the one behind them.
__device__ __forceinline__ bool same_bytes(const CaseArgs &g, int64_t o, uint32_t L, uint32_t where)
{
	const int64_t a = o + 1 - (int64_t)L;
	if (o >= g.text_end || a < g.text_origin - g.before_len)
		return false;
	const uint32_t *pw = g.case_pool + where;
	const uint8_t *pb = (const uint8_t *)pw;
	uint32_t i = 0;
	// bytes in `before`, then text bytes up to the first aligned text word
	for (; i < L && a + i < g.text_origin; i++)
		if (g.before[a + i - (g.text_origin - g.before_len)] != pb[i])
			return false;
	if (i == L)
		return true;
	const uint8_t *tp = g.text + (a + i - g.text_origin);
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

// One record: the number of entries it writes (head: 0 or 1) and, for the head form, the pattern.
// WRITE && all: the entries are written from cell 1 + d on.
template <bool WRITE>
__device__ __forceinline__ uint32_t one_record(const CaseArgs &g, int32_t o, uint32_t s, uint32_t d, int32_t &head)
{
	if (s >= g.num_states)   // not the planes of a STATE scan: nothing to report
		return 0;
	const uint32_t len = g.list_len[s];
	if (len == 0)
		return 0;
	const uint32_t from = g.list_begin[s];
	uint32_t n = 0;
	for (uint32_t j = 0; j < len; j++) {
		const int32_t p = g.list_pool[from + j];
		if ((uint32_t)p >= g.num_patterns)
			continue;
		if (g.case_ent) {
			const uint2 e = g.case_ent[p];
			if (e.x != acm::kCaseAny && (e.x == acm::kCaseNever || !same_bytes(g, (int64_t)o, e.y, e.x)))
				continue;
		} else if (g.pat_len[p] == 0) {
			continue;
		}
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
__global__ __launch_bounds__(kThreads) void k_case(CaseArgs g)
{
	__shared__ uint32_t wave_cnt[kPer * kWaves];
	__shared__ uint32_t red[2 * kWaves];

	const uint32_t tid = threadIdx.x;
	const uint32_t m = min((uint32_t)g.state_plane[0], g.max_records);
	const Share sh = share_of((m + kTile - 1) / kTile);

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
			cnt[q] = one_record<false>(g, off[q], state[q], 0, head[q]);
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
					(void)one_record<true>(g, off[q], state[q], d, unused);
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

extern "C" size_t acm_case_workspace_bytes(size_t max_records)
{
	return block_counts_bytes(grid_for(max_records));
}

extern "C" int acm_case_matches_async(const acm_dfa *d, const int32_t *d_state_plane, const int32_t *d_off_plane,
    size_t max_records, const void *d_text, long text_origin, long text_end, const void *d_before, size_t before_len,
    int all_patterns, int32_t *d_pat_out, int32_t *d_off_out, size_t out_capacity, void *d_tail_out, void *d_workspace,
    size_t workspace_bytes, void *stream)
{
	if (!d || !d_state_plane || !d_off_plane || !d_pat_out || !d_off_out || out_capacity < 2 ||
	    max_records > 0x7FFFFFFEul || text_end < text_origin || (text_end > text_origin && !d_text) ||
	    (before_len && !d_before) || before_len > 0x7FFFFFFFul)
		return acm::fail(ACM_ERR_ARG, "acm_case_matches_async: bad arguments");
	if (!d->d_pat_len && d->num_patterns)
		return acm::fail(ACM_ERR_ARG, "acm_case_matches_async: automaton has no pattern-length table");
	if (d->mixed && (!d->d_case_ent || !d->d_case_pool))
		return acm::fail(ACM_ERR_ARG, "acm_case_matches_async: mixed automaton without its case tables");
	if (!d_workspace || workspace_bytes < acm_case_workspace_bytes(max_records))
		return acm::fail(ACM_ERR_ARG, "acm_case_matches_async: workspace %zu B < required %zu B", workspace_bytes,
		    acm_case_workspace_bytes(max_records));
	hipStream_t s = (hipStream_t)stream;
	ACM_HIP_TRY(hipSetDevice(d->device));
	CaseArgs g;
	g.state_plane = d_state_plane;
	g.off_plane = d_off_plane;
	g.max_records = (uint32_t)max_records;
	g.text = (const uint8_t *)d_text;
	g.text_origin = (int64_t)text_origin;
	g.text_end = (int64_t)text_end;
	g.before = (const uint8_t *)d_before;
	g.before_len = (int64_t)before_len;
	g.all = all_patterns != 0;
	g.list_begin = d->d_list_begin;
	g.list_len = d->d_list_len;
	g.list_pool = d->d_list_pool;
	g.pat_len = d->d_pat_len;
	g.case_ent = d->mixed ? (const uint2 *)d->d_case_ent : nullptr;
	g.case_pool = d->d_case_pool;
	g.num_states = d->num_states;
	g.num_patterns = d->num_patterns;
	g.pat_out = d_pat_out;
	g.off_out = d_off_out;
	g.cap = clamp_cap(out_capacity);
	g.tail_out = (uint8_t *)d_tail_out;
	g.tail_len = (uint32_t)std::min<int64_t>((int64_t)d->max_pattern_len, (int64_t)before_len + (text_end - text_origin));
	g.block_counts = (int32_t *)d_workspace;
	const uint32_t blocks = grid_for(max_records);
	hipLaunchKernelGGL(k_case<false>, dim3(blocks), dim3(kThreads), 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_case<true>, dim3(blocks), dim3(kThreads), 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}
