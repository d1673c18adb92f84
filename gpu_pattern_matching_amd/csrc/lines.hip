// Line index on the device: where the lines of a text begin, which line an offset is on, which lines
// hold a record.  gfx950 only.  No automaton is involved.
//
// acm_line_index_async is the one pass here that runs over every text byte; two launches over a fixed
// grid (every block owns a contiguous run of 16 KiB tiles of the text), the text is read once:
//   k_line_mask   each lane loads 16 B (dwordx4) per step, four steps in flight, and tests the four words
//                 with a carry-free SWAR byte equality (exact per byte); the 16 hits become one uint16 of
//                 a 1-bit-per-byte mask in the workspace (n / 8 bytes), their popcount is summed per block
//   k_line_write  reads the mask 64 bits per lane, ranks the set bits with popcount and the block
//                 primitives of record_pass.h, and writes the starts in order.  Every
//                 block then takes a share of the INT32_MAX tail, block 0 writes d_info.
// Bytes in [n, round16(n)) are loaded (the scan's contract allows it) and masked off before they count.
//
// acm_line_number_async: a binary search per offset.  acm_line_select_async: a bit per line in the
// workspace, zeroed, set by one launch over the records (atomic or, skipped where the bit is already
// set), then the two-launch ordered write of record_pass.h over the bits.  Cost per record and per line,
// never per text byte.  acm_line_context_async: the same bits, a prefix of their counts, and per line a
// window clamped to its text; heads and tails of the runs of kept lines, written in order (see "context").
// acm_line_context_lines_async: the same with the kept bits as a plane and one ordered write over them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "acm_internal.h"
#include "record_pass.h"

namespace {

using namespace acm_rp;

constexpr size_t kCountBytes = kMaxBlocks * 4;   // the block counts in front of the masks / flags
constexpr uint32_t kTileWords = kThreads;        // 64-bit mask words per tile: 16 KiB of text
constexpr int kInFlight = 4;                     // 16-byte loads a lane has in flight in k_line_mask
constexpr int32_t kSentinel = 0x7FFFFFFF;

// 4 bits: byte j of w equals the byte every byte of pat repeats.  No carry crosses a byte: exact.
__device__ __forceinline__ uint32_t eq4(uint32_t w, uint32_t pat)
{
	const uint32_t x = w ^ pat;
	const uint32_t t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);   // 0x80 where the byte of x is 0
	return (((t >> 7) * 0x00204081u) >> 21) & 0xFu;   // bits 0, 8, 16, 24 -> 0, 1, 2, 3 (all partial products distinct)
}

struct Words {
	uint32_t w_begin, w_end;   // the block's mask words
};

__device__ __forceinline__ Words words_of(uint32_t words)
{
	const Share sh = share_of((words + kTileWords - 1) / kTileWords);
	return Words{ sh.t_begin * kTileWords, min(sh.t_end * kTileWords, words) };
}

// ------------------------------------------------------------------ index

struct IndexArgs {
	const uint4 *text;
	uint32_t n, groups, words;   // bytes; 16-byte groups that hold text; 64-bit mask words (4 groups each)
	int64_t origin;
	uint32_t delim;
	int prev_byte;
	const int32_t *prev_info;
	int32_t *line_start;
	uint32_t capacity;
	int32_t *info;
	int32_t *block_counts;
	uint16_t *mask16;            // [4 * words]
};

__global__ __launch_bounds__(kThreads) void k_line_mask(IndexArgs g)
{
	__shared__ uint32_t red[kWaves];
	const Words sh = words_of(g.words);
	const uint32_t g_end = sh.w_end * 4, pat = g.delim * 0x01010101u;
	uint32_t count = 0;
	for (uint32_t base = sh.w_begin * 4; base < g_end; base += kThreads * kInFlight) {
		uint4 v[kInFlight];
#pragma unroll
		for (int q = 0; q < kInFlight; q++) {
			const uint32_t i = base + q * kThreads + threadIdx.x;
			v[q] = i < min(g_end, g.groups) ? g.text[i] : make_uint4(0, 0, 0, 0);
		}
#pragma unroll
		for (int q = 0; q < kInFlight; q++) {
			const uint32_t i = base + q * kThreads + threadIdx.x;
			if (i >= g_end)
				continue;
			uint32_t m = 0;
			if (i < g.groups) {
				m = eq4(v[q].x, pat) | eq4(v[q].y, pat) << 4 | eq4(v[q].z, pat) << 8 | eq4(v[q].w, pat) << 12;
				const uint32_t left = g.n - i * 16;   // >= 1
				if (left < 16)
					m &= (1u << left) - 1;            // the bytes behind n never count
			}
			g.mask16[i] = (uint16_t)m;
			count += (uint32_t)__popc(m);
		}
	}
	count = block_sum(count, red);
	if (threadIdx.x == 0)
		g.block_counts[blockIdx.x] = (int32_t)count;
}

__global__ __launch_bounds__(kThreads) void k_line_write(IndexArgs g)
{
	__shared__ uint32_t red[2 * kWaves];
	const unsigned long long *mask64 = (const unsigned long long *)g.mask16;
	uint32_t delims;
	const uint32_t before = blocks_before(g.block_counts, red, delims);
	const bool begins = g.prev_info ? g.prev_info[3] != 0 : (g.prev_byte < 0 || (uint32_t)g.prev_byte == g.delim);
	const uint32_t org = g.n && begins ? 1 : 0;
	const uint32_t last_word = g.n ? (g.n - 1) / 64 : 0, last_bit = g.n ? (g.n - 1) % 64 : 0;
	const bool ends = g.n && (mask64[last_word] >> last_bit & 1);   // a delimiter on the last byte opens no line here
	const uint32_t m = org + delims - (ends ? 1 : 0);

	const Words sh = words_of(g.words);
	uint32_t base = org + before;
	for (uint32_t w0 = sh.w_begin; w0 < sh.w_end; w0 += kTileWords) {
		const uint32_t w = w0 + threadIdx.x;
		unsigned long long bits = w < sh.w_end ? mask64[w] : 0;
		if (ends && w == last_word)
			bits &= ~(1ull << last_bit);
		uint32_t tile_total;
		uint32_t rank = base + block_prefix((uint32_t)__popcll(bits), red, tile_total);
		while (bits) {
			const uint32_t b = (uint32_t)__ffsll((long long)bits) - 1;
			bits &= bits - 1;
			if (rank < g.capacity)
				g.line_start[rank] = (int32_t)(g.origin + (int64_t)w * 64 + b + 1);
			rank++;
		}
		base += tile_total;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		if (org)
			g.line_start[0] = (int32_t)g.origin;   // (capacity >= 1)
		unsigned long long in_front = 0;
		if (g.prev_info)
			in_front = ((unsigned long long)(uint32_t)g.prev_info[4] | (unsigned long long)(uint32_t)g.prev_info[5] << 32) +
			    (unsigned long long)(uint32_t)g.prev_info[1];
		g.info[0] = (int32_t)m;
		g.info[1] = (int32_t)delims;
		g.info[2] = (int32_t)org;
		g.info[3] = g.n ? (ends ? 1 : 0) : (begins ? 1 : 0);
		g.info[4] = (int32_t)(uint32_t)in_front;
		g.info[5] = (int32_t)(uint32_t)(in_front >> 32);
		g.info[6] = 0;
		g.info[7] = 0;
	}
	// the tail behind the starts, shared by the whole grid
	for (uint64_t i = (uint64_t)min(m, g.capacity) + (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < g.capacity;
	     i += (uint64_t)gridDim.x * kThreads)
		g.line_start[i] = kSentinel;
}

// ------------------------------------------------------------------ number

__device__ __forceinline__ uint32_t stored_starts(const int32_t *info, uint32_t capacity)
{
	return (uint32_t)min((int64_t)max(info[0], 0), (int64_t)capacity);
}

__global__ __launch_bounds__(kThreads) void k_line_number(const int32_t *line_start, uint32_t capacity, const int32_t *info,
    const int32_t *offsets, const int32_t *d_count, uint32_t count, int32_t *out)
{
	const uint32_t cnt = d_count ? min(count, (uint32_t)max(*d_count, 0)) : count;
	const uint32_t L = stored_starts(info, capacity);
	const int32_t org = info[2];
	for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < cnt; i += gridDim.x * kThreads)
		out[i] = (int32_t)upper_bound_i32(line_start, L, offsets[i]) - org;
}

// ------------------------------------------------------------------ select

struct SelectArgs {
	const int32_t *line_start;
	uint32_t capacity;
	const int32_t *info;
	int64_t origin, end;
	const int32_t *off_plane;
	uint32_t max_records;
	int invert;
	int32_t *rel_out, *begin_out, *next_out;
	uint32_t cap;
	int32_t *block_counts;
	uint32_t *flags;   // a bit per line: the lead (if there is one), then the starts
};

// the lines of the piece: lead = 1 when bytes lie in front of the first start
__device__ __forceinline__ uint32_t lines_of(const SelectArgs &g, uint32_t &L, uint32_t &lead)
{
	L = stored_starts(g.info, g.capacity);
	lead = g.end > g.origin && g.info[2] == 0 ? 1 : 0;
	return L + lead;
}

__global__ __launch_bounds__(kThreads) void k_line_mark(SelectArgs g)
{
	uint32_t L, lead;
	const uint32_t lines = lines_of(g, L, lead);
	const uint32_t m = min((uint32_t)max(g.off_plane[0], 0), g.max_records);
	for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < m; i += gridDim.x * kThreads) {
		const int32_t o = g.off_plane[1 + i];
		if ((int64_t)o < g.origin || (int64_t)o >= g.end)
			continue;
		const uint32_t ub = upper_bound_i32(g.line_start, L, o);
		if (ub + lead == 0)
			continue;
		const uint32_t line = ub + lead - 1;
		if (line >= lines)
			continue;
		const uint32_t bit = 1u << (line & 31);
		if (!(g.flags[line >> 5] & bit))   // records are in offset order: most find their line marked
			atomicOr(&g.flags[line >> 5], bit);
	}
}

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void k_line_select(SelectArgs g)
{
	__shared__ uint32_t red[2 * kWaves];
	uint32_t L, lead;
	const uint32_t lines = lines_of(g, L, lead);
	const uint32_t words = (lines + 31) / 32;
	const Words sh = words_of(words);
	uint32_t base = 0, total = 0;
	if (WRITE) {
		base = blocks_before(g.block_counts, red, total);
		if (blockIdx.x == 0 && threadIdx.x == 0) {
			write_ends(g.rel_out, g.cap, total, 0);
			write_ends(g.begin_out, g.cap, total, 0);
			write_ends(g.next_out, g.cap, total, 0);
		}
	}
	uint32_t kept = 0;
	for (uint32_t w0 = sh.w_begin; w0 < sh.w_end; w0 += kTileWords) {
		const uint32_t w = w0 + threadIdx.x;
		uint32_t bits = 0;
		if (w < sh.w_end) {
			bits = g.invert ? ~g.flags[w] : g.flags[w];
			const uint32_t left = lines - w * 32;   // >= 1
			if (left < 32)
				bits &= (1u << left) - 1;
		}
		if (!WRITE) {
			kept += (uint32_t)__popc(bits);
			continue;
		}
		uint32_t tile_total;
		uint32_t d = base + block_prefix((uint32_t)__popc(bits), red, tile_total);
		while (bits) {
			const uint32_t line = w * 32 + (uint32_t)__ffs((int)bits) - 1;
			bits &= bits - 1;
			if (d + 2 < g.cap) {
				// line j: the lead is j = 0 when there is one; start k = j - lead.  Delimiters in front: j.
				const int64_t k = (int64_t)line - lead;
				g.rel_out[1 + d] = (int32_t)line;
				g.begin_out[1 + d] = k < 0 ? (int32_t)g.origin : g.line_start[k];
				g.next_out[1 + d] = k + 1 < (int64_t)L ? g.line_start[k + 1] : (int32_t)g.end;
			}
			d++;
		}
		base += tile_total;
	}
	if (!WRITE) {
		kept = block_sum(kept, red);
		if (threadIdx.x == 0)
			g.block_counts[blockIdx.x] = (int32_t)kept;
	}
}

// ------------------------------------------------------------------ context

// The select pass's lines and flags (k_line_mark), then per line: kept iff a selected line of its text lies in
// [j - after, j + before].  Launches over the fixed grid, a block owning a run of flag words:
//   k_ctx_count   the flags become the SELECTED bits (inverted if asked, cut at the last line); per block their count
//   k_ctx_rank    rank[w] = the selected lines in front of word w
//   k_ctx_keep    a lane per line: the line's text [lo, hi) in lines by two searches (no segments: every line), the
//                 window clamped to it, kept iff the rank difference over the window is > 0; head = kept and (first
//                 line of its text or the line in front not kept), tail likewise: a bit per line each, per block
//                 the kept lines, heads and tails
//   k_ctx_heads   the ordered write over the head bits: rel, begin, and the head's line for the next launch
//   k_ctx_tails   the same over the tail bits (group k ends at tail k): next, lines
// Nothing depends on before or after but the two clamps.
struct CtxArgs {
	SelectArgs s;
	int64_t before, after;
	const int32_t *seg_start;
	uint32_t segments;
	int32_t *lines_out, *ctx_info;
	uint32_t *rank, *head, *tail;             // per flag word
	int32_t *blk_kept, *blk_head, *blk_tail;  // per block (s.block_counts: the selected lines)
	int32_t *head_line;                       // [capacity + 1] the first line of group k
};

__device__ __forceinline__ uint32_t lower_bound_i32(const int32_t *a, uint32_t n, int64_t key)
{
	uint32_t lo = 0, hi = n;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if ((int64_t)a[mid] < key)
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo;
}

__device__ __forceinline__ uint32_t selected_word(const SelectArgs &g, uint32_t w, uint32_t lines)
{
	uint32_t bits = g.invert ? ~g.flags[w] : g.flags[w];
	const uint32_t left = lines - w * 32;   // >= 1
	if (left < 32)
		bits &= (1u << left) - 1;
	return bits;
}

__global__ __launch_bounds__(kThreads) void k_ctx_count(CtxArgs c)
{
	__shared__ uint32_t red[kWaves];
	uint32_t L, lead;
	const uint32_t lines = lines_of(c.s, L, lead);
	const Words sh = words_of((lines + 31) / 32);
	uint32_t count = 0;
	for (uint32_t w = sh.w_begin + threadIdx.x; w < sh.w_end; w += kTileWords) {
		const uint32_t bits = selected_word(c.s, w, lines);
		c.s.flags[w] = bits;
		count += (uint32_t)__popc(bits);
	}
	count = block_sum(count, red);
	if (threadIdx.x == 0)
		c.s.block_counts[blockIdx.x] = (int32_t)count;
}

__global__ __launch_bounds__(kThreads) void k_ctx_rank(CtxArgs c)
{
	__shared__ uint32_t red[2 * kWaves];
	uint32_t L, lead;
	const uint32_t lines = lines_of(c.s, L, lead);
	const Words sh = words_of((lines + 31) / 32);
	uint32_t total;
	uint32_t base = blocks_before(c.s.block_counts, red, total);
	for (uint32_t w0 = sh.w_begin; w0 < sh.w_end; w0 += kTileWords) {
		const uint32_t w = w0 + threadIdx.x;
		const uint32_t cnt = w < sh.w_end ? (uint32_t)__popc(c.s.flags[w]) : 0;
		uint32_t tile_total;
		const uint32_t r = base + block_prefix(cnt, red, tile_total);
		if (w < sh.w_end)
			c.rank[w] = r;
		base += tile_total;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0)
		c.ctx_info[0] = (int32_t)total;
}

// selected lines in front of line x <= lines
__device__ __forceinline__ uint32_t selected_before(const CtxArgs &c, uint32_t x, uint32_t lines)
{
	if (x >= lines) {   // behind the last word's bits
		if (lines == 0)
			return 0;
		const uint32_t w = (lines - 1) >> 5;
		return c.rank[w] + (uint32_t)__popc(c.s.flags[w]);
	}
	const uint32_t w = x >> 5, b = x & 31;
	return c.rank[w] + (uint32_t)__popc(c.s.flags[w] & ((1u << b) - 1));
}

struct LineCtx {
	bool kept;
	uint32_t lo, hi;   // the lines of the line's text: [lo, hi)
};

// line j < lines
__device__ __forceinline__ LineCtx line_ctx(const CtxArgs &c, uint32_t j, uint32_t lines, uint32_t L, uint32_t lead)
{
	LineCtx r{ false, 0, lines };
	if (c.segments) {
		const int64_t first = j < lead ? c.s.origin : (int64_t)c.s.line_start[j - lead];
		const uint32_t t = upper_bound_i32(c.seg_start, c.segments, first);
		if (t > 0) {
			const int64_t x = c.seg_start[t - 1];
			r.lo = lead && c.s.origin >= x ? 0 : lead + lower_bound_i32(c.s.line_start, L, x);
		}
		if (t < c.segments)
			r.hi = lead + lower_bound_i32(c.s.line_start, L, (int64_t)c.seg_start[t]);
	}
	const int64_t a = max((int64_t)r.lo, (int64_t)j - c.after), b = min((int64_t)r.hi - 1, (int64_t)j + c.before);
	r.kept = selected_before(c, (uint32_t)b + 1, lines) > selected_before(c, (uint32_t)a, lines);
	return r;
}

__global__ __launch_bounds__(kThreads) void k_ctx_keep(CtxArgs c)
{
	__shared__ uint32_t red[kWaves];
	uint32_t L, lead;
	const uint32_t lines = lines_of(c.s, L, lead);
	const uint32_t words = (lines + 31) / 32;
	const Words sh = words_of(words);
	const uint32_t lane = lane_id();
	uint32_t kept = 0, heads = 0, tails = 0;   // (counted by lane 0 of every wave)
	const uint64_t j_end = min((uint64_t)sh.w_end * 32, (uint64_t)lines);
	for (uint64_t j0 = (uint64_t)sh.w_begin * 32; j0 < j_end; j0 += kThreads) {
		const uint64_t jj = j0 + threadIdx.x;
		const bool valid = jj < j_end;
		const uint32_t j = (uint32_t)jj;
		LineCtx x{ false, 0, 0 };
		if (valid)
			x = line_ctx(c, j, lines, L, lead);
		// the neighbours: the lanes beside this one, but for a wave's two ends
		bool prev = __shfl_up((int)x.kept, 1, 64) != 0, next = __shfl_down((int)x.kept, 1, 64) != 0;
		if (lane == 0 && x.kept && j > x.lo)
			prev = line_ctx(c, j - 1, lines, L, lead).kept;
		if (lane == 63 && x.kept && j + 1 < x.hi)
			next = line_ctx(c, j + 1, lines, L, lead).kept;
		const bool head = x.kept && (j == x.lo || !prev), tail = x.kept && (j + 1 == x.hi || !next);
		const uint64_t kb = __ballot(x.kept), hb = __ballot(head), tb = __ballot(tail);
		const uint32_t w = (uint32_t)((j0 + (threadIdx.x & ~63u)) >> 5);   // the wave's first word
		if (lane == 0) {
			kept += (uint32_t)__popcll(kb);
			heads += (uint32_t)__popcll(hb);
			tails += (uint32_t)__popcll(tb);
			if (w < sh.w_end) {
				c.head[w] = (uint32_t)hb;
				c.tail[w] = (uint32_t)tb;
			}
			if (w + 1 < sh.w_end) {
				c.head[w + 1] = (uint32_t)(hb >> 32);
				c.tail[w + 1] = (uint32_t)(tb >> 32);
			}
		}
	}
	kept = block_sum(kept, red);
	heads = block_sum(heads, red);
	tails = block_sum(tails, red);
	if (threadIdx.x == 0) {
		c.blk_kept[blockIdx.x] = (int32_t)kept;
		c.blk_head[blockIdx.x] = (int32_t)heads;
		c.blk_tail[blockIdx.x] = (int32_t)tails;
	}
}

template <bool TAILS>
__global__ __launch_bounds__(kThreads) void k_ctx_write(CtxArgs c)
{
	__shared__ uint32_t red[2 * kWaves];
	const SelectArgs &g = c.s;
	uint32_t L, lead;
	const uint32_t lines = lines_of(g, L, lead);
	const Words sh = words_of((lines + 31) / 32);
	uint32_t total;
	uint32_t base = blocks_before(TAILS ? c.blk_tail : c.blk_head, red, total);
	if (!TAILS) {
		uint32_t kept_all;
		blocks_before(c.blk_kept, red, kept_all);
		if (blockIdx.x == 0 && threadIdx.x == 0) {
			write_ends(g.rel_out, g.cap, total, 0);
			write_ends(g.begin_out, g.cap, total, 0);
			c.ctx_info[1] = (int32_t)kept_all;
			c.ctx_info[2] = (int32_t)total;
			c.ctx_info[3] = 0;
		}
	} else if (blockIdx.x == 0 && threadIdx.x == 0) {
		write_ends(g.next_out, g.cap, total, 0);
		if (c.lines_out)
			write_ends(c.lines_out, g.cap, total, 0);
	}
	const uint32_t *plane = TAILS ? c.tail : c.head;
	for (uint32_t w0 = sh.w_begin; w0 < sh.w_end; w0 += kTileWords) {
		const uint32_t w = w0 + threadIdx.x;
		uint32_t bits = w < sh.w_end ? plane[w] : 0;
		uint32_t tile_total;
		uint32_t d = base + block_prefix((uint32_t)__popc(bits), red, tile_total);
		while (bits) {
			const uint32_t line = w * 32 + (uint32_t)__ffs((int)bits) - 1;
			bits &= bits - 1;
			const int64_t k = (int64_t)line - lead;
			if (!TAILS) {
				c.head_line[d] = (int32_t)line;   // (d < lines <= capacity + 1)
				if (d + 2 < g.cap) {
					g.rel_out[1 + d] = (int32_t)line;
					g.begin_out[1 + d] = k < 0 ? (int32_t)g.origin : g.line_start[k];
				}
			} else if (d + 2 < g.cap) {
				g.next_out[1 + d] = k + 1 < (int64_t)L ? g.line_start[k + 1] : (int32_t)g.end;
				if (c.lines_out)
					c.lines_out[1 + d] = (int32_t)(line - (uint32_t)c.head_line[d] + 1);
			}
			d++;
		}
		base += tile_total;
	}
}

size_t flag_bytes(size_t capacity) { return round256((capacity / 32 + 1) * 4); }

struct CtxLayout {
	size_t flags, rank, head, tail, blk_kept, blk_head, blk_tail, head_line, total;
};

CtxLayout ctx_layout(size_t capacity)
{
	CtxLayout l;
	size_t at = kCountBytes;   // the selected lines per block, as in the select pass
	auto take = [&](size_t bytes) {
		const size_t here = at;
		at += round256(bytes);
		return here;
	};
	l.flags = take(flag_bytes(capacity));
	l.rank = take(flag_bytes(capacity));
	l.head = take(flag_bytes(capacity));
	l.tail = take(flag_bytes(capacity));
	l.blk_kept = take(kCountBytes);
	l.blk_head = take(kCountBytes);
	l.blk_tail = take(kCountBytes);
	l.head_line = take((capacity + 1) * 4);
	l.total = at;
	return l;
}

// ---- the per-line form: one entry per KEPT line (acm_line_context_lines_async) ----
// k_line_mark, k_ctx_count and k_ctx_rank as above, then
//   k_ctx_keep_lines    k_ctx_keep's lane per line, leaving the KEPT bits and the head bits as planes; per block the
//                       kept lines and the heads
//   k_ctx_lines_write   the ordered write over the kept bits: rel, begin, next, and the kind from the SELECTED and the
//                       head bit of the line
struct CtxLinesArgs {
	CtxArgs c;
	uint32_t *kept;      // per flag word
	int32_t *kind_out;
};

__global__ __launch_bounds__(kThreads) void k_ctx_keep_lines(CtxLinesArgs a)
{
	__shared__ uint32_t red[kWaves];
	const CtxArgs &c = a.c;
	uint32_t L, lead;
	const uint32_t lines = lines_of(c.s, L, lead);
	const uint32_t words = (lines + 31) / 32;
	const Words sh = words_of(words);
	const uint32_t lane = lane_id();
	uint32_t kept = 0, heads = 0;   // (counted by lane 0 of every wave)
	const uint64_t j_end = min((uint64_t)sh.w_end * 32, (uint64_t)lines);
	for (uint64_t j0 = (uint64_t)sh.w_begin * 32; j0 < j_end; j0 += kThreads) {
		const uint64_t jj = j0 + threadIdx.x;
		const uint32_t j = (uint32_t)jj;
		LineCtx x{ false, 0, 0 };
		if (jj < j_end)
			x = line_ctx(c, j, lines, L, lead);
		bool prev = __shfl_up((int)x.kept, 1, 64) != 0;   // the lane in front, but for a wave's first
		if (lane == 0 && x.kept && j > x.lo)
			prev = line_ctx(c, j - 1, lines, L, lead).kept;
		const bool head = x.kept && (j == x.lo || !prev);
		const uint64_t kb = __ballot(x.kept), hb = __ballot(head);
		const uint32_t w = (uint32_t)((j0 + (threadIdx.x & ~63u)) >> 5);   // the wave's first word
		if (lane == 0) {
			kept += (uint32_t)__popcll(kb);
			heads += (uint32_t)__popcll(hb);
			if (w < sh.w_end) {
				a.kept[w] = (uint32_t)kb;
				c.head[w] = (uint32_t)hb;
			}
			if (w + 1 < sh.w_end) {
				a.kept[w + 1] = (uint32_t)(kb >> 32);
				c.head[w + 1] = (uint32_t)(hb >> 32);
			}
		}
	}
	kept = block_sum(kept, red);
	heads = block_sum(heads, red);
	if (threadIdx.x == 0) {
		c.blk_kept[blockIdx.x] = (int32_t)kept;
		c.blk_head[blockIdx.x] = (int32_t)heads;
	}
}

__global__ __launch_bounds__(kThreads) void k_ctx_lines_write(CtxLinesArgs a)
{
	__shared__ uint32_t red[2 * kWaves];
	const CtxArgs &c = a.c;
	const SelectArgs &g = c.s;
	uint32_t L, lead;
	const uint32_t lines = lines_of(g, L, lead);
	const Words sh = words_of((lines + 31) / 32);
	uint32_t total, groups;
	blocks_before(c.blk_head, red, groups);
	uint32_t base = blocks_before(c.blk_kept, red, total);
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		write_ends(g.rel_out, g.cap, total, 0);
		write_ends(g.begin_out, g.cap, total, 0);
		write_ends(g.next_out, g.cap, total, 0);
		write_ends(a.kind_out, g.cap, total, 0);
		c.ctx_info[1] = (int32_t)total;
		c.ctx_info[2] = (int32_t)groups;
		c.ctx_info[3] = 0;
	}
	for (uint32_t w0 = sh.w_begin; w0 < sh.w_end; w0 += kTileWords) {
		const uint32_t w = w0 + threadIdx.x;
		uint32_t bits = 0, hbits = 0, sbits = 0;
		if (w < sh.w_end) {
			bits = a.kept[w];
			hbits = c.head[w];
			sbits = g.flags[w];
		}
		uint32_t tile_total;
		uint32_t d = base + block_prefix((uint32_t)__popc(bits), red, tile_total);
		while (bits) {
			const uint32_t b = (uint32_t)__ffs((int)bits) - 1;
			const uint32_t line = w * 32 + b;
			bits &= bits - 1;
			if (d + 2 < g.cap) {
				const int64_t k = (int64_t)line - lead;
				g.rel_out[1 + d] = (int32_t)line;
				g.begin_out[1 + d] = k < 0 ? (int32_t)g.origin : g.line_start[k];
				g.next_out[1 + d] = k + 1 < (int64_t)L ? g.line_start[k + 1] : (int32_t)g.end;
				a.kind_out[1 + d] = (int32_t)(((sbits >> b) & 1) * ACM_LINE_SELECTED | ((hbits >> b) & 1) * ACM_LINE_GROUP_HEAD);
			}
			d++;
		}
		base += tile_total;
	}
}

struct CtxLinesLayout {
	size_t flags, rank, head, kept, blk_kept, blk_head, total;
};

CtxLinesLayout ctx_lines_layout(size_t capacity)
{
	CtxLinesLayout l;
	size_t at = kCountBytes;   // the selected lines per block, as in the select pass
	auto take = [&](size_t bytes) {
		const size_t here = at;
		at += round256(bytes);
		return here;
	};
	l.flags = take(flag_bytes(capacity));
	l.rank = take(flag_bytes(capacity));
	l.head = take(flag_bytes(capacity));
	l.kept = take(flag_bytes(capacity));
	l.blk_kept = take(kCountBytes);
	l.blk_head = take(kCountBytes);
	l.total = at;
	return l;
}

size_t mask_words(size_t n) { return ((n + 15) / 16 + 3) / 4; }

// blocks of the fixed grid: four per CU of the current device, kMaxBlocks at most
int fixed_grid(uint32_t *blocks)
{
	static thread_local int cached_dev = -1;
	static thread_local uint32_t cached = 0;
	int dev = 0;
	ACM_HIP_TRY(hipGetDevice(&dev));
	if (dev != cached_dev) {
		int cus = 0;
		ACM_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
		cached = (uint32_t)std::max(1, std::min<int>(cus * 4, (int)kMaxBlocks));
		cached_dev = dev;
	}
	*blocks = cached;
	return ACM_OK;
}

}  // namespace

extern "C" size_t acm_line_index_workspace_bytes(size_t max_text)
{
	return round256(kCountBytes + mask_words(max_text) * 8);
}

extern "C" int acm_line_index_async(const void *d_text, size_t n, long text_origin, int delimiter, int prev_byte,
    const int32_t *d_prev_info, int32_t *d_line_start, size_t capacity, int32_t *d_info, void *d_workspace,
    size_t workspace_bytes, void *stream)
{
	if (!d_line_start || !d_info || capacity == 0 || capacity > 0xFFFFFFFFul || (n && !d_text) ||
	    ((uintptr_t)d_text & 15) || n > 0x7FFFFFFFul - 16 || delimiter < 0 || delimiter > 255 || prev_byte < -1 ||
	    prev_byte > 255 || d_prev_info == d_info)
		return acm::fail(ACM_ERR_ARG, "acm_line_index_async: bad arguments");
	if (!d_workspace || workspace_bytes < acm_line_index_workspace_bytes(n))
		return acm::fail(ACM_ERR_ARG, "acm_line_index_async: workspace %zu B < required %zu B", workspace_bytes,
		    acm_line_index_workspace_bytes(n));
	hipStream_t s = (hipStream_t)stream;
	uint32_t blocks = 0;
	if (int rc = fixed_grid(&blocks))
		return rc;
	IndexArgs g;
	g.text = (const uint4 *)d_text;
	g.n = (uint32_t)n;
	g.groups = (uint32_t)((n + 15) / 16);
	g.words = (uint32_t)mask_words(n);
	g.origin = (int64_t)text_origin;
	g.delim = (uint32_t)delimiter;
	g.prev_byte = prev_byte;
	g.prev_info = d_prev_info;
	g.line_start = d_line_start;
	g.capacity = (uint32_t)capacity;
	g.info = d_info;
	g.block_counts = (int32_t *)d_workspace;
	g.mask16 = (uint16_t *)((char *)d_workspace + kCountBytes);
	hipLaunchKernelGGL(k_line_mask, dim3(blocks), dim3(kThreads), 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_line_write, dim3(blocks), dim3(kThreads), 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}

extern "C" int acm_line_number_async(const int32_t *d_line_start, size_t capacity, const int32_t *d_info,
    const int32_t *d_offsets, const int32_t *d_count, size_t count, int32_t *d_line_out, void *stream)
{
	if (!d_line_start || !d_info || !d_offsets || !d_line_out || capacity == 0 || capacity > 0xFFFFFFFFul ||
	    count > 0x7FFFFFFFul)
		return acm::fail(ACM_ERR_ARG, "acm_line_number_async: bad arguments");
	if (count == 0)
		return ACM_OK;
	uint32_t blocks = 0;
	if (int rc = fixed_grid(&blocks))
		return rc;
	blocks = (uint32_t)std::min<size_t>(blocks, (count + kThreads - 1) / kThreads);
	hipLaunchKernelGGL(k_line_number, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, d_line_start, (uint32_t)capacity,
	    d_info, d_offsets, d_count, (uint32_t)count, d_line_out);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}

extern "C" size_t acm_line_select_workspace_bytes(size_t capacity)
{
	return round256(kCountBytes + (capacity / 32 + 1) * 4);   // a bit per start and one for the lead
}

extern "C" int acm_line_select_async(const int32_t *d_line_start, size_t capacity, const int32_t *d_info, long text_origin,
    long text_end, const int32_t *d_off_plane, size_t max_records, int invert, int32_t *d_rel_out, int32_t *d_begin_out,
    int32_t *d_next_out, size_t out_capacity, void *d_workspace, size_t workspace_bytes, void *stream)
{
	if (!d_line_start || !d_info || !d_off_plane || !d_rel_out || !d_begin_out || !d_next_out || capacity == 0 ||
	    capacity > 0xFFFFFFFEul || out_capacity < 2 || max_records > 0x7FFFFFFEul || text_end < text_origin)
		return acm::fail(ACM_ERR_ARG, "acm_line_select_async: bad arguments");
	if (!d_workspace || workspace_bytes < acm_line_select_workspace_bytes(capacity))
		return acm::fail(ACM_ERR_ARG, "acm_line_select_async: workspace %zu B < required %zu B", workspace_bytes,
		    acm_line_select_workspace_bytes(capacity));
	hipStream_t s = (hipStream_t)stream;
	uint32_t blocks = 0;
	if (int rc = fixed_grid(&blocks))
		return rc;
	SelectArgs g;
	g.line_start = d_line_start;
	g.capacity = (uint32_t)capacity;
	g.info = d_info;
	g.origin = (int64_t)text_origin;
	g.end = (int64_t)text_end;
	g.off_plane = d_off_plane;
	g.max_records = (uint32_t)max_records;
	g.invert = invert ? 1 : 0;
	g.rel_out = d_rel_out;
	g.begin_out = d_begin_out;
	g.next_out = d_next_out;
	g.cap = clamp_cap(out_capacity);
	g.block_counts = (int32_t *)d_workspace;
	g.flags = (uint32_t *)((char *)d_workspace + kCountBytes);
	ACM_HIP_TRY(hipMemsetAsync(g.flags, 0, (capacity / 32 + 1) * 4, s));
	const uint32_t mark_blocks = (uint32_t)std::max<size_t>(1, std::min<size_t>(blocks, (max_records + kThreads - 1) / kThreads));
	hipLaunchKernelGGL(k_line_mark, dim3(mark_blocks), dim3(kThreads), 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_line_select<false>, dim3(blocks), dim3(kThreads), 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_line_select<true>, dim3(blocks), dim3(kThreads), 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}

extern "C" size_t acm_line_context_workspace_bytes(size_t capacity, size_t segments)
{
	(void)segments;   // (the starts are searched where they lie)
	return ctx_layout(capacity).total;
}

extern "C" int acm_line_context_async(const int32_t *d_line_start, size_t capacity, const int32_t *d_info, long text_origin,
    long text_end, const int32_t *d_off_plane, size_t max_records, int invert, int before, int after, const int32_t *d_seg_start,
    size_t segments, int32_t *d_rel_out, int32_t *d_begin_out, int32_t *d_next_out, int32_t *d_lines_out, size_t out_capacity,
    int32_t *d_ctx_info, void *d_workspace, size_t workspace_bytes, void *stream)
{
	if (!d_line_start || !d_info || !d_off_plane || !d_rel_out || !d_begin_out || !d_next_out || !d_ctx_info || capacity == 0 ||
	    capacity > 0xFFFFFFFEul || out_capacity < 2 || max_records > 0x7FFFFFFEul || text_end < text_origin || before < 0 ||
	    after < 0 || segments > 0x7FFFFFFFul || (segments > 0) != (d_seg_start != nullptr))
		return acm::fail(ACM_ERR_ARG, "acm_line_context_async: bad arguments");
	const CtxLayout l = ctx_layout(capacity);
	if (!d_workspace || workspace_bytes < l.total)
		return acm::fail(ACM_ERR_ARG, "acm_line_context_async: workspace %zu B < required %zu B", workspace_bytes, l.total);
	hipStream_t s = (hipStream_t)stream;
	uint32_t blocks = 0;
	if (int rc = fixed_grid(&blocks))
		return rc;
	char *ws = (char *)d_workspace;
	CtxArgs c;
	SelectArgs &g = c.s;
	g.line_start = d_line_start;
	g.capacity = (uint32_t)capacity;
	g.info = d_info;
	g.origin = (int64_t)text_origin;
	g.end = (int64_t)text_end;
	g.off_plane = d_off_plane;
	g.max_records = (uint32_t)max_records;
	g.invert = invert ? 1 : 0;
	g.rel_out = d_rel_out;
	g.begin_out = d_begin_out;
	g.next_out = d_next_out;
	g.cap = clamp_cap(out_capacity);
	g.block_counts = (int32_t *)ws;
	g.flags = (uint32_t *)(ws + l.flags);
	c.before = before;
	c.after = after;
	c.seg_start = d_seg_start;
	c.segments = (uint32_t)segments;
	c.lines_out = d_lines_out;
	c.ctx_info = d_ctx_info;
	c.rank = (uint32_t *)(ws + l.rank);
	c.head = (uint32_t *)(ws + l.head);
	c.tail = (uint32_t *)(ws + l.tail);
	c.blk_kept = (int32_t *)(ws + l.blk_kept);
	c.blk_head = (int32_t *)(ws + l.blk_head);
	c.blk_tail = (int32_t *)(ws + l.blk_tail);
	c.head_line = (int32_t *)(ws + l.head_line);
	ACM_HIP_TRY(hipMemsetAsync(g.flags, 0, (capacity / 32 + 1) * 4, s));
	const uint32_t mark_blocks = (uint32_t)std::max<size_t>(1, std::min<size_t>(blocks, (max_records + kThreads - 1) / kThreads));
	hipLaunchKernelGGL(k_line_mark, dim3(mark_blocks), dim3(kThreads), 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_ctx_count, dim3(blocks), dim3(kThreads), 0, s, c);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_ctx_rank, dim3(blocks), dim3(kThreads), 0, s, c);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_ctx_keep, dim3(blocks), dim3(kThreads), 0, s, c);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_ctx_write<false>, dim3(blocks), dim3(kThreads), 0, s, c);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_ctx_write<true>, dim3(blocks), dim3(kThreads), 0, s, c);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}

extern "C" size_t acm_line_context_lines_workspace_bytes(size_t capacity, size_t segments)
{
	(void)segments;   // (the starts are searched where they lie)
	return ctx_lines_layout(capacity).total;
}

extern "C" int acm_line_context_lines_async(const int32_t *d_line_start, size_t capacity, const int32_t *d_info, long text_origin,
    long text_end, const int32_t *d_off_plane, size_t max_records, int invert, int before, int after, const int32_t *d_seg_start,
    size_t segments, int32_t *d_rel_out, int32_t *d_begin_out, int32_t *d_next_out, int32_t *d_kind_out, size_t out_capacity,
    int32_t *d_ctx_info, void *d_workspace, size_t workspace_bytes, void *stream)
{
	if (!d_line_start || !d_info || !d_off_plane || !d_rel_out || !d_begin_out || !d_next_out || !d_kind_out || !d_ctx_info ||
	    capacity == 0 || capacity > 0xFFFFFFFEul || out_capacity < 2 || max_records > 0x7FFFFFFEul || text_end < text_origin ||
	    before < 0 || after < 0 || segments > 0x7FFFFFFFul || (segments > 0) != (d_seg_start != nullptr))
		return acm::fail(ACM_ERR_ARG, "acm_line_context_lines_async: bad arguments");
	const CtxLinesLayout l = ctx_lines_layout(capacity);
	if (!d_workspace || workspace_bytes < l.total)
		return acm::fail(ACM_ERR_ARG, "acm_line_context_lines_async: workspace %zu B < required %zu B", workspace_bytes, l.total);
	hipStream_t s = (hipStream_t)stream;
	uint32_t blocks = 0;
	if (int rc = fixed_grid(&blocks))
		return rc;
	char *ws = (char *)d_workspace;
	CtxLinesArgs a{};
	CtxArgs &c = a.c;
	SelectArgs &g = c.s;
	g.line_start = d_line_start;
	g.capacity = (uint32_t)capacity;
	g.info = d_info;
	g.origin = (int64_t)text_origin;
	g.end = (int64_t)text_end;
	g.off_plane = d_off_plane;
	g.max_records = (uint32_t)max_records;
	g.invert = invert ? 1 : 0;
	g.rel_out = d_rel_out;
	g.begin_out = d_begin_out;
	g.next_out = d_next_out;
	g.cap = clamp_cap(out_capacity);
	g.block_counts = (int32_t *)ws;
	g.flags = (uint32_t *)(ws + l.flags);
	c.before = before;
	c.after = after;
	c.seg_start = d_seg_start;
	c.segments = (uint32_t)segments;
	c.ctx_info = d_ctx_info;
	c.rank = (uint32_t *)(ws + l.rank);
	c.head = (uint32_t *)(ws + l.head);
	c.blk_kept = (int32_t *)(ws + l.blk_kept);
	c.blk_head = (int32_t *)(ws + l.blk_head);
	a.kept = (uint32_t *)(ws + l.kept);
	a.kind_out = d_kind_out;
	ACM_HIP_TRY(hipMemsetAsync(g.flags, 0, (capacity / 32 + 1) * 4, s));
	const uint32_t mark_blocks = (uint32_t)std::max<size_t>(1, std::min<size_t>(blocks, (max_records + kThreads - 1) / kThreads));
	hipLaunchKernelGGL(k_line_mark, dim3(mark_blocks), dim3(kThreads), 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_ctx_count, dim3(blocks), dim3(kThreads), 0, s, c);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_ctx_rank, dim3(blocks), dim3(kThreads), 0, s, c);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_ctx_keep_lines, dim3(blocks), dim3(kThreads), 0, s, a);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_ctx_lines_write, dim3(blocks), dim3(kThreads), 0, s, a);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}
