// Match rewriting: the text with every selected match replaced, masked or deleted.  gfx950 only.  DESIGN.md 6p.
//
// A record (p, o) spans [s, e] as in the select pass (select.hip).  It is USED iff p is a pattern index, L >= 1 and
// text_origin <= s <= e < text_end; src = e - s + 1 bytes of the text become dst bytes of output: the pattern's
// replacement, its fill byte src times, or (no replacement) the span itself.  Launches:
//   k_rw_sum     the record-pass grid (record_pass.h) over max_records cells: per block the used and skipped
//                records, the sum of dst - src and of src, in 64 bits
//   k_rw_place   the same grid: a block sums the blocks in front of its own, ranks its records in input order and
//                writes the used ones densely: rec_end[r] = the output offset behind record r's replacement (int64),
//                rec[r] = {s - text_origin, src, dst, p}; d_at_out; block 0 writes d_info and hdr = {used, m}
//   k_rw_seg     (segments > 0) a thread per start: a binary search on rec[].s
//   k_rw_copy    (out_capacity > 0) a workgroup per kTileBytes of OUTPUT.  r0 = the first record whose rec_end lies
//                behind the tile's first byte, found by the wave 64 samples a step.  Searching the ENDS is what
//                keeps a tile from visiting records it owes no byte to: any number of deletions may sit on one
//                output offset, and all of them end at or in front of it.  A tile that no record begins in is one
//                gap: every 16-byte piece is an aligned store of source bytes at one byte shift.  Otherwise every
//                thread finds the record of its piece's first byte in [r0, the first record that ends behind the
//                tile]; a piece inside one gap streams as before, a piece that touches a record is put together
//                byte by byte in registers (gap bytes, replacement bytes from the blob, the fill byte) and stored
//                whole; only the piece that min(m, out_capacity) cuts is stored byte by byte.
// A tile's work is its bytes and a search per piece: bounded by log2(records) a byte whatever the planes hold.
// Planes that did not come from select (spans that overlap or descend) make rec_end unsorted: the searches then
// return some index in range, every source offset is tested against [0, n) before it is read, and every replacement
// index against dst.  No atomics; no read-modify-write of d_out.
#include <hip/hip_runtime.h>

#include "acm_internal.h"
#include "device_dfa.h"
#include "place64.h"
#include "record_pass.h"

namespace {

using namespace acm_rp;

constexpr int kPieces = kTileBytes / 16 / kThreads;           // 16-byte pieces per thread: 4
// the source of a streamed piece: two aligned 16-byte loads and a byte align, or (the other form measured in DESIGN.md
// 6p, kept buildable with -DACM_REWRITE_UNALIGNED_SOURCE) one unaligned 16-byte load
#ifdef ACM_REWRITE_UNALIGNED_SOURCE
constexpr bool kUnalignedSource = true;
#else
constexpr bool kUnalignedSource = false;
#endif

struct RwArgs {
	const int32_t *pat_plane, *off_plane;   // the input: [0] the count, then the records
	uint32_t R;                             // max_records
	const uint8_t *text;
	uint32_t n;
	int64_t origin;
	const uint32_t *pat_len;                // [patterns]
	const int4 *wild_ent;                   // [patterns] {cell index, pre, post, length}; null: a set without contexts
	uint32_t num_patterns;
	const int4 *repl_ent;                   // [patterns] {kind, bytes, first byte in the blob, fill byte}; null: no replacements
	const uint8_t *repl_blob;
	// workspace
	uint32_t *blk_used, *blk_skip;          // [gridDim.x of the record grid]
	int64_t *blk_delta, *blk_src;
	int64_t *hdr;                           // {used records, m}
	int64_t *rec_end;                       // [R] per used record, in input order: the output offset behind its replacement
	int4 *rec;                              // [R] {s - origin, src, dst, pattern}
	// output
	uint8_t *out;
	uint32_t cap;
	int32_t *at_out;
	uint32_t at_cap;
	const int32_t *seg_start;
	uint32_t segments;
	int32_t *seg_out;
	int32_t *info;
};

struct Ev {
	bool used;
	int32_t s, src, dst, pat;
};

__device__ __forceinline__ uint32_t records_of(const RwArgs &g) { return min((uint32_t)g.pat_plane[0], g.R); }

// record i < the count
__device__ __forceinline__ Ev eval(const RwArgs &g, uint32_t i)
{
	Ev v{ false, 0, 0, 0, 0 };
	const uint32_t p = (uint32_t)g.pat_plane[1 + i];
	const int32_t o = g.off_plane[1 + i];
	const Span sp = span_of(g.pat_len, g.wild_ent, g.num_patterns, p, o);   // (the select pass's span: record_pass.h)
	const int64_t s = sp.s, e = sp.e;
	if (!sp.ok || s < g.origin || s > e || e >= g.origin + (int64_t)g.n)
		return v;
	v.used = true;
	v.s = (int32_t)(s - g.origin);   // in [0, n)
	v.src = (int32_t)(e - s + 1);    // in [1, n]
	v.dst = v.src;
	v.pat = (int32_t)p;
	if (g.repl_ent) {
		const int4 r = g.repl_ent[p];
		if (r.x == acm::kReplBytes)
			v.dst = r.y;
	}
	return v;
}

__global__ __launch_bounds__(kThreads) void k_rw_sum(RwArgs g)
{
	__shared__ uint32_t red[kWaves];
	__shared__ int64_t red64[kWaves];

	const uint32_t tid = threadIdx.x;
	const uint32_t m = records_of(g);
	const Share sh = share_of((g.R + kTile - 1) / kTile);
	uint32_t used = 0, skip = 0;
	int64_t delta = 0, src = 0;
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++)
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t i = t * kTile + q * kThreads + tid;
			if (i >= m)
				continue;
			const Ev v = eval(g, i);
			used += v.used ? 1 : 0;
			skip += v.used ? 0 : 1;
			delta += (int64_t)v.dst - v.src;
			src += v.src;
		}
	used = block_sum(used, red);
	skip = block_sum(skip, red);
	delta = block_sum64(delta, red64);
	src = block_sum64(src, red64);
	if (tid == 0) {
		g.blk_used[blockIdx.x] = used;
		g.blk_skip[blockIdx.x] = skip;
		g.blk_delta[blockIdx.x] = delta;
		g.blk_src[blockIdx.x] = src;
	}
}

__global__ __launch_bounds__(kThreads) void k_rw_place(RwArgs g)
{
	__shared__ uint32_t red[kWaves];
	__shared__ int64_t red64[kWaves];

	const uint32_t tid = threadIdx.x;
	const uint32_t m = records_of(g);
	uint32_t used_before = 0, used_all = 0, skip_all = 0;
	int64_t delta_before = 0, delta_all = 0, src_all = 0;
	for (uint32_t j = tid; j < gridDim.x; j += kThreads) {
		const uint32_t u = g.blk_used[j];
		const int64_t d = g.blk_delta[j];
		used_all += u;
		delta_all += d;
		skip_all += g.blk_skip[j];
		src_all += g.blk_src[j];
		if (j < blockIdx.x) {
			used_before += u;
			delta_before += d;
		}
	}
	used_before = block_sum(used_before, red);
	used_all = block_sum(used_all, red);
	skip_all = block_sum(skip_all, red);
	delta_before = block_sum64(delta_before, red64);
	delta_all = block_sum64(delta_all, red64);
	src_all = block_sum64(src_all, red64);

	// a tile in input order: thread tid has its records [tid * kPer, tid * kPer + kPer)
	const Share sh = share_of((g.R + kTile - 1) / kTile);
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++) {
		Ev ev[kPer];
		uint32_t c = 0;
		int64_t dl = 0;
#pragma unroll
		for (int k = 0; k < kPer; k++) {
			const uint32_t i = t * kTile + tid * kPer + k;
			ev[k] = Ev{ false, 0, 0, 0, 0 };
			if (i < m)
				ev[k] = eval(g, i);
			c += ev[k].used ? 1 : 0;
			dl += (int64_t)ev[k].dst - ev[k].src;
		}
		uint32_t tile_c;
		int64_t tile_d;
		uint32_t rank = used_before + block_prefix(c, red, tile_c);   // (< m <= R: a used record per input record at most)
		int64_t dacc = delta_before + block_prefix64(dl, red64, tile_d);
#pragma unroll
		for (int k = 0; k < kPer; k++)
			if (ev[k].used) {
				const int64_t begin = (int64_t)ev[k].s + dacc;
				g.rec_end[rank] = begin + ev[k].dst;
				g.rec[rank] = make_int4(ev[k].s, ev[k].src, ev[k].dst, ev[k].pat);
				if (g.at_out && (uint64_t)rank + 2 < g.at_cap)
					g.at_out[1 + rank] = sat32(begin);
				rank++;
				dacc += (int64_t)ev[k].dst - ev[k].src;
			}
		used_before += tile_c;
		delta_before += tile_d;
	}
	if (blockIdx.x == 0 && tid == 0) {
		const int64_t total = (int64_t)g.n + delta_all;
		g.hdr[0] = used_all;
		g.hdr[1] = total;
		g.info[0] = (int32_t)used_all;
		g.info[1] = (int32_t)skip_all;
		g.info[2] = (int32_t)(uint32_t)((uint64_t)total & 0xFFFFFFFFu);
		g.info[3] = (int32_t)(total >> 32);
		g.info[4] = (int32_t)(uint32_t)((uint64_t)src_all & 0xFFFFFFFFu);
		g.info[5] = (int32_t)(src_all >> 32);
		g.info[6] = (g.out && total > (int64_t)g.cap) ? 1 : 0;
		g.info[7] = 0;
		if (g.at_out)
			write_ends(g.at_out, g.at_cap, used_all, 0);
	}
}

// ---- where each start lies in the output ----

__global__ __launch_bounds__(kThreads) void k_rw_seg(RwArgs g)
{
	const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
	if (k >= g.segments)
		return;
	const uint32_t U = (uint32_t)min((uint64_t)g.hdr[0], (uint64_t)g.R);
	const int64_t x = max(g.origin, min((int64_t)g.seg_start[k], g.origin + (int64_t)g.n)) - g.origin;   // in [0, n]
	uint32_t lo = 0, hi = U;   // the used records with s < x
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if ((int64_t)g.rec[mid].x < x)
			lo = mid + 1;
		else
			hi = mid;
	}
	int64_t delta = 0;   // of the records in front: where the last of them ends in the output, less where it ends in the text
	if (lo > 0) {
		const int4 r = g.rec[lo - 1];
		delta = g.rec_end[lo - 1] - ((int64_t)r.x + r.y);
	}
	g.seg_out[k] = sat32(x + delta);
}

// ---- the copy ----

struct Cur {          // the record a byte is looked up in
	uint32_t r;       // U: behind the last record
	int64_t ob, oe;   // its replacement in the output: [ob, oe)
	int4 rec;
	int4 rp;          // its pattern's replacement
};

__device__ __forceinline__ void cur_load(const RwArgs &g, uint32_t U, Cur &c)
{
	if (c.r >= U)
		return;
	c.oe = g.rec_end[c.r];
	c.rec = g.rec[c.r];
	c.ob = c.oe - c.rec.z;
	c.rp = make_int4(acm::kReplNone, 0, 0, 0);
	if (g.repl_ent && (uint32_t)c.rec.w < g.num_patterns)
		c.rp = g.repl_ent[c.rec.w];
}

__device__ __forceinline__ uint32_t text_byte(const RwArgs &g, int64_t sx)
{
	return (sx >= 0 && sx < (int64_t)g.n) ? g.text[sx] : 0u;
}

// output bytes [x0, x1), x1 - x0 <= 16, x0 a multiple of 16; r: a record at or in front of the one x0 lies in
__device__ __forceinline__ void slow_piece(const RwArgs &g, uint32_t U, int64_t m, int64_t x0, int64_t x1, uint32_t r)
{
	Cur c;
	c.r = r;
	c.ob = c.oe = 0;
	cur_load(g, U, c);
	uint32_t w[4] = { 0, 0, 0, 0 };
#pragma unroll
	for (int j = 0; j < 16; j++) {
		const int64_t x = x0 + j;
		if (x >= x1)
			break;
		if (c.r < U && x >= c.oe) {   // the next record that ends behind x: mostly the next one
			uint32_t nr = c.r + 1;
			if (nr < U && g.rec_end[nr] <= x)
				nr = nr + 1 + upper_bound64(g.rec_end + nr + 1, U - nr - 1, x);
			c.r = nr;
			cur_load(g, U, c);
		}
		uint32_t b;
		if (c.r >= U) {
			b = text_byte(g, x - (m - (int64_t)g.n));   // behind the last record: the text's tail
		} else if (x < c.ob) {
			b = text_byte(g, (int64_t)c.rec.x - (c.ob - x));   // the gap in front of the record
		} else {
			const int64_t k = x - c.ob;
			if (k >= (int64_t)c.rec.z)
				b = 0;   // (planes that did not come from select)
			else if (c.rp.x == acm::kReplFill)
				b = (uint32_t)c.rp.w & 0xFF;
			else if (c.rp.x == acm::kReplBytes)
				b = k < (int64_t)c.rp.y ? g.repl_blob[(int64_t)c.rp.z + k] : 0u;
			else
				b = text_byte(g, (int64_t)c.rec.x + k);
		}
		w[j >> 2] |= b << (8 * (j & 3));
	}
	if (x1 - x0 == 16) {
		*(uint4 *)(g.out + x0) = make_uint4(w[0], w[1], w[2], w[3]);
	} else {
#pragma unroll
		for (int j = 0; j < 16; j++)
			if (x0 + j < x1)
				g.out[x0 + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
	}
}

__global__ __launch_bounds__(kThreads) void k_rw_copy(RwArgs g)
{
	const uint32_t tid = threadIdx.x;
	const uint32_t U = (uint32_t)min((uint64_t)g.hdr[0], (uint64_t)g.R);
	const int64_t m = g.hdr[1];
	const int64_t limit = m <= 0 ? 0 : min(m, (int64_t)g.cap);
	const int64_t t0 = (int64_t)blockIdx.x * kTileBytes;
	if (t0 >= limit)
		return;
	const int64_t t1 = min(t0 + (int64_t)kTileBytes, limit);
	const int64_t tail = m - (int64_t)g.n;   // output offset less source offset behind the last record

	// the first record that ends behind the tile's first byte, and whether the tile lies in the gap in front of it
	const uint32_t r0 = wave_upper_bound64(g.rec_end, U, t0);
	bool one_gap = true;
	int64_t shift = tail;
	if (r0 < U) {
		const int4 rec = g.rec[r0];
		const int64_t ob = g.rec_end[r0] - rec.z;
		one_gap = ob >= t1;
		shift = ob - rec.x;
	}
	uint32_t r_end = r0;   // one behind the records a piece of the tile can begin in
	if (!one_gap)
		r_end = min(r0 + wave_upper_bound64(g.rec_end + r0, U - r0, t1 - 1) + 1, U);

	uint4 v[kPieces];
	uint32_t rr[kPieces];
	int how[kPieces];   // 0: no piece, 1: streamed, 2: put together
#pragma unroll
	for (int q = 0; q < kPieces; q++) {
		const int64_t x0 = t0 + ((int64_t)q * kThreads + tid) * 16;
		how[q] = 0;
		rr[q] = r0;
		if (x0 >= t1)
			continue;
		how[q] = 2;
		bool gap = one_gap;
		int64_t sh = shift;
		if (!one_gap) {
			const uint32_t r = r0 + upper_bound64(g.rec_end + r0, r_end - r0, x0);
			rr[q] = r;
			gap = true;
			sh = tail;
			if (r < U) {
				const int4 rec = g.rec[r];
				const int64_t ob = g.rec_end[r] - rec.z;
				gap = ob >= x0 + 16;
				sh = ob - rec.x;
			}
		}
		const int64_t sx = x0 - sh;
		if (gap && x0 + 16 <= t1 && sx >= 0 && sx + 16 <= (int64_t)g.n) {
			how[q] = 1;
			v[q] = load_source<kUnalignedSource>(g.text, sx);
		}
	}
#pragma unroll
	for (int q = 0; q < kPieces; q++)
		if (how[q] == 1)
			*(uint4 *)(g.out + t0 + ((int64_t)q * kThreads + tid) * 16) = v[q];
#pragma unroll
	for (int q = 0; q < kPieces; q++)
		if (how[q] == 2) {
			const int64_t x0 = t0 + ((int64_t)q * kThreads + tid) * 16;
			slow_piece(g, U, m, x0, min(x0 + 16, t1), rr[q]);
		}
}

// ---- host side ----

struct Layout {
	size_t blk_used, blk_skip, blk_delta, blk_src, hdr, rec_end, rec, total;
};

Layout layout_of(size_t max_records, uint32_t blocks)
{
	Layout l;
	size_t at = 0;
	auto take = [&](size_t bytes) {
		const size_t here = at;
		at += round256(bytes);
		return here;
	};
	l.blk_used = take((size_t)blocks * sizeof(uint32_t));
	l.blk_skip = take((size_t)blocks * sizeof(uint32_t));
	l.blk_delta = take((size_t)blocks * sizeof(int64_t));
	l.blk_src = take((size_t)blocks * sizeof(int64_t));
	l.hdr = take(4 * sizeof(int64_t));
	l.rec_end = take(max_records * sizeof(int64_t));
	l.rec = take(max_records * sizeof(int4));
	l.total = at;
	return l;
}

}  // namespace

extern "C" size_t acm_rewrite_workspace_bytes(size_t max_records, size_t segments)
{
	(void)segments;   // (the starts are searched where they lie)
	return layout_of(max_records, grid_for(max_records)).total;
}

extern "C" int acm_rewrite_async(const acm_dfa *d, const void *d_text, size_t n, long text_origin,
    const int32_t *d_pat_plane, const int32_t *d_off_plane, size_t max_records, void *d_out, size_t out_capacity,
    int32_t *d_at_out, size_t at_capacity, const int32_t *d_seg_start, size_t segments, int32_t *d_seg_out, int32_t *d_info,
    void *d_workspace, size_t workspace_bytes, void *stream)
{
	if (!d || !d_pat_plane || !d_off_plane || !d_info || (!d_text && n > 0) || ((uintptr_t)d_text & 15) ||
	    ((uintptr_t)d_out & 15) || n > kMaxBytes || out_capacity > kMaxBytes || (!d_out && out_capacity > 0) ||
	    (d_at_out && at_capacity < 2) || max_records > 0x7FFFFFFEul || segments > 0x7FFFFFFFul ||
	    text_origin < (long)INT32_MIN || text_origin > (long)INT32_MAX)
		return acm::fail(ACM_ERR_ARG, "acm_rewrite_async: bad arguments");
	if ((segments > 0) != (d_seg_start != nullptr) || (segments > 0) != (d_seg_out != nullptr))
		return acm::fail(ACM_ERR_ARG, "acm_rewrite_async: segments without both arrays, or arrays without segments");
	if ((d->num_patterns && !d->d_pat_len) || (d->wild && !d->d_wild_ent) || (d->replacements && (!d->d_repl_ent || !d->d_repl_blob)))
		return acm::fail(ACM_ERR_ARG, "acm_rewrite_async: automaton without its span or replacement tables");
	const uint32_t blocks = grid_for(max_records);
	const Layout l = layout_of(max_records, blocks);
	if (!d_workspace || workspace_bytes < l.total)
		return acm::fail(ACM_ERR_ARG, "acm_rewrite_async: workspace %zu B < required %zu B", workspace_bytes, l.total);

	char *ws = (char *)d_workspace;
	RwArgs g{};
	g.pat_plane = d_pat_plane;
	g.off_plane = d_off_plane;
	g.R = (uint32_t)max_records;
	g.text = (const uint8_t *)d_text;
	g.n = (uint32_t)n;
	g.origin = (int64_t)text_origin;
	g.pat_len = d->d_pat_len;
	g.wild_ent = d->wild ? (const int4 *)d->d_wild_ent : nullptr;
	g.num_patterns = d->num_patterns;
	g.repl_ent = d->replacements ? (const int4 *)d->d_repl_ent : nullptr;
	g.repl_blob = d->d_repl_blob;
	g.blk_used = (uint32_t *)(ws + l.blk_used);
	g.blk_skip = (uint32_t *)(ws + l.blk_skip);
	g.blk_delta = (int64_t *)(ws + l.blk_delta);
	g.blk_src = (int64_t *)(ws + l.blk_src);
	g.hdr = (int64_t *)(ws + l.hdr);
	g.rec_end = (int64_t *)(ws + l.rec_end);
	g.rec = (int4 *)(ws + l.rec);
	g.out = (uint8_t *)d_out;
	g.cap = (uint32_t)out_capacity;
	g.at_out = d_at_out;
	g.at_cap = clamp_cap(at_capacity);
	g.seg_start = d_seg_start;
	g.segments = (uint32_t)segments;
	g.seg_out = d_seg_out;
	g.info = d_info;

	ACM_HIP_TRY(hipSetDevice(d->device));
	hipStream_t s = (hipStream_t)stream;
	const dim3 grid(blocks), block(kThreads);
	hipLaunchKernelGGL(k_rw_sum, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_rw_place, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	if (segments > 0) {
		hipLaunchKernelGGL(k_rw_seg, dim3((uint32_t)((segments + kThreads - 1) / kThreads)), block, 0, s, g);
		ACM_HIP_TRY(hipGetLastError());
	}
	if (out_capacity > 0) {
		hipLaunchKernelGGL(k_rw_copy, dim3((uint32_t)((out_capacity + kTileBytes - 1) / kTileBytes)), block, 0, s, g);
		ACM_HIP_TRY(hipGetLastError());
	}
	return ACM_OK;
}
