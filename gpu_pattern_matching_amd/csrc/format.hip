// Formatting extract: the extract (extract.hip) with a generated prefix in front of every range's bytes -- a name from a
// table, a line number, a byte offset, each followed by a separator that depends on the range's kind (grep -H -n -b).
// gfx950 only.  DESIGN.md 6r.
//
// Range i of the planes is used as in the extract.  A used range puts into the output, in input order: the glue (iff its
// HEAD bit is set and a used range of the same text id lies in front), the prefix, its bytes, the terminator.  Launches:
//   k_fm_sum     the record-pass grid over max_ranges cells: per block the used and skipped ranges, the output bytes
//                (without the glue in front of the block's first used range), the text bytes, the terminators, and the
//                text id (and HEAD bit) of its first and the text id of its last used range.  A part's size includes the
//                prefix: the name's length from the offset table, the digits of the two numbers from a count against
//                the powers of ten
//   k_fm_place   the same grid: block sums in front, the glue at every block's front, the used ranges written densely:
//                rng_end[r] (int64), rng[r] = {b - text_origin, bytes, prefix bytes, glue bytes | terminator << 8 |
//                selected << 9}, pre[r] = {line number, byte offset, where the name lies, its length}; d_at_out; the
//                buckets of the texts; block 0 writes d_info and hdr = {used, m}
//   k_fm_seg     (segments > 0, two launches) a 64-bit inclusive prefix over the buckets: d_seg_out
//   k_fm_copy    (out_capacity > 0) a workgroup per kTileBytes of OUTPUT, staged in LDS, the extract's copy kernel with
//                one more thing a range's thread puts into LDS: its prefix, clipped to the tile.  Digits are made from
//                the value (a division by ten each) and written backwards; the separators are single bytes; a name of
//                at most kShortName bytes is copied by the range's thread, a longer one by the 64 lanes of its wave.
//                The bytes go as in the extract: aligned 16-byte source pieces, a piece a lane, shifted to the
//                destination's dword phase in registers.  A tile inside the bytes of one range streams.
// No atomics decide an order; no read-modify-write of d_out; no byte at or behind min(m, out_capacity) is written.
#include <hip/hip_runtime.h>

#include "acm_internal.h"
#include "place64.h"
#include "record_pass.h"

namespace {

using namespace acm_rp;

constexpr uint32_t kTileBytes = 16384;   // output bytes a workgroup owns, staged in LDS
constexpr int kMaxGlue = ACM_EXTRACT_MAX_GLUE;
constexpr int32_t kMaxName = ACM_FORMAT_MAX_NAME;
constexpr int32_t kShortName = 32;       // a longer name is copied by the whole wave
constexpr int64_t kMaxBase = 1000000000000000000ll;
constexpr unsigned kKnownFlags = ACM_EXTRACT_END_INCLUSIVE | ACM_FORMAT_NAME | ACM_FORMAT_NUMBER | ACM_FORMAT_OFFSET;

__constant__ uint64_t kPow10[19] = { 1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull,
	1000000000ull, 10000000000ull, 100000000000ull, 1000000000000ull, 10000000000000ull, 100000000000000ull,
	1000000000000000ull, 10000000000000000ull, 100000000000000000ull, 1000000000000000000ull };

struct Glue {
	uint8_t b[kMaxGlue];
};

struct BlockSum {          // what k_fm_sum leaves per block
	int64_t bytes, src;    // output bytes (see above), text bytes
	uint32_t used, skip, terms;
	uint32_t first_lo, last_lo;   // the low words of the keys of the block's first and last used range (used > 0)
	uint32_t pad;
};

struct PreRec {            // what the copy kernel makes a used range's prefix from
	int64_t num, off;      // the values to print (>= 0)
	int32_t name_at, name_len;
};

struct FmArgs {
	const int32_t *begin_plane, *end_plane, *kind_plane, *num_plane, *seg_num;
	uint32_t R;
	const uint8_t *text;
	uint32_t n;
	int64_t origin;
	int inclusive;
	unsigned flags;
	int64_t number_base, offset_base;
	uint32_t sel_sep, ctx_sep;
	const uint8_t *names;
	const int32_t *name_off;
	int64_t names_bytes;
	Glue glue;
	int glue_len, term;
	const int32_t *seg_start;
	uint32_t segments;
	// workspace
	BlockSum *blk;           // [gridDim.x of the range grid]
	int64_t *hdr;            // {used ranges, m}
	int64_t *rng_end;        // [R] per used range, in input order: the output offset behind its part
	int4 *rng;               // [R] {b - origin, bytes, prefix bytes, glue bytes | terminator << 8 | selected << 9}
	PreRec *pre;             // [R]
	int64_t *bucket;         // [segments + 1] output bytes of the ranges of each text id
	int64_t *seg_blk;        // [blocks of the segment grid]
	// output
	uint8_t *out;
	uint32_t cap;
	int32_t *at_out;
	uint32_t at_cap;
	int32_t *seg_out;
	int32_t *info;
};

struct Ev {
	bool used;
	int32_t s, len, tid, term;   // term: 1 iff a terminator follows
	int32_t head, sel;           // the kind bits
	int32_t pre;                 // prefix bytes
	int32_t glue;                // glue bytes in front (set by tile_eval)
	PreRec p;
};

__device__ __forceinline__ uint32_t ranges_of(const FmArgs &g)
{
	return (uint32_t)min((int64_t)max(g.begin_plane[0], 0), (int64_t)g.R);
}

// decimal digits of v: 1..19
__device__ __forceinline__ int32_t digits_of(uint64_t v)
{
	int32_t d = 1;
#pragma unroll
	for (int k = 1; k < 19; k++)
		d += v >= kPow10[k] ? 1 : 0;
	return d;
}

// range i < the count
__device__ __forceinline__ Ev eval(const FmArgs &g, uint32_t i)
{
	Ev v{};
	const int64_t b = g.begin_plane[1 + i];
	const int64_t e = (int64_t)g.end_plane[1 + i] + g.inclusive;
	if (b < g.origin || b >= e || e > g.origin + (int64_t)g.n)
		return v;
	v.used = true;
	v.s = (int32_t)(b - g.origin);   // in [0, n)
	v.len = (int32_t)(e - b);        // in [1, n - s]
	v.tid = g.segments ? (int32_t)upper_bound_i32(g.seg_start, g.segments, b) : 0;
	v.term = g.term >= 0 && g.text[(int64_t)v.s + v.len - 1] != (uint8_t)g.term ? 1 : 0;
	const int32_t kind = g.kind_plane ? g.kind_plane[1 + i] : (int32_t)ACM_LINE_SELECTED;
	v.sel = kind & 1;
	v.head = (kind >> 1) & 1;
	if (g.flags & ACM_FORMAT_NAME) {
		const int64_t a = g.name_off[v.tid], z = g.name_off[v.tid + 1];   // (tid + 1 <= segments + 1)
		if (a >= 0 && a <= z && z <= g.names_bytes && z - a <= (int64_t)kMaxName) {
			v.p.name_at = (int32_t)a;
			v.p.name_len = (int32_t)(z - a);
		}
		v.pre += v.p.name_len + 1;
	}
	if (g.flags & ACM_FORMAT_NUMBER) {
		const int64_t first = v.tid > 0 && g.seg_num ? g.seg_num[v.tid - 1] : 0;
		v.p.num = max(g.number_base + (int64_t)g.num_plane[1 + i] - first, (int64_t)0);
		v.pre += digits_of((uint64_t)v.p.num) + 1;
	}
	if (g.flags & ACM_FORMAT_OFFSET) {
		const int64_t first = v.tid > 0 ? (int64_t)g.seg_start[v.tid - 1] : g.origin;
		v.p.off = max(g.offset_base + b - first, (int64_t)0);
		v.pre += digits_of((uint64_t)v.p.off) + 1;
	}
	return v;
}

// (cell index + 1) << 32 | HEAD << 31 | text id (< 2^31)
__device__ __forceinline__ int64_t key_of(uint32_t i, const Ev &v)
{
	return (int64_t)((uint64_t)(i + 1) << 32 | (uint32_t)v.head << 31 | (uint32_t)v.tid);
}

__device__ __forceinline__ int32_t tid_of_key(int64_t key) { return (int32_t)((uint32_t)key & 0x7FFFFFFFu); }

__device__ __forceinline__ int64_t part_of(const Ev &v) { return (int64_t)v.glue + v.pre + v.len + v.term; }

// The kPer cells of tile t that thread tid owns, with the glue in front of each: extract.hip's tile_eval, the glue only
// in front of a range whose HEAD bit is set.  carry: the key of the last used range in front of the tile (0: none); it is
// moved behind the tile.  first: the key of the first used range seen so far (0: none yet).  Called by every thread.
__device__ __forceinline__ void tile_eval(const FmArgs &g, uint32_t t, uint32_t m, int64_t &carry, int64_t &first, Ev (&ev)[kPer],
    int64_t *red64)
{
	int64_t mine = 0, lowest = 0;
#pragma unroll
	for (int k = 0; k < kPer; k++) {
		const uint32_t i = t * kTile + threadIdx.x * kPer + k;
		ev[k] = Ev{};
		if (i < m)
			ev[k] = eval(g, i);
		if (ev[k].used) {
			mine = key_of(i, ev[k]);
			if (!lowest)
				lowest = mine;
		}
	}
	int64_t tile_max;
	int64_t prev = max(carry, block_prefix_max64(mine, red64, tile_max));
#pragma unroll
	for (int k = 0; k < kPer; k++)
		if (ev[k].used) {
			ev[k].glue = prev && ev[k].head && tid_of_key(prev) == ev[k].tid ? g.glue_len : 0;
			prev = key_of(t * kTile + threadIdx.x * kPer + k, ev[k]);
		}
	if (!first) {   // (uniform: first is the same in every thread)
		// the smallest key of the tile: the maximum of the complements
		int64_t dummy;
		const int64_t inv = lowest ? INT64_MAX - lowest : 0;
		block_prefix_max64(inv, red64, dummy);
		first = dummy ? INT64_MAX - dummy : 0;
	}
	carry = max(carry, tile_max);
}

__global__ __launch_bounds__(kThreads) void k_fm_sum(FmArgs g)
{
	__shared__ uint32_t red[kWaves];
	__shared__ int64_t red64[kWaves];

	const uint32_t m = ranges_of(g);
	const Share sh = share_of((g.R + kTile - 1) / kTile);
	uint32_t used = 0, skip = 0, terms = 0;
	int64_t bytes = 0, src = 0, carry = 0, first = 0;
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++) {
		Ev ev[kPer];
		tile_eval(g, t, m, carry, first, ev, red64);
#pragma unroll
		for (int k = 0; k < kPer; k++) {
			const uint32_t i = t * kTile + threadIdx.x * kPer + k;
			if (i >= m)
				continue;
			used += ev[k].used ? 1 : 0;
			skip += ev[k].used ? 0 : 1;
			terms += (uint32_t)ev[k].term;
			bytes += ev[k].used ? part_of(ev[k]) : 0;
			src += ev[k].len;
		}
	}
	used = block_sum(used, red);
	skip = block_sum(skip, red);
	terms = block_sum(terms, red);
	bytes = block_sum64(bytes, red64);
	src = block_sum64(src, red64);
	if (threadIdx.x == 0) {
		BlockSum b;
		b.bytes = bytes;
		b.src = src;
		b.used = used;
		b.skip = skip;
		b.terms = terms;
		b.first_lo = (uint32_t)first;
		b.last_lo = (uint32_t)carry;
		b.pad = 0;
		g.blk[blockIdx.x] = b;
	}
}

// the glue in front of block j's first used range: the last block in front that has a used range decides
__device__ __forceinline__ int64_t front_glue(const FmArgs &g, uint32_t j)
{
	if (g.blk[j].used == 0 || !(g.blk[j].first_lo >> 31))
		return 0;
	for (uint32_t p = j; p-- > 0;)
		if (g.blk[p].used)
			return ((g.blk[p].last_lo ^ g.blk[j].first_lo) & 0x7FFFFFFFu) == 0 ? g.glue_len : 0;
	return 0;
}

__global__ __launch_bounds__(kThreads) void k_fm_place(FmArgs g)
{
	__shared__ uint32_t red[kWaves];
	__shared__ int64_t red64[kWaves];

	const uint32_t tid = threadIdx.x;
	const uint32_t m = ranges_of(g);
	uint32_t used_before = 0, used_all = 0, skip_all = 0, terms_all = 0;
	int64_t bytes_before = 0, bytes_all = 0, src_all = 0, last_before = 0;
	for (uint32_t j = tid; j < gridDim.x; j += kThreads) {
		const BlockSum b = g.blk[j];
		const int64_t bytes = b.bytes + front_glue(g, j);
		used_all += b.used;
		skip_all += b.skip;
		terms_all += b.terms;
		bytes_all += bytes;
		src_all += b.src;
		if (j < blockIdx.x) {
			used_before += b.used;
			bytes_before += bytes;
			if (b.used)
				last_before = max(last_before, (int64_t)((uint64_t)(j + 1) << 32 | (b.last_lo & 0x7FFFFFFFu)));
		}
	}
	used_before = block_sum(used_before, red);
	used_all = block_sum(used_all, red);
	skip_all = block_sum(skip_all, red);
	terms_all = block_sum(terms_all, red);
	bytes_before = block_sum64(bytes_before, red64);
	bytes_all = block_sum64(bytes_all, red64);
	src_all = block_sum64(src_all, red64);
	{
		int64_t all;
		block_prefix_max64(last_before, red64, all);
		last_before = all;   // 0: no used range in front of this block
	}

	const Share sh = share_of((g.R + kTile - 1) / kTile);
	// a key in front of every key of this block that carries the text id of the last used range in front
	// (the keys of this block are (i + 1) << 32 | ... with i >= kTile: a block in front owns tile 0)
	int64_t carry = last_before ? (int64_t)(1ull << 32 | (uint32_t)last_before) : 0, first = 1;
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++) {
		Ev ev[kPer];
		tile_eval(g, t, m, carry, first, ev, red64);
		uint32_t c = 0;
		int64_t by = 0;
#pragma unroll
		for (int k = 0; k < kPer; k++) {
			c += ev[k].used ? 1 : 0;
			by += ev[k].used ? part_of(ev[k]) : 0;
		}
		uint32_t tile_c;
		int64_t tile_b;
		uint32_t rank = used_before + block_prefix(c, red, tile_c);   // (< m <= R)
		int64_t at = bytes_before + block_prefix64(by, red64, tile_b);
#pragma unroll
		for (int k = 0; k < kPer; k++)
			if (ev[k].used) {
				const int64_t part = part_of(ev[k]);
				g.rng_end[rank] = at + part;
				g.rng[rank] = make_int4(ev[k].s, ev[k].len, ev[k].pre, ev[k].glue | ev[k].term << 8 | ev[k].sel << 9);
				g.pre[rank] = ev[k].p;
				if (g.at_out && (uint64_t)rank + 2 < g.at_cap)
					g.at_out[1 + rank] = sat32(at + ev[k].glue + ev[k].pre);
				if (g.segments)
					atomicAdd((unsigned long long *)&g.bucket[ev[k].tid], (unsigned long long)part);
				rank++;
				at += part;
			}
		used_before += tile_c;
		bytes_before += tile_b;
	}
	if (blockIdx.x == 0 && tid == 0) {
		g.hdr[0] = used_all;
		g.hdr[1] = bytes_all;
		g.info[0] = (int32_t)used_all;
		g.info[1] = (int32_t)skip_all;
		g.info[2] = (int32_t)(uint32_t)((uint64_t)bytes_all & 0xFFFFFFFFu);
		g.info[3] = (int32_t)(bytes_all >> 32);
		g.info[4] = (int32_t)(uint32_t)((uint64_t)src_all & 0xFFFFFFFFu);
		g.info[5] = (int32_t)(src_all >> 32);
		g.info[6] = (g.out && bytes_all > (int64_t)g.cap) ? 1 : 0;
		g.info[7] = (int32_t)min(terms_all, 0x7FFFFFFFu);
		if (g.at_out)
			write_ends(g.at_out, g.at_cap, used_all, 0);
	}
}

// ---- where each text's part lies in the output: seg_out[k] = the buckets [0, k] (as in extract.hip) ----

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void k_fm_seg(FmArgs g)
{
	__shared__ int64_t red64[kWaves];
	const Share sh = share_of((g.segments + kThreads - 1) / kThreads);
	int64_t base = 0;
	if (WRITE) {
		for (uint32_t j = threadIdx.x; j < blockIdx.x; j += kThreads)
			base += g.seg_blk[j];
		base = block_sum64(base, red64);
	}
	int64_t sum = 0;
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++) {
		const uint32_t k = t * kThreads + threadIdx.x;
		const int64_t v = k < g.segments ? g.bucket[k] : 0;
		if (!WRITE) {
			sum += v;
			continue;
		}
		int64_t tile_total;
		const int64_t ex = base + block_prefix64(v, red64, tile_total);
		if (k < g.segments)
			g.seg_out[k] = sat32(ex + v);
		base += tile_total;
	}
	if (!WRITE) {
		sum = block_sum64(sum, red64);
		if (threadIdx.x == 0)
			g.seg_blk[blockIdx.x] = sum;
	}
}

// ---- the copy ----

// the decimal digits of v (nd of them) to the output offsets [x, x + nd), the part inside [t0, t1) into the tile
__device__ __forceinline__ void put_number(uint8_t *tile, int64_t t0, int64_t t1, int64_t x, uint64_t v, int32_t nd)
{
	int32_t k = nd - 1;
	for (; v > 0xFFFFFFFFull; k--) {   // (rare: a base beyond 2^32)
		const uint64_t q = v / 10;
		const int64_t at = x + k;
		if (at >= t0 && at < t1)
			tile[at - t0] = (uint8_t)('0' + (uint32_t)(v - q * 10));
		v = q;
	}
	uint32_t w = (uint32_t)v;
	for (; k >= 0; k--) {
		const uint32_t q = w / 10;
		const int64_t at = x + k;
		if (at >= t0 && at < t1)
			tile[at - t0] = (uint8_t)('0' + (w - q * 10));
		w = q;
	}
}

__global__ __launch_bounds__(kThreads) void k_fm_copy(FmArgs g)
{
	__shared__ __attribute__((aligned(16))) uint8_t tile[kTileBytes];
	__shared__ uint32_t pre[kThreads];                 // pieces of the ranges in front, of the ranges in flight
	__shared__ int32_t r_sa[kThreads], r_sb[kThreads];   // their clipped source [sa, sb)
	__shared__ uint16_t r_dp[kThreads];                  // the tile offset of sa
	__shared__ uint32_t red[kWaves];                     // (and the two bounds of the tile's ranges)
	// 16 KiB + 3.5 KiB, as the extract's copy: eight workgroups a CU fit the 160 KiB of LDS

	const uint32_t tid = threadIdx.x;
	const uint32_t U = (uint32_t)min((uint64_t)g.hdr[0], (uint64_t)g.R);
	const int64_t m = g.hdr[1];
	const int64_t limit = m <= 0 ? 0 : min(m, (int64_t)g.cap);
	const int64_t t0 = (int64_t)blockIdx.x * kTileBytes;
	if (t0 >= limit || U == 0)
		return;
	const int64_t t1 = min(t0 + (int64_t)kTileBytes, limit);
	const int len = (int)(t1 - t0);

	// the ranges that own a byte of [t0, t1): rng_end ascends strictly, and t1 <= m = the last end
	if (tid < 128) {
		const uint32_t r = wave_upper_bound64(g.rng_end, U, tid < 64 ? t0 : t1 - 1);
		if ((tid & 63) == 0)
			red[tid / 64] = min(r, U - 1);
	}
	__syncthreads();
	const uint32_t r0 = red[0], r_last = red[1];

	if (r0 == r_last) {
		const int4 rec = g.rng[r0];
		const int64_t ob = g.rng_end[r0] - ((rec.w >> 8) & 1) - rec.y;   // where the range's bytes begin in the output
		if (t0 >= ob && t1 <= ob + rec.y) {
			// one range's bytes: a stream at one shift
			for (int x = (int)tid * 16; x < len; x += kThreads * 16) {
				const int64_t sx = (int64_t)rec.x + (t0 + x - ob);
				if (x + 16 <= len && sx + 16 <= (int64_t)g.n) {
					*(uint4 *)(g.out + t0 + x) = load_source<false>(g.text, sx);
				} else {
					for (int j = 0; j < 16 && x + j < len; j++)
						g.out[t0 + x + j] = g.text[sx + j];   // (sx + j < rec.x + rec.y <= n)
				}
			}
			return;
		}
	}

	for (uint32_t rb = r0; rb <= r_last; rb += kThreads) {
		const uint32_t r = rb + tid;
		uint32_t pieces = 0;
		int32_t sa = 0, sb = 0;
		uint32_t dp = 0;
		int32_t nm_dst = 0, nm_src = 0, nm_cnt = 0;   // the part of a long name that lies in the tile
		if (r <= r_last) {
			const int4 rec = g.rng[r];
			const int64_t end = g.rng_end[r];
			const int32_t glue = rec.w & 0xFF, term = (rec.w >> 8) & 1;
			const int64_t tb = end - term;           // the terminator, if any
			const int64_t bb = tb - rec.y;           // the bytes
			const int64_t pb = bb - rec.z;           // the prefix
			const int64_t gb = pb - glue;            // the glue
			for (int64_t x = max(gb, t0); x < min(pb, t1); x++)
				tile[x - t0] = g.glue.b[(x - gb) & (kMaxGlue - 1)];
			if (term && tb >= t0 && tb < t1)
				tile[tb - t0] = (uint8_t)g.term;
			if (rec.z > 0 && pb < t1 && bb > t0) {
				const PreRec p = g.pre[r];
				const uint8_t sep = (uint8_t)((rec.w >> 9) & 1 ? g.sel_sep : g.ctx_sep);
				int64_t x = pb;
				if (g.flags & ACM_FORMAT_NAME) {
					const int64_t lo = max(x, t0), hi = min(x + p.name_len, t1);
					if (hi > lo) {
						if (p.name_len > kShortName) {
							nm_dst = (int32_t)(lo - t0);
							nm_src = p.name_at + (int32_t)(lo - x);
							nm_cnt = (int32_t)(hi - lo);
						} else {
							for (int64_t y = lo; y < hi; y++)
								tile[y - t0] = g.names[p.name_at + (y - x)];   // (in [name_at, name_at + name_len))
						}
					}
					x += p.name_len;
					if (x >= t0 && x < t1)
						tile[x - t0] = sep;
					x++;
				}
				if (g.flags & ACM_FORMAT_NUMBER) {
					const int32_t nd = digits_of((uint64_t)p.num);
					put_number(tile, t0, t1, x, (uint64_t)p.num, nd);
					x += nd;
					if (x >= t0 && x < t1)
						tile[x - t0] = sep;
					x++;
				}
				if (g.flags & ACM_FORMAT_OFFSET) {
					const int32_t nd = digits_of((uint64_t)p.off);
					put_number(tile, t0, t1, x, (uint64_t)p.off, nd);
					x += nd;
					if (x >= t0 && x < t1)
						tile[x - t0] = sep;
				}
			}
			const int64_t xa = max(bb, t0), xb = min(tb, t1);
			if (xa < xb) {
				sa = (int32_t)(rec.x + (xa - bb));
				sb = (int32_t)(rec.x + (xb - bb));
				dp = (uint32_t)(xa - t0);   // < kTileBytes
				pieces = (uint32_t)(((sb + 15) >> 4) - (sa >> 4));
			}
		}
		// the long names of this wave's ranges, one after the other, a byte a lane
		for (uint64_t todo = __ballot(nm_cnt > 0); todo; todo &= todo - 1) {
			const int src = __builtin_ctzll(todo);
			const int32_t dst = __shfl(nm_dst, src, 64), from = __shfl(nm_src, src, 64), cnt = __shfl(nm_cnt, src, 64);
			for (int32_t k = (int32_t)lane_id(); k < cnt; k += 64)
				tile[dst + k] = g.names[from + k];
		}
		uint32_t total;
		const uint32_t before = block_prefix(pieces, red, total);
		__syncthreads();   // (the arrays of the ranges in flight before are no longer read)
		pre[tid] = before;
		r_sa[tid] = sa;
		r_sb[tid] = sb;
		r_dp[tid] = (uint16_t)dp;
		__syncthreads();
		for (uint32_t p = tid; p < total; p += kThreads) {
			uint32_t lo = 0, hi = kThreads;   // the last range with pre <= p that has a piece: pre ascends
			while (hi - lo > 1) {
				const uint32_t mid = (lo + hi) >> 1;
				if (pre[mid] <= p)
					lo = mid;
				else
					hi = mid;
			}
			const int32_t a = r_sa[lo], b = r_sb[lo];
			const int32_t A = ((a >> 4) + (int32_t)(p - pre[lo])) << 4;   // the piece: text[A, A + 16), aligned
			const int plo = max(a, A) - A, phi = min(b, A + 16) - A;
			const uint4 v = *(const uint4 *)(g.text + A);   // (A < b <= n: readable up to round16(n))
			lds_put(tile, v, plo, phi, (int)r_dp[lo] + (A - a));
		}
	}
	__syncthreads();
	for (int x = (int)tid * 16; x < len; x += kThreads * 16) {
		if (x + 16 <= len) {
			*(uint4 *)(g.out + t0 + x) = *(const uint4 *)(tile + x);
		} else {
			for (int j = 0; x + j < len; j++)
				g.out[t0 + x + j] = tile[x + j];
		}
	}
}

// ---- host side ----

struct Layout {
	size_t blk, hdr, rng_end, rng, pre, bucket, seg_blk, total;
};

uint32_t seg_grid(size_t segments)
{
	return (uint32_t)std::max<size_t>(1, std::min<size_t>((segments + kThreads - 1) / kThreads, kMaxBlocks));
}

Layout layout_of(size_t max_ranges, size_t segments)
{
	Layout l;
	size_t at = 0;
	auto take = [&](size_t bytes) {
		const size_t here = at;
		at += round256(bytes);
		return here;
	};
	l.blk = take((size_t)kMaxBlocks * sizeof(BlockSum));
	l.hdr = take(4 * sizeof(int64_t));
	l.seg_blk = take((size_t)kMaxBlocks * sizeof(int64_t));
	l.rng_end = take(max_ranges * sizeof(int64_t));
	l.rng = take(max_ranges * sizeof(int4));
	l.pre = take(max_ranges * sizeof(PreRec));
	l.bucket = take(segments ? (segments + 1) * sizeof(int64_t) : 0);
	l.total = at;
	return l;
}

constexpr size_t kMaxBytes = 0x7FFFFFFFul - 16;   // 2^31 - 17

}  // namespace

extern "C" size_t acm_format_workspace_bytes(size_t max_ranges, size_t segments)
{
	return layout_of(max_ranges, segments).total;
}

extern "C" int acm_format_async(const void *d_text, size_t n, long text_origin, const int32_t *d_begin_plane,
    const int32_t *d_end_plane, size_t max_ranges, unsigned flags, const int32_t *d_kind_plane, const int32_t *d_num_plane,
    const int32_t *d_seg_num, long number_base, long offset_base, int sel_sep, int ctx_sep, const uint8_t *d_names,
    const int32_t *d_name_off, size_t names_bytes, const uint8_t *glue, int glue_len, int terminator, void *d_out,
    size_t out_capacity, int32_t *d_at_out, size_t at_capacity, const int32_t *d_seg_start, size_t segments, int32_t *d_seg_out,
    int32_t *d_info, void *d_workspace, size_t workspace_bytes, void *stream)
{
	if (!d_begin_plane || !d_end_plane || !d_info || (!d_text && n > 0) || ((uintptr_t)d_text & 15) || ((uintptr_t)d_out & 15) ||
	    n > kMaxBytes || out_capacity > kMaxBytes || (!d_out && out_capacity > 0) || (d_at_out && at_capacity < 2) ||
	    max_ranges > 0x7FFFFFFEul || segments > 0x7FFFFFFFul || text_origin < (long)INT32_MIN || text_origin > (long)INT32_MAX)
		return acm::fail(ACM_ERR_ARG, "acm_format_async: bad arguments");
	if ((segments > 0) != (d_seg_start != nullptr) || (segments > 0) != (d_seg_out != nullptr))
		return acm::fail(ACM_ERR_ARG, "acm_format_async: segments without both arrays, or arrays without segments");
	if (flags & ~kKnownFlags)
		return acm::fail(ACM_ERR_ARG, "acm_format_async: unknown flag bits 0x%x", flags);
	if ((flags & ACM_FORMAT_NAME) && (!d_names || !d_name_off || names_bytes > 0x7FFFFFFFul))
		return acm::fail(ACM_ERR_ARG, "acm_format_async: ACM_FORMAT_NAME without both name arrays, or a table over 2^31 - 1 bytes");
	if ((flags & ACM_FORMAT_NUMBER) && !d_num_plane)
		return acm::fail(ACM_ERR_ARG, "acm_format_async: ACM_FORMAT_NUMBER without d_num_plane");
	if (number_base < 0 || (int64_t)number_base > kMaxBase || offset_base < 0 || (int64_t)offset_base > kMaxBase)
		return acm::fail(ACM_ERR_ARG, "acm_format_async: number_base or offset_base outside 0..10^18");
	if (sel_sep < 0 || sel_sep > 255 || ctx_sep < 0 || ctx_sep > 255)
		return acm::fail(ACM_ERR_ARG, "acm_format_async: a separator outside 0..255");
	if (glue_len < 0 || glue_len > kMaxGlue || (!glue && glue_len > 0))
		return acm::fail(ACM_ERR_ARG, "acm_format_async: glue of %d bytes (0..%d, not NULL)", glue_len, kMaxGlue);
	if (terminator < -1 || terminator > 255)
		return acm::fail(ACM_ERR_ARG, "acm_format_async: terminator %d outside -1..255", terminator);
	const Layout l = layout_of(max_ranges, segments);
	if (!d_workspace || workspace_bytes < l.total)
		return acm::fail(ACM_ERR_ARG, "acm_format_async: workspace %zu B < required %zu B", workspace_bytes, l.total);

	char *ws = (char *)d_workspace;
	FmArgs g{};
	g.begin_plane = d_begin_plane;
	g.end_plane = d_end_plane;
	g.kind_plane = d_kind_plane;
	g.num_plane = d_num_plane;
	g.seg_num = d_seg_num;
	g.R = (uint32_t)max_ranges;
	g.text = (const uint8_t *)d_text;
	g.n = (uint32_t)n;
	g.origin = (int64_t)text_origin;
	g.inclusive = (flags & ACM_EXTRACT_END_INCLUSIVE) ? 1 : 0;
	g.flags = flags;
	g.number_base = (int64_t)number_base;
	g.offset_base = (int64_t)offset_base;
	g.sel_sep = (uint32_t)sel_sep;
	g.ctx_sep = (uint32_t)ctx_sep;
	g.names = d_names;
	g.name_off = d_name_off;
	g.names_bytes = (int64_t)names_bytes;
	for (int i = 0; i < glue_len; i++)
		g.glue.b[i] = glue[i];
	g.glue_len = glue_len;
	g.term = terminator;
	g.seg_start = d_seg_start;
	g.segments = (uint32_t)segments;
	g.blk = (BlockSum *)(ws + l.blk);
	g.hdr = (int64_t *)(ws + l.hdr);
	g.rng_end = (int64_t *)(ws + l.rng_end);
	g.rng = (int4 *)(ws + l.rng);
	g.pre = (PreRec *)(ws + l.pre);
	g.bucket = (int64_t *)(ws + l.bucket);
	g.seg_blk = (int64_t *)(ws + l.seg_blk);
	g.out = (uint8_t *)d_out;
	g.cap = (uint32_t)out_capacity;
	g.at_out = d_at_out;
	g.at_cap = clamp_cap(at_capacity);
	g.seg_out = d_seg_out;
	g.info = d_info;

	hipStream_t s = (hipStream_t)stream;
	const dim3 grid(grid_for(max_ranges)), block(kThreads);
	if (segments > 0)
		ACM_HIP_TRY(hipMemsetAsync(g.bucket, 0, (segments + 1) * sizeof(int64_t), s));
	hipLaunchKernelGGL(k_fm_sum, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_fm_place, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	if (segments > 0) {
		const dim3 sgrid(seg_grid(segments));
		hipLaunchKernelGGL(k_fm_seg<false>, sgrid, block, 0, s, g);
		ACM_HIP_TRY(hipGetLastError());
		hipLaunchKernelGGL(k_fm_seg<true>, sgrid, block, 0, s, g);
		ACM_HIP_TRY(hipGetLastError());
	}
	if (out_capacity > 0) {
		hipLaunchKernelGGL(k_fm_copy, dim3((uint32_t)((out_capacity + kTileBytes - 1) / kTileBytes)), block, 0, s, g);
		ACM_HIP_TRY(hipGetLastError());
	}
	return ACM_OK;
}
