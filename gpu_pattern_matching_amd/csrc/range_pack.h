// Range packing: ranges of a device text gathered into one packed output.  The core of the extract (extract.hip) and of the
// format pass (format.hip), which instantiate it with a policy P.  Internal to the library, gfx950 only.  DESIGN.md 6q, 6r.
//
// Range i of the planes is [b, e) (e one further with ACM_EXTRACT_END_INCLUSIVE); it is USED iff
// text_origin <= b < e <= text_end.  A used range puts into the output, in input order: the glue (iff it is a HEAD and the
// last used range in front of it has the same text id), the prefix (P::kPrefix), its bytes, the terminator (iff its last
// byte is another).  Without a prefix policy every used range is a head and its prefix is empty: the extract.  With one,
// P::eval sets a range's kind bits, the size of its prefix and a P::Rec to print it from, and P::put_prefix prints it.
// Launches:
//   k_pack_sum   the record-pass grid (record_pass.h) over max_ranges cells, a thread owning kPer consecutive cells:
//                per block the used and skipped ranges, the output bytes (without the glue in front of the block's
//                first used range: that one needs the block in front), the text bytes, the terminators, and the low
//                key word (HEAD bit and text id) of its first and of its last used range
//   k_pack_place the same grid: a block sums the blocks in front of its own, decides the glue at every block's front
//                from the summaries, ranks its ranges in input order and writes the used ones densely:
//                rng_end[r] = the output offset behind range r's part (int64), rng[r] = {b - text_origin, bytes, prefix
//                bytes, glue bytes | terminator << 8 | selected << 9}, with a prefix pre[r]; d_at_out; with segments the
//                part's size is added to its text's bucket (integer atomics: a sum, no order); block 0 writes d_info
//                and hdr = {used, m}
//   k_pack_seg   (segments > 0, two launches) a 64-bit inclusive prefix over the buckets: d_seg_out
//   k_pack_copy  (out_capacity > 0) a workgroup per kTileBytes of OUTPUT, staged in LDS.  The ranges of the tile are
//                [first range that ends behind the tile's first byte, range of the tile's last byte], found by two waves
//                at once on rng_end (ascending: every used range has a byte).  A tile inside the bytes of one range
//                streams: 16-byte source pieces at one byte shift, aligned stores.  Otherwise the tile's ranges are
//                taken kThreads at a time: a thread per range puts its glue, prefix and terminator into LDS and counts
//                the 16-byte ALIGNED source pieces its bytes lie in; a block prefix of the counts hands the pieces out, a
//                piece a lane: one aligned 16-byte load, shifted to the destination's dword phase in registers and
//                written to LDS as dwords (bytes only at a range's two ends).  Then LDS goes to d_out in aligned
//                16-byte stores; only the piece that min(m, out_capacity) cuts is stored byte by byte.
// The "last used range in front" of a cell is an exclusive prefix MAXIMUM of (cell index + 1) << 32 | HEAD << 31 | text id
// (the extract's keys leave the HEAD bit out, see key_of): the same shuffles as a sum.  No atomics decide an order; no read-modify-write of d_out; no byte at or behind
// min(m, out_capacity) is written.
#pragma once

#include <hip/hip_runtime.h>

#include "acm_internal.h"
#include "place64.h"
#include "record_pass.h"

namespace acm_rp {

constexpr int kMaxGlue = ACM_EXTRACT_MAX_GLUE;
constexpr size_t kMaxSegments = 0x7FFFFFFFul;
static_assert(kMaxSegments < (1ull << 31), "a text id (<= segments) shares a key's low word with the HEAD bit");

struct Glue {
	uint8_t b[kMaxGlue];
};

struct BlockSum {          // what k_pack_sum leaves per block
	int64_t bytes, src;    // output bytes (see above), text bytes
	uint32_t used, skip, terms;
	uint32_t first_lo, last_lo;   // the low words of the keys of the block's first and last used range (used > 0)
	uint32_t pad;
};

template <class P>
struct PackArgs {
	const int32_t *begin_plane, *end_plane;
	uint32_t R;
	const uint8_t *text;
	uint32_t n;
	int64_t origin;
	int inclusive;
	Glue glue;
	int glue_len, term;
	const int32_t *seg_start;
	uint32_t segments;
	// workspace
	BlockSum *blk;           // [gridDim.x of the range grid]
	int64_t *hdr;            // {used ranges, m}
	int64_t *rng_end;        // [R] per used range, in input order: the output offset behind its part
	int4 *rng;               // [R] {b - origin, bytes, prefix bytes, glue bytes | terminator << 8 | selected << 9}
	int64_t *bucket;         // [segments + 1] output bytes of the ranges of each text id
	int64_t *seg_blk;        // [blocks of the segment grid]
	// output
	uint8_t *out;
	uint32_t cap;
	int32_t *at_out;
	uint32_t at_cap;
	int32_t *seg_out;
	int32_t *info;
	P x;                     // what the instantiation adds
};

template <class P>
struct Ev {
	bool used;
	int32_t s, len, tid, term;   // term: 1 iff a terminator follows
	int32_t head, sel;           // the kind bits (P::kPrefix: without a prefix policy every used range is a head)
	int32_t pre;                 // prefix bytes
	int32_t glue;                // glue bytes in front (set by tile_eval)
	typename P::Rec p;
};

template <class P>
__device__ __forceinline__ uint32_t ranges_of(const PackArgs<P> &g)
{
	return (uint32_t)min((int64_t)max(g.begin_plane[0], 0), (int64_t)g.R);
}

// range i < the count
template <class P>
__device__ __forceinline__ Ev<P> eval(const PackArgs<P> &g, uint32_t i)
{
	Ev<P> v{};
	const int64_t b = g.begin_plane[1 + i];
	const int64_t e = (int64_t)g.end_plane[1 + i] + g.inclusive;
	if (b < g.origin || b >= e || e > g.origin + (int64_t)g.n)
		return v;
	v.used = true;
	v.s = (int32_t)(b - g.origin);   // in [0, n)
	v.len = (int32_t)(e - b);        // in [1, n - s]
	v.tid = g.segments ? (int32_t)upper_bound_i32(g.seg_start, g.segments, b) : 0;
	v.term = g.term >= 0 && g.text[(int64_t)v.s + v.len - 1] != (uint8_t)g.term ? 1 : 0;
	if constexpr (P::kPrefix)
		g.x.eval(g, i, b, v);
	return v;
}

// (cell index + 1) << 32 | HEAD << 31 | text id (< 2^31).  Without a prefix policy every used range is a head: its keys
// leave the bit out and nothing reads Ev::head (the bit and its masks cost the extract's sum and place kernels fifty
// instructions each).
template <class P>
constexpr uint32_t kHeadBit = P::kPrefix ? 0x80000000u : 0;

template <class P>
__device__ __forceinline__ int64_t key_of(uint32_t i, const Ev<P> &v)
{
	return (int64_t)((uint64_t)(i + 1) << 32 | (v.head ? kHeadBit<P> : 0) | (uint32_t)v.tid);
}

template <class P>
__device__ __forceinline__ int32_t tid_of_key(int64_t key) { return (int32_t)((uint32_t)key & ~kHeadBit<P>); }

template <class P>
__device__ __forceinline__ int64_t part_of(const Ev<P> &v) { return (int64_t)v.glue + v.pre + v.len + v.term; }

// The kPer cells of tile t that thread tid owns, [t * kTile + tid * kPer, + kPer), with the glue in front of each.
// carry: the key of the last used range in front of the tile (0: none); it is moved behind the tile.  first: the key
// of the first used range seen so far (0: none yet).  Called by every thread of the block.
template <class P>
__device__ __forceinline__ void tile_eval(const PackArgs<P> &g, uint32_t t, uint32_t m, int64_t &carry, int64_t &first,
    Ev<P> (&ev)[kPer], int64_t *red64)
{
	int64_t mine = 0, lowest = 0;
#pragma unroll
	for (int k = 0; k < kPer; k++) {
		const uint32_t i = t * kTile + threadIdx.x * kPer + k;
		ev[k] = Ev<P>{};
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
			const bool head = !P::kPrefix || ev[k].head;
			ev[k].glue = prev && head && tid_of_key<P>(prev) == ev[k].tid ? g.glue_len : 0;
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

template <class P>
__global__ __launch_bounds__(kThreads) void k_pack_sum(PackArgs<P> g)
{
	__shared__ uint32_t red[kWaves];
	__shared__ int64_t red64[kWaves];

	const uint32_t m = ranges_of(g);
	const Share sh = share_of((g.R + kTile - 1) / kTile);
	uint32_t used = 0, skip = 0, terms = 0;
	int64_t bytes = 0, src = 0, carry = 0, first = 0;
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++) {
		Ev<P> ev[kPer];
		tile_eval(g, t, m, carry, first, ev, red64);
#pragma unroll
		for (int k = 0; k < kPer; k++) {
			const uint32_t i = t * kTile + threadIdx.x * kPer + k;
			if (i >= m)
				continue;
			used += ev[k].used ? 1 : 0;
			skip += ev[k].used ? 0 : 1;
			terms += (uint32_t)ev[k].term;
			bytes += part_of(ev[k]);   // (0 for a range that is not used)
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

// the glue in front of block j's first used range, a head: the last block in front that has a used range decides
template <class P>
__device__ __forceinline__ int64_t front_glue(const PackArgs<P> &g, uint32_t j)
{
	if (g.blk[j].used == 0 || (g.blk[j].first_lo & kHeadBit<P>) != kHeadBit<P>)
		return 0;
	for (uint32_t p = j; p-- > 0;)
		if (g.blk[p].used)
			return ((g.blk[p].last_lo ^ g.blk[j].first_lo) & ~kHeadBit<P>) == 0 ? g.glue_len : 0;
	return 0;
}

template <class P>
__global__ __launch_bounds__(kThreads) void k_pack_place(PackArgs<P> g)
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
				last_before = max(last_before, (int64_t)((uint64_t)(j + 1) << 32 | (b.last_lo & ~kHeadBit<P>)));
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
		Ev<P> ev[kPer];
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
				if constexpr (P::kPrefix)
					g.x.pre[rank] = ev[k].p;
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

// ---- where each text's part lies in the output: seg_out[k] = the buckets [0, k] ----

template <class P, bool WRITE>
__global__ __launch_bounds__(kThreads) void k_pack_seg(PackArgs<P> g)
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

struct LongName {   // the part of a name too long for one thread that lies in the tile: copied by the thread's wave
	int32_t dst = 0, src = 0, cnt = 0;
};

template <class P>
__global__ __launch_bounds__(kThreads) void k_pack_copy(PackArgs<P> g)
{
	__shared__ __attribute__((aligned(16))) uint8_t tile[kTileBytes];
	__shared__ uint32_t pre[kThreads];                 // pieces of the ranges in front, of the ranges in flight
	__shared__ int32_t r_sa[kThreads], r_sb[kThreads];   // their clipped source [sa, sb)
	__shared__ uint16_t r_dp[kThreads];                  // the tile offset of sa
	__shared__ uint32_t red[kWaves];                     // (and the two bounds of the tile's ranges)
	// 16 KiB + 3.5 KiB: eight workgroups a CU fit the 160 KiB of LDS, and with them every tile of a 32 MiB output at once

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
	// (two waves search at the same time: the two chains of dependent loads overlap)
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
		LongName nm;
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
			if constexpr (P::kPrefix)
				if (rec.z > 0 && pb < t1 && bb > t0) {
					const typename P::Rec p = g.x.pre[r];
					g.x.put_prefix(tile, t0, t1, pb, p, (rec.w >> 9) & 1, nm);
				}
			const int64_t xa = max(bb, t0), xb = min(tb, t1);
			if (xa < xb) {
				sa = (int32_t)(rec.x + (xa - bb));
				sb = (int32_t)(rec.x + (xb - bb));
				dp = (uint32_t)(xa - t0);   // < kTileBytes
				pieces = (uint32_t)(((sb + 15) >> 4) - (sa >> 4));
			}
		}
		if constexpr (P::kPrefix)
			g.x.put_long_names(tile, nm);   // (every lane of the wave)
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

// rec_bytes: the size of a range's prefix record, 0 without a prefix policy (no pre region)
inline Layout layout_of(size_t max_ranges, size_t segments, size_t rec_bytes)
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
	l.pre = take(max_ranges * rec_bytes);
	l.bucket = take(segments ? (segments + 1) * sizeof(int64_t) : 0);
	l.total = at;
	return l;
}

template <class P>
inline size_t pack_workspace_bytes(size_t max_ranges, size_t segments)
{
	return layout_of(max_ranges, segments, P::kPrefix ? sizeof(typename P::Rec) : 0).total;
}

struct PackCall {   // the arguments the two entry points share, in the order of their signatures
	const void *text;
	size_t n;
	long origin;
	const int32_t *begin_plane, *end_plane;
	size_t max_ranges;
	unsigned flags;
	const uint8_t *glue;
	int glue_len, terminator;
	void *out;
	size_t out_capacity;
	int32_t *at_out;
	size_t at_capacity;
	const int32_t *seg_start;
	size_t segments;
	int32_t *seg_out, *info;
	void *workspace;
	size_t workspace_bytes;
	void *stream;
};

// Checks the call `who`, with more_checks() (its own ACM_OK or failure) between the flags and the glue, and enqueues it.
// x: the policy's own arguments; its pre, if any, is set here.
template <class P, class More>
inline int pack_async(const char *who, const PackCall &c, unsigned known_flags, P x, More more_checks)
{
	if (!c.begin_plane || !c.end_plane || !c.info || (!c.text && c.n > 0) || ((uintptr_t)c.text & 15) || ((uintptr_t)c.out & 15) ||
	    c.n > kMaxBytes || c.out_capacity > kMaxBytes || (!c.out && c.out_capacity > 0) || (c.at_out && c.at_capacity < 2) ||
	    c.max_ranges > 0x7FFFFFFEul || c.segments > kMaxSegments || c.origin < (long)INT32_MIN || c.origin > (long)INT32_MAX)
		return acm::fail(ACM_ERR_ARG, "%s: bad arguments", who);
	if ((c.segments > 0) != (c.seg_start != nullptr) || (c.segments > 0) != (c.seg_out != nullptr))
		return acm::fail(ACM_ERR_ARG, "%s: segments without both arrays, or arrays without segments", who);
	if (c.flags & ~known_flags)
		return acm::fail(ACM_ERR_ARG, "%s: unknown flag bits 0x%x", who, c.flags);
	if (const int rc = more_checks())
		return rc;
	if (c.glue_len < 0 || c.glue_len > kMaxGlue || (!c.glue && c.glue_len > 0))
		return acm::fail(ACM_ERR_ARG, "%s: glue of %d bytes (0..%d, not NULL)", who, c.glue_len, kMaxGlue);
	if (c.terminator < -1 || c.terminator > 255)
		return acm::fail(ACM_ERR_ARG, "%s: terminator %d outside -1..255", who, c.terminator);
	const Layout l = layout_of(c.max_ranges, c.segments, P::kPrefix ? sizeof(typename P::Rec) : 0);
	if (!c.workspace || c.workspace_bytes < l.total)
		return acm::fail(ACM_ERR_ARG, "%s: workspace %zu B < required %zu B", who, c.workspace_bytes, l.total);

	char *ws = (char *)c.workspace;
	PackArgs<P> g{};
	g.begin_plane = c.begin_plane;
	g.end_plane = c.end_plane;
	g.R = (uint32_t)c.max_ranges;
	g.text = (const uint8_t *)c.text;
	g.n = (uint32_t)c.n;
	g.origin = (int64_t)c.origin;
	g.inclusive = (c.flags & ACM_EXTRACT_END_INCLUSIVE) ? 1 : 0;
	for (int i = 0; i < c.glue_len; i++)
		g.glue.b[i] = c.glue[i];
	g.glue_len = c.glue_len;
	g.term = c.terminator;
	g.seg_start = c.seg_start;
	g.segments = (uint32_t)c.segments;
	g.blk = (BlockSum *)(ws + l.blk);
	g.hdr = (int64_t *)(ws + l.hdr);
	g.rng_end = (int64_t *)(ws + l.rng_end);
	g.rng = (int4 *)(ws + l.rng);
	g.bucket = (int64_t *)(ws + l.bucket);
	g.seg_blk = (int64_t *)(ws + l.seg_blk);
	g.out = (uint8_t *)c.out;
	g.cap = (uint32_t)c.out_capacity;
	g.at_out = c.at_out;
	g.at_cap = clamp_cap(c.at_capacity);
	g.seg_out = c.seg_out;
	g.info = c.info;
	g.x = x;
	if constexpr (P::kPrefix)
		g.x.pre = (typename P::Rec *)(ws + l.pre);

	hipStream_t s = (hipStream_t)c.stream;
	const dim3 grid(grid_for(c.max_ranges)), block(kThreads);
	if (c.segments > 0)
		ACM_HIP_TRY(hipMemsetAsync(g.bucket, 0, (c.segments + 1) * sizeof(int64_t), s));
	hipLaunchKernelGGL(k_pack_sum<P>, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_pack_place<P>, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	if (c.segments > 0) {
		const dim3 sgrid((uint32_t)std::max<size_t>(1, std::min<size_t>((c.segments + kThreads - 1) / kThreads, kMaxBlocks)));
		hipLaunchKernelGGL((k_pack_seg<P, false>), sgrid, block, 0, s, g);
		ACM_HIP_TRY(hipGetLastError());
		hipLaunchKernelGGL((k_pack_seg<P, true>), sgrid, block, 0, s, g);
		ACM_HIP_TRY(hipGetLastError());
	}
	if (c.out_capacity > 0) {
		hipLaunchKernelGGL(k_pack_copy<P>, dim3((uint32_t)((c.out_capacity + kTileBytes - 1) / kTileBytes)), block, 0, s, g);
		ACM_HIP_TRY(hipGetLastError());
	}
	return ACM_OK;
}

}  // namespace acm_rp
