// Formatting extract: the extract with a generated prefix in front of every range's bytes -- a name from a table, a line
// number, a byte offset, each followed by a separator that depends on the range's kind (grep -H -n -b).  gfx950 only.
// DESIGN.md 6r.
//
// The range-packing core (range_pack.h) with the prefix policy below.  What it adds to the core's launches:
//   eval         (k_pack_sum, k_pack_place) a range's SELECTED and HEAD bits from the kind plane (without one: selected,
//                no head, so no glue), and its prefix: the name's place and length from the offset table, the two numbers
//                and the size of it all, the digits from a count against the powers of ten.  k_pack_place keeps
//                pre[r] = {line number, byte offset, where the name lies, its length}
//   put_prefix   (k_pack_copy) a range's thread puts its prefix into LDS, clipped to the tile.  Digits are made from
//                the value (a division by ten each) and written backwards; the separators are single bytes; a name of
//                at most kShortName bytes is copied by the range's thread, a longer one by the 64 lanes of its wave
//                (put_long_names).
#include "range_pack.h"

namespace {

using namespace acm_rp;

constexpr int32_t kMaxName = ACM_FORMAT_MAX_NAME;
constexpr int32_t kShortName = 32;       // a longer name is copied by the whole wave
constexpr int64_t kMaxBase = 1000000000000000000ll;
constexpr unsigned kKnownFlags = ACM_EXTRACT_END_INCLUSIVE | ACM_FORMAT_NAME | ACM_FORMAT_NUMBER | ACM_FORMAT_OFFSET;

__constant__ uint64_t kPow10[19] = { 1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull,
	1000000000ull, 10000000000ull, 100000000000ull, 1000000000000ull, 10000000000000ull, 100000000000000ull,
	1000000000000000ull, 10000000000000000ull, 100000000000000000ull, 1000000000000000000ull };

// decimal digits of v: 1..19
__device__ __forceinline__ int32_t digits_of(uint64_t v)
{
	int32_t d = 1;
#pragma unroll
	for (int k = 1; k < 19; k++)
		d += v >= kPow10[k] ? 1 : 0;
	return d;
}

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

struct Prefix {
	static constexpr bool kPrefix = true;
	struct Rec {               // what the copy kernel makes a used range's prefix from
		int64_t num, off;      // the values to print (>= 0)
		int32_t name_at, name_len;
	};

	const int32_t *kind_plane, *num_plane, *seg_num;
	unsigned flags;
	int64_t number_base, offset_base;
	uint32_t sel_sep, ctx_sep;
	const uint8_t *names;
	const int32_t *name_off;
	int64_t names_bytes;
	Rec *pre;                  // [R] workspace, beside rng

	// used range i, which begins at b: the kind bits, the prefix record and its size
	__device__ __forceinline__ void eval(const PackArgs<Prefix> &g, uint32_t i, int64_t b, Ev<Prefix> &v) const
	{
		const int32_t kind = kind_plane ? kind_plane[1 + i] : (int32_t)ACM_LINE_SELECTED;
		v.sel = kind & 1;
		v.head = (kind >> 1) & 1;
		if (flags & ACM_FORMAT_NAME) {
			const int64_t a = name_off[v.tid], z = name_off[v.tid + 1];   // (tid + 1 <= segments + 1)
			if (a >= 0 && a <= z && z <= names_bytes && z - a <= (int64_t)kMaxName) {
				v.p.name_at = (int32_t)a;
				v.p.name_len = (int32_t)(z - a);
			}
			v.pre += v.p.name_len + 1;
		}
		if (flags & ACM_FORMAT_NUMBER) {
			const int64_t first = v.tid > 0 && seg_num ? seg_num[v.tid - 1] : 0;
			v.p.num = max(number_base + (int64_t)num_plane[1 + i] - first, (int64_t)0);
			v.pre += digits_of((uint64_t)v.p.num) + 1;
		}
		if (flags & ACM_FORMAT_OFFSET) {
			const int64_t first = v.tid > 0 ? (int64_t)g.seg_start[v.tid - 1] : g.origin;
			v.p.off = max(offset_base + b - first, (int64_t)0);
			v.pre += digits_of((uint64_t)v.p.off) + 1;
		}
	}

	// the prefix made from p to the output offsets from pb on, the part inside [t0, t1) into the tile; a long name is
	// left to put_long_names
	__device__ __forceinline__ void put_prefix(uint8_t *tile, int64_t t0, int64_t t1, int64_t pb, const Rec &p, int sel,
	    LongName &nm) const
	{
		const uint8_t sep = (uint8_t)(sel ? sel_sep : ctx_sep);
		int64_t x = pb;
		if (flags & ACM_FORMAT_NAME) {
			const int64_t lo = max(x, t0), hi = min(x + p.name_len, t1);
			if (hi > lo) {
				if (p.name_len > kShortName) {
					nm.dst = (int32_t)(lo - t0);
					nm.src = p.name_at + (int32_t)(lo - x);
					nm.cnt = (int32_t)(hi - lo);
				} else {
					for (int64_t y = lo; y < hi; y++)
						tile[y - t0] = names[p.name_at + (y - x)];   // (in [name_at, name_at + name_len))
				}
			}
			x += p.name_len;
			if (x >= t0 && x < t1)
				tile[x - t0] = sep;
			x++;
		}
		if (flags & ACM_FORMAT_NUMBER) {
			const int32_t nd = digits_of((uint64_t)p.num);
			put_number(tile, t0, t1, x, (uint64_t)p.num, nd);
			x += nd;
			if (x >= t0 && x < t1)
				tile[x - t0] = sep;
			x++;
		}
		if (flags & ACM_FORMAT_OFFSET) {
			const int32_t nd = digits_of((uint64_t)p.off);
			put_number(tile, t0, t1, x, (uint64_t)p.off, nd);
			x += nd;
			if (x >= t0 && x < t1)
				tile[x - t0] = sep;
		}
	}

	// the long names of this wave's ranges, one after the other, a byte a lane
	__device__ __forceinline__ void put_long_names(uint8_t *tile, const LongName &nm) const
	{
		for (uint64_t todo = __ballot(nm.cnt > 0); todo; todo &= todo - 1) {
			const int src = __builtin_ctzll(todo);
			const int32_t dst = __shfl(nm.dst, src, 64), from = __shfl(nm.src, src, 64), cnt = __shfl(nm.cnt, src, 64);
			for (int32_t k = (int32_t)lane_id(); k < cnt; k += 64)
				tile[dst + k] = names[from + k];
		}
	}
};

}  // namespace

extern "C" size_t acm_format_workspace_bytes(size_t max_ranges, size_t segments)
{
	return pack_workspace_bytes<Prefix>(max_ranges, segments);
}

extern "C" int acm_format_async(const void *d_text, size_t n, long text_origin, const int32_t *d_begin_plane,
    const int32_t *d_end_plane, size_t max_ranges, unsigned flags, const int32_t *d_kind_plane, const int32_t *d_num_plane,
    const int32_t *d_seg_num, long number_base, long offset_base, int sel_sep, int ctx_sep, const uint8_t *d_names,
    const int32_t *d_name_off, size_t names_bytes, const uint8_t *glue, int glue_len, int terminator, void *d_out,
    size_t out_capacity, int32_t *d_at_out, size_t at_capacity, const int32_t *d_seg_start, size_t segments, int32_t *d_seg_out,
    int32_t *d_info, void *d_workspace, size_t workspace_bytes, void *stream)
{
	const PackCall c{ d_text, n, text_origin, d_begin_plane, d_end_plane, max_ranges, flags, glue, glue_len, terminator, d_out,
		out_capacity, d_at_out, at_capacity, d_seg_start, segments, d_seg_out, d_info, d_workspace, workspace_bytes, stream };
	const Prefix x{ d_kind_plane, d_num_plane, d_seg_num, flags, (int64_t)number_base, (int64_t)offset_base, (uint32_t)sel_sep,
		(uint32_t)ctx_sep, d_names, d_name_off, (int64_t)names_bytes, nullptr };
	return pack_async("acm_format_async", c, kKnownFlags, x, [&]() -> int {
		if ((flags & ACM_FORMAT_NAME) && (!d_names || !d_name_off || names_bytes > 0x7FFFFFFFul))
			return acm::fail(ACM_ERR_ARG, "acm_format_async: ACM_FORMAT_NAME without both name arrays, or a table over 2^31 - 1 bytes");
		if ((flags & ACM_FORMAT_NUMBER) && !d_num_plane)
			return acm::fail(ACM_ERR_ARG, "acm_format_async: ACM_FORMAT_NUMBER without d_num_plane");
		if (number_base < 0 || (int64_t)number_base > kMaxBase || offset_base < 0 || (int64_t)offset_base > kMaxBase)
			return acm::fail(ACM_ERR_ARG, "acm_format_async: number_base or offset_base outside 0..10^18");
		if (sel_sep < 0 || sel_sep > 255 || ctx_sep < 0 || ctx_sep > 255)
			return acm::fail(ACM_ERR_ARG, "acm_format_async: a separator outside 0..255");
		return ACM_OK;
	});
}
