// Extraction: ranges of a device text gathered into one packed output.  gfx950 only.  DESIGN.md 6q.
//
// The range-packing core (range_pack.h) with no prefix policy: every used range is a head, so the glue goes in front of a
// used range iff the last used range in front of it has the same text id; nothing stands between the glue and the bytes.
#include "range_pack.h"

namespace {

using namespace acm_rp;

struct NoPrefix {
	static constexpr bool kPrefix = false;
	struct Rec {};
};

}  // namespace

extern "C" size_t acm_extract_workspace_bytes(size_t max_ranges, size_t segments)
{
	return pack_workspace_bytes<NoPrefix>(max_ranges, segments);
}

extern "C" int acm_extract_async(const void *d_text, size_t n, long text_origin, const int32_t *d_begin_plane,
    const int32_t *d_end_plane, size_t max_ranges, unsigned flags, const uint8_t *glue, int glue_len, int terminator, void *d_out,
    size_t out_capacity, int32_t *d_at_out, size_t at_capacity, const int32_t *d_seg_start, size_t segments, int32_t *d_seg_out,
    int32_t *d_info, void *d_workspace, size_t workspace_bytes, void *stream)
{
	const PackCall c{ d_text, n, text_origin, d_begin_plane, d_end_plane, max_ranges, flags, glue, glue_len, terminator, d_out,
		out_capacity, d_at_out, at_capacity, d_seg_start, segments, d_seg_out, d_info, d_workspace, workspace_bytes, stream };
	return pack_async("acm_extract_async", c, ACM_EXTRACT_END_INCLUSIVE, NoPrefix{}, [] { return (int)ACM_OK; });
}
