// Position constraints per pattern: where in its text an entry may start.  gfx950 only.
//
// A window (acm_automaton_set_position) keeps pattern p of length L >= 1 that ends at offset o, so starts
// at a = o - L + 1, iff lo <= a - T0 <= hi (from the start of its text [T0, Tend)) or, with
// ACM_POS_FROM_END, lo <= Tend - a <= hi.  The predicate needs no text: the pattern's length, the offset
// and the bounds of the text the record lies in.  So the pass takes either form of plane:
//   ACM_REPORT_STATE  final states: the entries of a record are its state's match list (as word.hip,
//                     case.hip)
//   ACM_REPORT_HEAD   pattern indices, one entry per record: a HEAD scan, or what the word, case and
//                     expand passes write in their all-patterns form.  A run of records with equal offset
//                     is one offset.
// The text of a record is found as the tally finds its row: the starts a tile spans are staged in LDS
// (record_pass.h) and searched once per record; the start behind it, if it is <= text_end, is the text's
// end.  Otherwise the text is open: its end is open_end, or unknown (-1), and then an end-anchored entry
// is undecided: dropped and counted.
//
// Tables (device_dfa.hip, positioned automata only): d_pos_ent[p] = {lo, hi, flags, length}, one 16-byte
// load per entry.  An automaton without constraints has none; the pass then reads d_pat_len, keeps every
// entry of length >= 1 and looks up no segment.
//
// The pass is a two-launch ordered write over a fixed grid (record_pass.h):
//   k_position<false>  counts the cells every block writes and the undecided entries it drops
//   k_position<true>   counts again and writes in position order; block 0 writes the header, the trailer
//                      and d_info (the sum of the blocks' undecided counts: integers, the same on every run)
// First-entry form over HEAD input: a record that is kept (or undecided) is the first of its run iff no
// record in front of it with the same offset is kept; it finds that by looking back through the input
// plane and evaluating the predicate again (same offset, so same text).  No state is shared between
// threads, so tile and block cuts do not matter.
#include <hip/hip_runtime.h>

#include "acm_internal.h"
#include "device_dfa.h"
#include "record_pass.h"

namespace {

using namespace acm_rp;

constexpr int64_t kEndUnknown = INT64_MIN;

struct PosArgs {
	const int32_t *pat_plane, *off_plane;
	uint32_t max_records;
	int states;                  // the cells are states (ACM_REPORT_STATE), else pattern indices
	int all;
	const int32_t *seg_start;
	uint32_t segments;
	int64_t lead_begin, text_end, open_end;   // open_end: kEndUnknown when the caller passed -1
	const uint32_t *list_begin, *list_len;
	const int32_t *list_pool;
	const uint32_t *pat_len;
	const int4 *pos_ent;         // null: the automaton is not positioned, every entry of length >= 1 is kept
	uint32_t num_states, num_patterns;
	int32_t *pat_out, *off_out;
	uint32_t cap;
	int32_t *info;               // [4]
	int32_t *block_counts;       // [2][gridDim.x]: cells written, undecided entries
};

enum { kDrop = 0, kKeep = 1, kUndecided = 2 };

// the window of pattern p at offset o of the text [T0, Tend) (Tend: kEndUnknown)
__device__ __forceinline__ int verdict(const PosArgs &g, uint32_t p, int32_t o, int64_t T0, int64_t Tend)
{
	if (p >= g.num_patterns)
		return kDrop;
	if (!g.pos_ent)
		return g.pat_len[p] != 0 ? kKeep : kDrop;
	const int4 e = g.pos_ent[p];   // {lo, hi, flags, length}
	if (e.w == 0)
		return kDrop;
	if (e.x == 0 && e.y == INT32_MAX && e.z == 0)
		return kKeep;
	const int64_t a = (int64_t)o + 1 - (int64_t)e.w;
	int64_t v;
	if (e.z & ACM_POS_FROM_END) {
		if (Tend == kEndUnknown)
			return kUndecided;
		v = Tend - a;
	} else {
		v = a - T0;
	}
	return (v >= (int64_t)e.x && (e.y == INT32_MAX || v <= (int64_t)e.y)) ? kKeep : kDrop;
}

// One record at cell i of the input: the number of entries it writes (first form: 0 or 1, the pattern in
// head; undecided entries are added to und).  WRITE && all && states: the entries are written from cell
// 1 + d on.
template <bool WRITE>
__device__ __forceinline__ uint32_t one_record(const PosArgs &g, uint32_t i, int32_t o, uint32_t c, int64_t T0, int64_t Tend,
    uint32_t d, int32_t &head, uint32_t &und)
{
	if (!g.states) {
		const int v = verdict(g, c, o, T0, Tend);
		if (v == kDrop)
			return 0;
		if (!g.all)   // first of its run?  The records in front with this offset lie in the same text.
			for (uint32_t j = i; j > 0; j--) {
				if (g.off_plane[j] != o)   // (cell j holds record j - 1)
					break;
				if (verdict(g, (uint32_t)g.pat_plane[j], o, T0, Tend) == kKeep)
					return 0;
			}
		if (v == kUndecided) {
			und++;
			return 0;
		}
		head = (int32_t)c;
		return 1;
	}
	if (c >= g.num_states)   // not the planes of a STATE scan: nothing to report
		return 0;
	const uint32_t len = g.list_len[c];
	if (len == 0)
		return 0;
	const uint32_t from = g.list_begin[c];
	uint32_t n = 0;
	for (uint32_t j = 0; j < len; j++) {
		const int32_t p = g.list_pool[from + j];
		const int v = verdict(g, (uint32_t)p, o, T0, Tend);
		if (v != kKeep) {
			und += v == kUndecided;
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
__global__ __launch_bounds__(kThreads) void k_position(PosArgs g)
{
	__shared__ int32_t slice[kSliceMax];
	__shared__ uint32_t bounds[2];
	__shared__ uint32_t wave_cnt[kPer * kWaves];
	__shared__ uint32_t red[2 * kWaves];

	const uint32_t tid = threadIdx.x;
	const uint32_t m = min((uint32_t)g.pat_plane[0], g.max_records);
	const Share sh = share_of((m + kTile - 1) / kTile);
	const bool want_text = g.pos_ent && g.segments;   // (without windows no entry asks where its text lies)

	if (WRITE && sh.t_begin == sh.t_end && blockIdx.x != 0)   // nothing to write (a batch with few records)
		return;
	uint32_t base = 0;   // WRITE: cells written by the blocks in front of this one
	if (WRITE) {
		uint32_t total;
		base = blocks_before(g.block_counts, red, total);
		if (blockIdx.x == 0) {
			uint32_t u = 0;
			for (uint32_t j = tid; j < gridDim.x; j += kThreads)
				u += (uint32_t)g.block_counts[gridDim.x + j];
			u = block_sum(u, red);
			if (tid == 0) {
				const int32_t last = g.pat_plane[1 + m];   // the trailer is the input's
				write_ends(g.pat_out, g.cap, total, last);
				write_ends(g.off_out, g.cap, total, last);
				g.info[0] = (int32_t)u;
				g.info[1] = g.info[2] = g.info[3] = 0;
			}
		}
	}

	uint32_t kept = 0, und = 0;
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++) {
		const uint32_t r0 = t * kTile, r1 = min(r0 + kTile, m);
		int32_t off[kPer];
		uint32_t cell[kPer];
#pragma unroll
		for (int q = 0; q < kPer; q++) {   // loaded first: in flight while the slice is found and staged
			const uint32_t i = r0 + q * kThreads + tid;
			off[q] = i < r1 ? g.off_plane[1 + i] : 0;
			cell[q] = i < r1 ? (uint32_t)g.pat_plane[1 + i] : 0xFFFFFFFFu;
		}
		Slice st{};
		if (want_text) {
			st = stage_slice(g.off_plane, r0, r1, g.seg_start, g.segments, slice, bounds);
			__syncthreads();
		}
		// start number k of the array, from the staged slice where it holds it (k < segments)
		auto start_at = [&](uint32_t k) -> int64_t {
			return (st.in_lds && k >= st.k0 && k - st.k0 < st.len) ? slice[k - st.k0] : g.seg_start[k];
		};
		uint32_t cnt[kPer];
		int32_t head[kPer];
		int64_t T0[kPer], Tend[kPer];
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t i = r0 + q * kThreads + tid;
			head[q] = 0;
			cnt[q] = 0;
			T0[q] = g.lead_begin;
			Tend[q] = g.open_end;
			if (i >= r1)
				continue;
			if (want_text) {
				// starts <= the offset: in [0, segments] whatever the offset is
				const uint32_t ub = starts_le(st, slice, g.seg_start, g.segments, off[q]);
				if (ub > 0)
					T0[q] = start_at(ub - 1);
				if (ub < g.segments) {
					const int64_t next = start_at(ub);
					if (next <= g.text_end)
						Tend[q] = next;
				}
			}
			uint32_t u = 0;
			cnt[q] = one_record<false>(g, i, off[q], cell[q], T0[q], Tend[q], 0, head[q], u);
			kept += cnt[q];
			und += u;
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
				if (!g.all || !g.states) {
					if (d + 2 < g.cap) {
						g.pat_out[1 + d] = head[q];
						g.off_out[1 + d] = off[q];
					}
				} else {
					int32_t unused;
					uint32_t u;
					(void)one_record<true>(g, r0 + q * kThreads + tid, off[q], cell[q], T0[q], Tend[q], d, unused, u);
				}
			}
		}
		base += tile_total;
	}
	if (!WRITE) {
		kept = block_sum(kept, red);
		und = block_sum(und, red);
		if (tid == 0) {
			g.block_counts[blockIdx.x] = (int32_t)kept;
			g.block_counts[gridDim.x + blockIdx.x] = (int32_t)und;
		}
	}
}

}  // namespace

extern "C" size_t acm_position_workspace_bytes(size_t max_records)
{
	return round256(2 * (size_t)grid_for(max_records) * sizeof(int32_t));
}

extern "C" int acm_position_matches_async(const acm_dfa *d, const int32_t *d_pat_plane, const int32_t *d_off_plane,
    size_t max_records, int report, const int32_t *d_seg_start, size_t segments, long lead_begin, long text_end,
    long open_end, int all_patterns, int32_t *d_pat_out, int32_t *d_off_out, size_t out_capacity, int32_t *d_info,
    void *d_workspace, size_t workspace_bytes, void *stream)
{
	if (!d || !d_pat_plane || !d_off_plane || !d_pat_out || !d_off_out || !d_info || out_capacity < 2 ||
	    max_records > 0x7FFFFFFEul || (report != ACM_REPORT_HEAD && report != ACM_REPORT_STATE) ||
	    (segments && !d_seg_start) || segments > 0x7FFFFFFFul || (open_end != -1 && open_end < text_end))
		return acm::fail(ACM_ERR_ARG, "acm_position_matches_async: bad arguments");
	if (!d->d_pat_len && d->num_patterns)
		return acm::fail(ACM_ERR_ARG, "acm_position_matches_async: automaton has no pattern-length table");
	if (report == ACM_REPORT_STATE && (!d->d_list_begin || !d->d_list_len || !d->d_list_pool))
		return acm::fail(ACM_ERR_ARG, "acm_position_matches_async: automaton has no match lists");
	if (d->positioned && !d->d_pos_ent)
		return acm::fail(ACM_ERR_ARG, "acm_position_matches_async: positioned automaton without its window table");
	if (!d_workspace || workspace_bytes < acm_position_workspace_bytes(max_records))
		return acm::fail(ACM_ERR_ARG, "acm_position_matches_async: workspace %zu B < required %zu B", workspace_bytes,
		    acm_position_workspace_bytes(max_records));
	hipStream_t s = (hipStream_t)stream;
	ACM_HIP_TRY(hipSetDevice(d->device));
	PosArgs g;
	g.pat_plane = d_pat_plane;
	g.off_plane = d_off_plane;
	g.max_records = (uint32_t)max_records;
	g.states = report == ACM_REPORT_STATE;
	g.all = all_patterns != 0;
	g.seg_start = d_seg_start;
	g.segments = (uint32_t)segments;
	g.lead_begin = (int64_t)lead_begin;
	g.text_end = (int64_t)text_end;
	g.open_end = open_end == -1 ? kEndUnknown : (int64_t)open_end;
	g.list_begin = d->d_list_begin;
	g.list_len = d->d_list_len;
	g.list_pool = d->d_list_pool;
	g.pat_len = d->d_pat_len;
	g.pos_ent = d->positioned ? (const int4 *)d->d_pos_ent : nullptr;
	g.num_states = d->num_states;
	g.num_patterns = d->num_patterns;
	g.pat_out = d_pat_out;
	g.off_out = d_off_out;
	g.cap = clamp_cap(out_capacity);
	g.info = d_info;
	g.block_counts = (int32_t *)d_workspace;
	const uint32_t blocks = grid_for(max_records);
	hipLaunchKernelGGL(k_position<false>, dim3(blocks), dim3(kThreads), 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_position<true>, dim3(blocks), dim3(kThreads), 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}
