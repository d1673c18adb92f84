// The entry-filter layer on the record-pass core: what the passes that keep or drop match-list entries
// (word.hip, case.hip, position.hip, wildcard.hip, approx.hip) share.  Internal to the library, gfx950 only.  DESIGN.md 6f.
//
// Such a pass reads the planes of a scan (a cell and an offset per record), walks the match list of every
// record's state, keeps the entries a predicate of its own accepts and writes them in position order: the
// first kept entry of each record (head form) or all of them.  It is the two-launch ordered write of
// record_pass.h; entry_pass<WRITE> below is both launches, and a pass object supplies what is the pass's own:
//   bool head_form()       a record writes at most one cell, the head that record<false> found
//   uint32_t record<W>(row, i, o, c, d, head)
//                          the cells record i (offset o, input cell c) writes.  W, called where !head_form()
//                          and the count is not 0: writes them from cell 1 + d on.  !W is called for every row
//                          of the tile: behind the records (i >= r1) c is 0xFFFFFFFF, no state and no pattern
//   struct Row             what record<false> leaves for record<true> of the same record (EntryPass: nothing)
//   void ready()           once, before any other hook: a barrier, where the kernel staged something in LDS
//   void tile(r0, r1)      before the records [r0, r1) of a tile are counted (EntryPass: nothing)
//   void block0(red)       WRITE, every thread of block 0: what it writes beside header and trailer
//   void counted(red)      !WRITE, every thread, behind the tiles: a second per-block counter
#pragma once

#include "acm_internal.h"
#include "device_dfa.h"
#include "record_pass.h"

namespace acm_rp {

struct EntryArgs {
	// what a block without records reads lies in the first 64 bytes: one line of the argument segment
	const int32_t *cell_plane, *off_plane;   // the input: [0] the count, then the records, then the trailer
	uint32_t max_records;
	int all;
	int32_t *block_counts;                   // [gridDim.x] cells written; a pass may keep more behind them
	const uint32_t *list_begin, *list_len;
	const int32_t *list_pool;
	const uint32_t *pat_len;
	uint32_t num_states, num_patterns;
	int32_t *pat_out, *off_out;
	uint32_t cap;
};

// entry (p, o) into cell 1 + d of the output planes, where it lies in front of the trailer's cell
__device__ __forceinline__ void emit(const EntryArgs &g, uint32_t d, int32_t p, int32_t o)
{
	if (d + 2 < g.cap) {
		g.pat_out[1 + d] = p;
		g.off_out[1 + d] = o;
	}
}

// entries in the match list of s; 0 where s is no state (not the planes of a STATE scan: nothing to report)
__device__ __forceinline__ uint32_t list_len_of(const EntryArgs &g, uint32_t s)
{
	return s < g.num_states ? g.list_len[s] : 0u;
}

// One record of state s at offset o: the number of entries of its list that keep(p, o) accepts (p is a
// pattern of the automaton).  Head form: 0 or 1, and the first such pattern in head.  WRITE && all: the
// entries are written from cell 1 + d on.
template <bool WRITE, class Keep>
__device__ __forceinline__ uint32_t walk_list(const EntryArgs &g, int32_t o, uint32_t s, uint32_t d, int32_t &head, Keep keep)
{
	const uint32_t len = list_len_of(g, s);
	if (len == 0)
		return 0;
	const uint32_t from = g.list_begin[s];
	uint32_t n = 0;
	for (uint32_t j = 0; j < len; j++) {
		const int32_t p = g.list_pool[from + j];
		if ((uint32_t)p >= g.num_patterns || !keep((uint32_t)p, o))
			continue;
		if (!g.all) {
			head = p;
			return 1;
		}
		if (WRITE)
			emit(g, d + n, p, o);
		n++;
	}
	return n;
}

// the hooks a pass need not have
struct EntryPass {
	struct Row {};
	__device__ __forceinline__ void ready() {}
	__device__ __forceinline__ void tile(uint32_t, uint32_t) {}
	__device__ __forceinline__ void block0(uint32_t *) {}
	__device__ __forceinline__ void counted(uint32_t *) {}
};

// The body of k_<pass><WRITE>, called by every thread.  wave_cnt: kPer * kWaves cells of LDS, red: 2 * kWaves.
template <bool WRITE, class Pass>
__device__ __forceinline__ void entry_pass(const EntryArgs &g, Pass &pass, uint32_t *wave_cnt, uint32_t *red)
{
	const uint32_t tid = threadIdx.x;
	const uint32_t m = min((uint32_t)g.cell_plane[0], g.max_records);
	const Share sh = share_of((m + kTile - 1) / kTile);
	pass.ready();   // (behind the count cell's load, which a barrier in front of it would hold up)

	if (WRITE && sh.t_begin == sh.t_end && blockIdx.x != 0)   // nothing to write (a batch with few records)
		return;
	uint32_t base = 0;   // WRITE: cells written by the blocks in front of this one
	if (WRITE) {
		uint32_t total;
		base = blocks_before(g.block_counts, red, total);
		if (blockIdx.x == 0) {
			if (tid == 0) {
				const int32_t last = g.cell_plane[1 + m];   // the trailer is the input's
				write_ends(g.pat_out, g.cap, total, last);
				write_ends(g.off_out, g.cap, total, last);
			}
			pass.block0(red);
		}
	}

	uint32_t kept = 0;
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++) {
		const uint32_t r0 = t * kTile, r1 = min(r0 + kTile, m);
		int32_t off[kPer];
		uint32_t cell[kPer];
#pragma unroll
		for (int q = 0; q < kPer; q++) {   // loaded first: in flight while the pass prepares the tile
			const uint32_t i = r0 + q * kThreads + tid;
			off[q] = i < r1 ? g.off_plane[1 + i] : 0;
			cell[q] = i < r1 ? (uint32_t)g.cell_plane[1 + i] : 0xFFFFFFFFu;
		}
		pass.tile(r0, r1);
		uint32_t cnt[kPer];
		int32_t head[kPer];
		typename Pass::Row row[kPer];
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t i = r0 + q * kThreads + tid;
			head[q] = 0;
			cnt[q] = pass.template record<false>(row[q], i, off[q], cell[q], 0, head[q]);
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
				if (pass.head_form())
					emit(g, d, head[q], off[q]);
				else
					(void)pass.template record<true>(row[q], r0 + q * kThreads + tid, off[q], cell[q], d, head[q]);
			}
		}
		base += tile_total;
	}
	if (!WRITE) {
		kept = block_sum(kept, red);
		pass.counted(red);   // (in front of the store: a barrier behind a store waits for it)
		if (tid == 0)
			g.block_counts[blockIdx.x] = (int32_t)kept;
	}
}

// ---- before ++ text: the bytes a pass may look at (word.hip, case.hip, wildcard.hip) ----

struct TextWindow {
	const uint8_t *text;     // byte at offset text_origin + i
	int64_t text_origin, text_end;
	const uint8_t *before;   // bytes at [text_origin - before_len, text_origin)
	int64_t before_len;
	uint8_t *tail_out;       // null, or the last tail_len bytes of before ++ text: the next piece's before
	uint32_t tail_len;
};

// the byte at stream offset p of before ++ text.  The caller has checked that p lies in it.
__device__ __forceinline__ uint32_t window_byte(const TextWindow &w, int64_t p)
{
	return p >= w.text_origin ? w.text[p - w.text_origin] : w.before[p - (w.text_origin - w.before_len)];
}

// called by every thread of one block
__device__ __forceinline__ void write_tail(const TextWindow &w)
{
	if (w.tail_out)
		for (uint32_t j = threadIdx.x; j < w.tail_len; j += kThreads)
			w.tail_out[j] = (uint8_t)window_byte(w, w.text_end - (int64_t)w.tail_len + j);
}

// ---- host side ----

inline bool window_ok(const void *d_text, long text_origin, long text_end, const void *d_before, size_t before_len)
{
	return text_end >= text_origin && (text_end == text_origin || d_text) && (!before_len || d_before) &&
	       before_len <= 0x7FFFFFFFul;
}

inline TextWindow window_of(const acm_dfa *d, const void *d_text, long text_origin, long text_end, const void *d_before,
    size_t before_len, void *d_tail_out)
{
	const int64_t len = (int64_t)before_len + (text_end - text_origin);
	return TextWindow{ (const uint8_t *)d_text, (int64_t)text_origin, (int64_t)text_end, (const uint8_t *)d_before,
		(int64_t)before_len, (uint8_t *)d_tail_out, (uint32_t)std::min<int64_t>((int64_t)d->max_pattern_len, len) };
}

// what every entry point is called with
struct EntryCall {
	const acm_dfa *d;
	const int32_t *cell_plane, *off_plane;
	size_t max_records;
	int all_patterns;
	int32_t *pat_out, *off_out;
	size_t out_capacity;
	void *workspace;
	size_t workspace_bytes;
};

// null, or what is wrong with the tables of an entry point's own: check(d) where there is a d
template <class Check>
inline const char *tables_error(const acm_dfa *d, Check check)
{
	return d ? check(*d) : nullptr;
}

// The checks the entry points share, in the order and with the texts they have had, then e filled.  fn: the
// entry point's name.  own_ok: its own arguments are fine.  tables: tables_error().  need: its workspace.
inline int entry_args(EntryArgs &e, const char *fn, const EntryCall &c, bool own_ok, const char *tables, size_t need)
{
	const acm_dfa *d = c.d;
	if (!d || !c.cell_plane || !c.off_plane || !c.pat_out || !c.off_out || c.out_capacity < 2 ||
	    c.max_records > 0x7FFFFFFEul || !own_ok)
		return acm::fail(ACM_ERR_ARG, "%s: bad arguments", fn);
	if (!d->d_pat_len && d->num_patterns)
		return acm::fail(ACM_ERR_ARG, "%s: automaton has no pattern-length table", fn);
	if (tables)
		return acm::fail(ACM_ERR_ARG, "%s: %s", fn, tables);
	if (!c.workspace || c.workspace_bytes < need)
		return acm::fail(ACM_ERR_ARG, "%s: workspace %zu B < required %zu B", fn, c.workspace_bytes, need);
	e = EntryArgs{ c.cell_plane, c.off_plane, (uint32_t)c.max_records, c.all_patterns != 0, (int32_t *)c.workspace,
		d->d_list_begin, d->d_list_len, d->d_list_pool, d->d_pat_len, d->num_states, d->num_patterns, c.pat_out, c.off_out,
		clamp_cap(c.out_capacity) };
	return ACM_OK;
}

// the two launches of a pass over at most max_records records, on the automaton's device
template <class Args>
inline int launch_passes(void (*count)(Args), void (*write)(Args), const acm_dfa *d, size_t max_records, const Args &g,
    void *stream)
{
	ACM_HIP_TRY(hipSetDevice(d->device));
	const dim3 blocks(grid_for(max_records));
	hipLaunchKernelGGL(count, blocks, dim3(kThreads), 0, (hipStream_t)stream, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(write, blocks, dim3(kThreads), 0, (hipStream_t)stream, g);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}

}  // namespace acm_rp
