// Rules: boolean conditions over the sequences that hit one text.  gfx950 only.  DESIGN.md 6k.
//
// A rule (acm_automaton_add_rule, include/acmatch.h) is operands -- sequence indices -- and an expression over
// their counts in one text.  The input is the output of the sequence pass: (sequence, end offset) records in
// offset order.  A record at offset o lies in text k = (starts <= o) - 1, the lead text -1.  Out: one record
// (rule, text, offset) per (rule, text) whose expression is true, at the position of its TRIGGER: the first
// record in that text of the rule's lowest-numbered operand that occurs there.
//
// Tables (device_dfa.hip, only for a set with rules): a SLOT is an operand of a rule, numbered rule-major.
// d_rule_ent[sequence] = slot or -1; d_rule_slot[s] = {rule, operand}; d_rule_tab[r] = {first slot, operands,
// program begin, program cells}; d_rule_prog: the postfix programs, {op, argument} cells (acm::RuleOp).
//
// Ordered stably by slot, the records of every slot are a contiguous list still in offset order, so their text
// indices do not decrease: the count of an operand in a text is two binary searches in that list.  Launches, on
// the record-pass grid (record_pass.h) over n = max_records cells:
//   k_rule_key           per cell: sort key (slot, or all-ones: no operand, or behind the count), its index, its
//                        text index + 1 (the tile's starts staged in LDS, as the sequence pass) and emit[] = 0;
//                        every slot's range of ordered cells is set empty
//   k_radix_hist / k_radix_offsets / k_radix_scatter   (radix_pass.h, shared with sequence.hip)
//                        1 to 4 stable radix passes of 8 bits: ceil(bits(slots) / 8)
//   k_rule_bounds        an ordered cell whose neighbour has another key begins or ends its slot's range: no
//                        search, no loop; the text indices gathered in order
//   k_rule_eval          an ordered cell whose predecessor has another slot or another text heads an (operand,
//                        text) run.  If a lower-numbered operand of its rule occurs in its text another head is the
//                        trigger; otherwise it runs the program and sets emit[its input index]
//   k_rule_emit<write>   the core's count and write launches over the input order (emit_flagged, radix_pass.h)
// 5 + 3 * passes launches, whatever the planes hold.  No atomics decide an order.  Every index that is read from
// memory is bounded before it is used.  The evaluation stack is acm::kRuleStack entries in registers: pushes and
// pops shift it, so that every index is a constant (a runtime-indexed private array would go to scratch).
#include <hip/hip_runtime.h>

#include "acm_internal.h"
#include "device_dfa.h"
#include "radix_pass.h"
#include "record_pass.h"

namespace {

using namespace acm_rp;

struct RuleArgs {
	const int32_t *seq_plane, *off_plane;   // the input: [0] the count, then the records, then the trailer
	uint32_t n;                             // max_records: the cells that are keyed and ordered
	const int32_t *seg_start;
	uint32_t segments;
	const int32_t *ent;                     // [sequences] slot or -1
	const int2 *slot_tab;                   // [slots] {rule, operand}
	const int4 *rule_tab;                   // [rules] {first slot, operands, program begin, program cells}
	const int2 *prog;                       // [prog_cells] {op, argument}
	uint32_t sequences, slots, rules, prog_cells;
	// workspace
	uint32_t *text;                         // [n] by input index: text index + 1, 0: the lead text
	uint32_t *key_in, *val_in;              // the cells as keyed; keys/vals: the ordered cells
	const uint32_t *keys, *vals;
	uint32_t *stext;                        // [n] in slot order: text[vals[]]
	uint32_t *emit;                         // [n] by input index: 1: the trigger of a rule that holds
	uint2 *slot_range;                      // [slots] the ordered cells [x, y) of each slot
	uint32_t *operands;                     // [1] the ordered cells that have a slot
	int32_t *counts;                        // [gridDim.x] block counts of the emit step
	int32_t *heads, *evals;                 // [gridDim.x] block counts of k_rule_eval: run heads, programs run
	// output
	int32_t *rule_out, *text_out, *off_out;
	uint32_t cap;
	int32_t *info;
};

__device__ __forceinline__ uint32_t records_of(const RuleArgs &g) { return min((uint32_t)g.seq_plane[0], g.n); }

// the slot of input cell i < records_of, or kNoKey
__device__ __forceinline__ uint32_t slot_of(const RuleArgs &g, uint32_t i)
{
	const uint32_t q = (uint32_t)g.seq_plane[1 + i];
	const int32_t slot = q < g.sequences ? g.ent[q] : -1;
	return (slot >= 0 && (uint32_t)slot < g.slots) ? (uint32_t)slot : kNoKey;
}

__global__ __launch_bounds__(kThreads) void k_rule_key(RuleArgs g)
{
	__shared__ int32_t slice[kSliceMax];
	__shared__ uint32_t bounds[2];

	const uint32_t tid = threadIdx.x;
	for (uint32_t s = blockIdx.x * kThreads + tid; s < g.slots; s += gridDim.x * kThreads)
		g.slot_range[s] = make_uint2(0, 0);
	if (blockIdx.x == 0 && tid == 0)
		g.operands[0] = 0;
	const uint32_t m = records_of(g);
	const Share sh = share_of((g.n + kTile - 1) / kTile);
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++) {
		const uint32_t r0 = t * kTile, r1 = min(r0 + kTile, m);   // (r1 <= r0: a tile behind the records)
		const bool want_text = g.segments && r1 > r0;
		Slice st{};
		if (want_text) {
			st = stage_slice(g.off_plane, r0, r1, g.seg_start, g.segments, slice, bounds);
			__syncthreads();
		}
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t i = r0 + q * kThreads + tid;
			if (i >= g.n)
				continue;
			uint32_t key = kNoKey, text = 0;
			if (i < r1) {
				key = slot_of(g, i);
				if (key != kNoKey && want_text)
					text = min(starts_le(st, slice, g.seg_start, g.segments, g.off_plane[1 + i]), g.segments);
			}
			g.key_in[i] = key;
			g.val_in[i] = i;
			g.text[i] = text;
			g.emit[i] = 0;
		}
	}
}

// ---- the ordered cells: the range of every slot, and the text indices in order ----

__global__ __launch_bounds__(kThreads) void k_rule_bounds(RuleArgs g)
{
	const uint32_t tid = threadIdx.x;
	const Share sh = share_of((g.n + kTile - 1) / kTile);
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++)
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t i = t * kTile + q * kThreads + tid;
			if (i >= g.n)
				continue;
			const uint32_t key = g.keys[i], at = g.vals[i];
			const uint32_t prev = i > 0 ? g.keys[i - 1] : kNoKey, next = i + 1 < g.n ? g.keys[i + 1] : kNoKey;
			const bool has = key < g.slots;   // (or key == kNoKey)
			g.stext[i] = (has && at < g.n) ? g.text[at] : 0;
			if (has && (i == 0 || prev != key))
				g.slot_range[key].x = i;
			if (has && (i + 1 == g.n || next != key)) {
				g.slot_range[key].y = i + 1;
				if (i + 1 == g.n || next >= g.slots)
					g.operands[0] = i + 1;
			}
		}
}

// ---- the rules ----

// occurrences in text t (index + 1) of the operand with this slot
__device__ __forceinline__ uint32_t count_in_text(const RuleArgs &g, uint32_t slot, uint32_t t)
{
	if (slot >= g.slots)
		return 0;
	const uint2 r = g.slot_range[slot];
	const uint32_t x = min(r.x, g.n), y = min(r.y, g.n);
	if (y <= x)
		return 0;
	const uint32_t a = lower_bound_u32(g.stext + x, y - x, t);
	return lower_bound_u32(g.stext + x + a, y - x - a, t + 1);   // (t <= segments < 2^31)
}

// the rule's program over the counts of text t: is the expression true?
__device__ __forceinline__ bool run_program(const RuleArgs &g, const int4 rule, uint32_t t)
{
	int64_t c[acm::kRuleStack];
	uint32_t truth = 0;   // bit k: the truth of stack entry k, entry 0 the top
#pragma unroll
	for (int k = 0; k < acm::kRuleStack; k++)
		c[k] = 0;
	const uint32_t pb = min((uint32_t)rule.z, g.prog_cells), pe = pb + min((uint32_t)rule.w, g.prog_cells - pb);
	for (uint32_t pc = pb; pc < pe; pc++) {
		const int2 ins = g.prog[pc];
		if (ins.x == acm::kRulePush) {
			const uint32_t op = (uint32_t)ins.y;
			const int64_t v = op < (uint32_t)rule.y ? (int64_t)count_in_text(g, (uint32_t)rule.x + op, t) : 0;
#pragma unroll
			for (int k = acm::kRuleStack - 1; k > 0; k--)
				c[k] = c[k - 1];
			c[0] = v;
			truth = truth << 1 | (v > 0);
		} else if (ins.x == acm::kRuleAnd || ins.x == acm::kRuleOr) {
			const uint32_t b = truth & 1, a = truth >> 1 & 1;
			c[0] += c[1];
#pragma unroll
			for (int k = 1; k + 1 < acm::kRuleStack; k++)
				c[k] = c[k + 1];
			truth = (truth >> 1 & ~1u) | (ins.x == acm::kRuleAnd ? a & b : a | b);
		} else {
			const int64_t v = c[0], n = ins.y;
			const bool is = ins.x == acm::kRuleEq ? v == n : ins.x == acm::kRuleGt ? v > n : ins.x == acm::kRuleLt ? v < n : false;
			truth = (truth & ~1u) | is;
		}
	}
	return truth & 1;
}

__global__ __launch_bounds__(kThreads) void k_rule_eval(RuleArgs g)
{
	__shared__ uint32_t red[kWaves];

	const uint32_t tid = threadIdx.x;
	const uint32_t m = records_of(g);
	const uint32_t cells = min(g.operands[0], g.n);
	const Share sh = share_of((cells + kTile - 1) / kTile);
	uint32_t heads = 0, evals = 0;
	for (uint32_t t = sh.t_begin; t < sh.t_end; t++)
#pragma unroll
		for (int q = 0; q < kPer; q++) {
			const uint32_t i = t * kTile + q * kThreads + tid;
			if (i >= cells)
				continue;
			const uint32_t slot = g.keys[i], text = g.stext[i], at = g.vals[i];
			if (slot >= g.slots || at >= m)   // (never: the cells in front of operands[0] have a slot)
				continue;
			if (i > 0 && g.keys[i - 1] == slot && g.stext[i - 1] == text)
				continue;
			heads++;
			const int2 sl = g.slot_tab[slot];   // {rule, operand}
			if ((uint32_t)sl.x >= g.rules)
				continue;
			const int4 rule = g.rule_tab[sl.x];   // {first slot, operands, program begin, program cells}
			bool lower = false;
			for (uint32_t j = 0; j < (uint32_t)sl.y && !lower; j++)
				lower = count_in_text(g, (uint32_t)rule.x + j, text) > 0;
			if (lower)
				continue;
			evals++;
			if (run_program(g, rule, text))
				g.emit[at] = 1;
		}
	heads = block_sum(heads, red);
	evals = block_sum(evals, red);
	if (tid == 0) {
		g.heads[blockIdx.x] = (int32_t)heads;
		g.evals[blockIdx.x] = (int32_t)evals;
	}
}

// ---- the records, in input order ----

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void k_rule_emit(RuleArgs g)
{
	__shared__ uint32_t wave_cnt[kPer * kWaves];
	__shared__ uint32_t red[2 * kWaves];

	const uint32_t m = records_of(g);
	uint32_t heads = 0, evals = 0;
	if (WRITE && blockIdx.x == 0) {   // the block that writes the info sums k_rule_eval's block counts
		for (uint32_t b = threadIdx.x; b < gridDim.x; b += kThreads) {
			heads += (uint32_t)g.heads[b];
			evals += (uint32_t)g.evals[b];
		}
		heads = block_sum(heads, red);
		evals = block_sum(evals, red);
	}
	emit_flagged<WRITE>(
	    g.emit, m, g.counts, g.cap, wave_cnt, red,
	    [&](uint32_t total) {
		    const int32_t last = g.seq_plane[1 + m];   // the trailer is the input's
		    write_ends(g.rule_out, g.cap, total, last);
		    write_ends(g.text_out, g.cap, total, last);
		    write_ends(g.off_out, g.cap, total, last);
		    g.info[0] = (int32_t)min(g.operands[0], g.n);
		    g.info[1] = (int32_t)heads;
		    g.info[2] = (int32_t)evals;
		    g.info[3] = 0;
	    },
	    [&](uint32_t i, uint32_t d) {
		    const uint32_t slot = slot_of(g, i);
		    g.rule_out[1 + d] = slot != kNoKey ? g.slot_tab[slot].x : -1;
		    g.text_out[1 + d] = (int32_t)g.text[i] - 1;
		    g.off_out[1 + d] = g.off_plane[1 + i];
	    });
}

// a set without rules: no record
__global__ void k_rule_none(RuleArgs g)
{
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		const int32_t last = g.seq_plane[1 + records_of(g)];
		write_ends(g.rule_out, g.cap, 0, last);
		write_ends(g.text_out, g.cap, 0, last);
		write_ends(g.off_out, g.cap, 0, last);
		g.info[0] = g.info[1] = g.info[2] = g.info[3] = 0;
	}
}

// ---- host side ----

struct Layout {
	size_t text, key[2], val[2], stext, emit, hist, digit_total, slot_range, operands, counts, heads, evals, total;
};

Layout layout_of(size_t n, uint32_t blocks, uint32_t slots)
{
	Layout l;
	size_t at = 0;
	auto take = [&](size_t bytes) {
		const size_t here = at;
		at += round256(bytes);
		return here;
	};
	l.text = take(n * sizeof(uint32_t));
	for (int k = 0; k < 2; k++) {
		l.key[k] = take(n * sizeof(uint32_t));
		l.val[k] = take(n * sizeof(uint32_t));
	}
	l.stext = take(n * sizeof(uint32_t));
	l.emit = take(n * sizeof(uint32_t));
	l.hist = take(radix_hist_bytes(blocks));
	l.digit_total = take(radix_digit_total_bytes());
	l.slot_range = take((size_t)slots * sizeof(uint2));
	l.operands = take(sizeof(uint32_t));
	l.counts = take((size_t)blocks * sizeof(int32_t));
	l.heads = take((size_t)blocks * sizeof(int32_t));
	l.evals = take((size_t)blocks * sizeof(int32_t));
	l.total = std::max<size_t>(at, 256);
	return l;
}

}  // namespace

extern "C" size_t acm_rule_workspace_bytes(const acm_dfa *d, size_t max_records)
{
	return layout_of(max_records, grid_for(max_records), d ? d->rule_slots : 0).total;
}

extern "C" int acm_rule_matches_async(const acm_dfa *d, const int32_t *d_seq_plane, const int32_t *d_off_plane, size_t max_records,
    const int32_t *d_seg_start, size_t segments, int32_t *d_rule_out, int32_t *d_text_out, int32_t *d_off_out, size_t out_capacity,
    int32_t *d_info, void *d_workspace, size_t workspace_bytes, void *stream)
{
	if (!d || !d_seq_plane || !d_off_plane || !d_rule_out || !d_text_out || !d_off_out || !d_info || out_capacity < 2 ||
	    max_records > 0x7FFFFFFEul || (segments && !d_seg_start) || segments > 0x7FFFFFFFul)
		return acm::fail(ACM_ERR_ARG, "acm_rule_matches_async: bad arguments");
	if (d->rule_slots && (!d->d_rule_ent || !d->d_rule_slot || !d->d_rule_tab || !d->d_rule_prog))
		return acm::fail(ACM_ERR_ARG, "acm_rule_matches_async: automaton with rules without their tables");
	const uint32_t blocks = grid_for(max_records);
	const Layout l = layout_of(max_records, blocks, d->rule_slots);
	if (!d_workspace || workspace_bytes < l.total)
		return acm::fail(ACM_ERR_ARG, "acm_rule_matches_async: workspace %zu B < required %zu B", workspace_bytes, l.total);

	char *ws = (char *)d_workspace;
	RuleArgs g{};
	g.seq_plane = d_seq_plane;
	g.off_plane = d_off_plane;
	g.n = (uint32_t)max_records;
	g.seg_start = d_seg_start;
	g.segments = (uint32_t)segments;
	g.ent = d->d_rule_ent;
	g.slot_tab = (const int2 *)d->d_rule_slot;
	g.rule_tab = (const int4 *)d->d_rule_tab;
	g.prog = (const int2 *)d->d_rule_prog;
	g.sequences = d->rule_sequences;
	g.slots = d->rule_slots;
	g.rules = d->num_rules;
	g.prog_cells = d->rule_prog_cells;
	g.text = (uint32_t *)(ws + l.text);
	g.stext = (uint32_t *)(ws + l.stext);
	g.emit = (uint32_t *)(ws + l.emit);
	g.slot_range = (uint2 *)(ws + l.slot_range);
	g.operands = (uint32_t *)(ws + l.operands);
	g.counts = (int32_t *)(ws + l.counts);
	g.heads = (int32_t *)(ws + l.heads);
	g.evals = (int32_t *)(ws + l.evals);
	g.rule_out = d_rule_out;
	g.text_out = d_text_out;
	g.off_out = d_off_out;
	g.cap = clamp_cap(out_capacity);
	g.info = d_info;

	ACM_HIP_TRY(hipSetDevice(d->device));
	hipStream_t s = (hipStream_t)stream;
	const dim3 grid(blocks), block(kThreads);
	if (!d->rule_slots) {
		hipLaunchKernelGGL(k_rule_none, dim3(1), dim3(64), 0, s, g);
		ACM_HIP_TRY(hipGetLastError());
		return ACM_OK;
	}
	uint32_t *const key[2] = { (uint32_t *)(ws + l.key[0]), (uint32_t *)(ws + l.key[1]) };
	uint32_t *const val[2] = { (uint32_t *)(ws + l.val[0]), (uint32_t *)(ws + l.val[1]) };
	g.key_in = key[0];
	g.val_in = val[0];
	hipLaunchKernelGGL(k_rule_key, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	int cur = 0;   // the buffers that hold the ordered cells
	ACM_HIP_TRY(radix_order(g.n, key, val, (uint32_t *)(ws + l.hist), (uint32_t *)(ws + l.digit_total), radix_passes(d->rule_slots),
	    blocks, s, cur));
	g.keys = key[cur];
	g.vals = val[cur];
	hipLaunchKernelGGL(k_rule_bounds, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_rule_eval, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_rule_emit<false>, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_rule_emit<true>, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}
