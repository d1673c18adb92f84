// The scan pipeline: speculative chain walk -> boundary resolve -> block scan
// of per-chain counts -> ordered scatter.  gfx950 only.
//
// Replaces ahomatch.cl:1-165 (+ its launch, ocl_aho_match.c:96-131) and the
// prefix-sum/compaction stage behind it (databuf.c:648-651), with the serial
// semantics of SURVEY App. B.1: one record per text position whose transition
// enters a final state, each position exactly once, in position order.
//
// How a serial DFA walk is made parallel without a per-lane warm-up:
//
//   The text is cut into chains of S bytes (S = 16..256, a power of two).
//
//   K1 k_spec_walk   every lane walks its chains from the ROOT state.  The
//                    state reached after m bytes equals the true serial state
//                    as soon as the true state's depth is <= m (a state only
//                    remembers its last depth bytes); from then on the two
//                    walks coincide.  K1 records the end state e[j], the
//                    tentative hits (staged per wave), their number and the
//                    step of the first one.  Its tile epilogue already settles
//                    the common case of the next two stages (see below).
//   K2a k_probe      lane c walks chain c from e[c-1] -- the state chain c
//                    starts in whenever chain c-1 has merged -- until the
//                    depth test says it has merged with chain c's own root
//                    walk: typically after one byte.
//   K2b k_resolve    lane j: if every chain of its look-back window
//                    (q = ceil(L/S) chains) merged in its probe, the true
//                    start state is known without walking and K1's records
//                    stand.  Otherwise it rebuilds the start state by walking
//                    (re-using probe results wherever the walk enters a chain
//                    in the state the probe assumed), re-walks the head of
//                    its own chain from the true state, stages the true hits
//                    and, if a K1 hit lies in the unmerged head, takes the
//                    whole chain over (K1's records for it are dropped).
//                    Worst case (q-1)*S + S steps: the price of a classic
//                    (L-1)-byte halo, paid only where the text really is deep
//                    inside a pattern.
//   k_scan_top + k_scatter_all   per-chain counts -> offsets -> records land
//                    in position order; pattern index = out[state] is looked
//                    up here, off the walk's critical path.
//
// Deep walks (K2) get everything about the state they enter with the state
// itself: deep[idx] = state | depth << 32 | run << 48.  depth feeds the merge
// test; run is the length of the unary trie path ahead, along which states
// are consecutive ids and the walk only compares text with in_byte[] --
// 16 bytes per load level instead of one table lookup per byte.  (A nocase
// automaton: that compare is the one place the text is folded, k_probe /
// k_resolve<NOCASE = true>; the tables fold everything else.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "acm_internal.h"
#include "chain.h"
#include "deep_walk.h"
#include "device_dfa.h"
#include "sparse.h"

namespace {

using acm_dev::ChainText;
using acm_dev::Deep;
using acm_dev::deep_step;
using acm_dev::fast_forward;

constexpr int kBlock1 = 1024;          // K1 workgroup: 16 waves, one per CU (LDS bound)
constexpr int kWaves1 = kBlock1 / 64;
constexpr int kBlock2 = 256;
constexpr uint32_t kNoFirst = 0xFFFFu;
constexpr uint8_t kProbeTodo = 0xFF;

struct ScanArgs {
	const uint32_t *cold;   // [states][1 << ls] next state, a cell per byte class
	const uint64_t *deep;   // [states][1 << ls] next | depth(next) << 32 | run(next) << 48
	const uint16_t *hot;    // [H][1 << ls]
	const uint8_t *cls;     // [256] byte -> class (the identity when ls == 8)
	uint32_t ls;            // log2 of the cells per row
	uint32_t halo_bytes;    // halo mode (below, walk_tile): bytes every chain walks in front of its own; else 0
	uint32_t halo_mode;
	uint32_t halo_pre;      // halo mode: the chains' text is loaded up front (k_halo_walk)
	const int32_t *out;
	const uint32_t *dev2ref;
	const uint8_t *in_byte;
	const uint4 *text16;
	const uint8_t *text;
	uint32_t n;             // text bytes
	uint32_t n_pad;         // n rounded up to 16 (readable)
	uint32_t S, logS;       // chain bytes
	uint32_t n_chains;
	uint32_t n_tiles;       // K1 wave tiles
	uint32_t H;             // hot rows
	uint32_t hot_depth1;    // hot ids below this have depth <= 1
	uint32_t F;             // first final dev id
	uint32_t L;             // max pattern length
	uint32_t q;             // look-back chains
	uint32_t init_state;    // dev numbering
	const uint32_t *init_ptr;   // not null: the state to start in is THERE (handed over on the device, k_carry_init), init_state is not
	uint32_t drop_before;   // records ending before this offset are context (halo), not output
	int32_t off_shift;      // added to every reported offset
	// workspace
	uint32_t *end_state;    // [chains] e[j]: end state of chain j's root walk
	uint32_t *c1f;          // [chains] K1 hit count | first-hit step << 16
	uint32_t *k2info;       // [chains] K2 hit count | K1 records dropped << 16
	uint32_t *wend;         // [chains] end state of the probe walk of chain c from e[c-1]
	uint8_t *probe;         // [chains] bit0 probe merged, bit1 head needs an emission walk
	uint8_t *rflag;         // [chains] 1: resolved by the walk kernel's epilogue
	int32_t *cnt;           // [chains] final record count of the chain
	int32_t *off;           // [blocks] per-256-chain totals, scanned in place
	uint32_t *wave_cnt1;
	uint32_t *wave_cnt2;
	uint32_t *misc;         // [0] last state (dev), [1] total records, [2] which pipeline produced the planes
	uint2 *stage1;
	uint2 *stage2;
	// output
	int32_t *pat_plane;
	int32_t *off_plane;
	uint32_t plane_capacity;
	uint32_t fold_blocks;      // > 0: off[] holds the raw totals of this many blocks; the scatter adds them up itself
};

// the state the text starts in (wave-uniform: one scalar load where it was handed over on the device)
__device__ __forceinline__ uint32_t init_of(const ScanArgs &a)
{
	return a.init_ptr ? *a.init_ptr : a.init_state;
}

__device__ __forceinline__ uint32_t mbcnt64(uint64_t m)
{
	return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

__device__ __forceinline__ uint32_t cold_next(const ScanArgs &a, uint32_t idx)
{
	return a.cold[idx];
}

template <int K>
__device__ __forceinline__ uint32_t byte_of(const uint4 &w)
{
	const uint32_t d = (K < 4) ? w.x : (K < 8) ? w.y : (K < 12) ? w.z : w.w;
	return (d >> (8 * (K & 3))) & 0xFFu;
}

// ---------------------------------------------------------------------------
// K1
// ---------------------------------------------------------------------------

// One DFA step for C independent chains, loads issued back to back so the
// chains hide each other's latency.  Cold lanes (state beyond the LDS rows,
// or an LDS cell that says "look in HBM") gather from the cold plane; the
// branch around that is wave-uniform.  (Issuing the HBM gather before the LDS
// result is known -- the plane a lane needs only depends on its state --
// measured 35% SLOWER on MI355X, so the gather waits for the LDS cell.)
template <int C, int K, bool GUARD, bool CLS, bool HALO>
__device__ __forceinline__ void step_all(const ScanArgs &a, const uint16_t *hot, const uint8_t *clsmap, uint32_t ls,
    const uint4 (&w)[C],
    uint32_t (&st)[C], uint32_t (&cnt)[C], uint32_t (&first)[C], const uint32_t (&base)[C],
    const uint32_t (&len)[C], const uint32_t (&lead)[C], uint32_t hb, uint32_t g, uint32_t &wcount, uint2 *stage)
{
	uint32_t idx[C], e[C];
	bool need[C];
	bool any_need = false;
#pragma unroll
	for (int c = 0; c < C; c++) {
		const uint32_t b = byte_of<K>(w[c]);
		idx[c] = CLS ? (st[c] << ls) | clsmap[b] : (st[c] << 8) | b;   // (the class of a byte: one more LDS read, off the chain)
		e[c] = hot[st[c] < a.H ? idx[c] : 0u];
	}
#pragma unroll
	for (int c = 0; c < C; c++) {
		need[c] = (st[c] >= a.H) | (e[c] == acm::kHotSentinel);
		any_need |= need[c];
	}
	if (__builtin_amdgcn_ballot_w64(any_need)) {
		uint32_t v[C];
#pragma unroll
		for (int c = 0; c < C; c++)
			v[c] = cold_next(a, need[c] ? idx[c] : 0u);
#pragma unroll
		for (int c = 0; c < C; c++)
			e[c] = need[c] ? v[c] : e[c];
	}
	// 1-based step inside the chain; in halo mode the first hb bytes of the walk lie in front of
	// the chain (steps <= 0): they only bring the state up to date
	const int32_t step = (int32_t)(g * 16 + K + 1) - (HALO ? (int32_t)hb : 0);
	bool hit[C];
	bool any_hit = false;
#pragma unroll
	for (int c = 0; c < C; c++) {
		if (GUARD && (step > (int32_t)len[c] || (HALO && step <= -(int32_t)lead[c])))
			e[c] = st[c];  // past the end of the text, or in front of where this chain's walk starts: freeze
		hit[c] = (e[c] >= a.F) && (!HALO || step >= 1) && (!GUARD || step <= (int32_t)len[c]);
		any_hit |= hit[c];
	}
	if (__builtin_amdgcn_ballot_w64(any_hit)) {
#pragma unroll
		for (int c = 0; c < C; c++) {
			hit[c] = hit[c] && (base[c] + (uint32_t)step - 1 >= a.drop_before);
			const uint64_t m = __builtin_amdgcn_ballot_w64(hit[c]);
			if (m) {
				if (hit[c]) {
					stage[wcount + mbcnt64(m)] =
					    make_uint2(base[c] + (uint32_t)step - 1, e[c] | (cnt[c] << 24));
					if (cnt[c] == 0)
						first[c] = (uint32_t)step;
					cnt[c]++;
				}
				wcount += (uint32_t)__popcll(m);
			}
		}
	}
#pragma unroll
	for (int c = 0; c < C; c++)
		st[c] = e[c];
}

// End of a wave tile: the common case of the boundary resolve, done where the
// data already is.  Lane l holds e[chain], its left neighbour holds e[chain-1]
// (a shuffle away), the first text byte of the chain is still in a register
// and the hot rows are in LDS -- so the probe's first step (does the walk from
// e[chain-1] merge with this chain's own root walk after one byte?) costs one
// LDS lookup.  A chain whose probe merges that way, and whose look-back window
// is made of such chains, is final: count = K1 count, nothing to re-walk.
// Everything else is left to k_probe / k_resolve through the flag arrays.
template <int C>
__device__ __forceinline__ void tile_epilogue(const ScanArgs &a, const uint16_t *hot, uint32_t ls, uint32_t wt,
    uint32_t lane, const uint32_t (&st)[C], const uint32_t (&cnt)[C], const uint32_t (&chain)[C],
    const uint32_t (&fb)[C])
{
	bool decided[C];
	uint64_t dmask[C];
#pragma unroll
	for (int c = 0; c < C; c++) {
		// both shuffles are executed by the whole wave (a shuffle inside a divergent
		// branch cannot read lanes that did not take the branch)
		uint32_t pe = __shfl_up(st[c], 1, 64);
		const uint32_t prev_slot_last = __shfl(st[c > 0 ? c - 1 : 0], 63, 64);
		bool known = true;
		if (lane == 0) {
			if (c > 0)
				pe = prev_slot_last;
			else if (chain[c] == 0)
				pe = init_of(a);
			else
				known = false;   // previous chain belongs to another wave
		}
		bool ok = false;
		if (known && chain[c] < a.n_chains) {
			if (pe == 0) {
				ok = true;
			} else if (pe < a.H) {
				const uint32_t t = hot[(pe << ls) | fb[c]];   // fb: the class of the chain's first byte
				ok = t < a.hot_depth1;   // non-final, depth <= 1 (a sentinel cell is never below)
			}
		}
		decided[c] = ok;
		dmask[c] = __builtin_amdgcn_ballot_w64(ok);
	}
	// chain j is settled when its own probe merged at step <= 1 and so did the
	// probes of the q-1 chains before it (then the true start state is e[j-1])
	const uint32_t window = a.q - 1;
#pragma unroll
	for (int c = 0; c < C; c++) {
		if (chain[c] >= a.n_chains)
			continue;
		bool final_here = decided[c] && window <= 32;
		const int p = c * 64 + (int)lane;   // position inside the tile
		for (uint32_t k = 1; final_here && k <= window; k++) {
			const int pos = p - (int)k;
			if (pos < 0) {
				final_here = (wt == 0);   // before the first chain of the text: nothing to check
				break;
			}
			uint64_t mword = dmask[0];
#pragma unroll
			for (int cc = 1; cc < C; cc++)
				mword = (pos >> 6) == cc ? dmask[cc] : mword;
			final_here = (mword >> (pos & 63)) & 1ull;
		}
		a.probe[chain[c]] = decided[c] ? 1 : kProbeTodo;
		if (decided[c])
			a.wend[chain[c]] = st[c];
		a.rflag[chain[c]] = final_here ? 1 : 0;
		if (final_here) {
			a.k2info[chain[c]] = 0;
			a.cnt[chain[c]] = (int32_t)cnt[c];
		}
	}
}

// Halo mode (HALO): when the longest pattern is short against the chain (L - 1 <= S, a set of
// words), a chain does not start in the root at its first byte and leave the truth to the probe
// and resolve kernels -- it starts hb = L - 1 bytes (rounded up to 16) EARLIER: the DFA state only
// remembers the last L - 1 bytes, so from its own first byte on the walk is the serial one.  Hits
// in front of the chain are not counted; the chain's count is final, the tile's total goes to the
// scatter kernel directly, k_probe and k_resolve are not launched.  A chain less than hb bytes
// into the text starts at byte 0 in the carried-in state.
// PRE (halo mode, chains of up to five 16-byte groups): all text of the lane's chains is loaded up
// front, a chain's five loads back to back.  Taken one group per trip through the loop, a 64-byte
// line of the text is touched by four or five loads many microseconds apart -- lane-per-chain is a
// gather, 16 bytes per lane at a stride of one chain -- and with 8 MB of such lines in flight per
// XCD against 4 MB of L2 they are fetched again and again (135 MB counted for a 32 MiB text).
constexpr int kPreGroups = 5;
template <int C, bool GUARD, bool CLS, bool HALO, bool PRE = false>
__device__ __forceinline__ void walk_tile(const ScanArgs &a, const uint16_t *hot, const uint8_t *clsmap, uint32_t wt,
    uint32_t lane)
{
	const uint32_t ls = CLS ? a.ls : 8u;
	const uint32_t hb = HALO ? a.halo_bytes : 0u;
	uint32_t st[C], cnt[C], first[C], base[C], len[C], chain[C], fb[C], lead[C];
	uint32_t wcount = 0;
	uint2 *stage = a.stage1 + (((size_t)wt * C * 64) << a.logS);
#pragma unroll
	for (int c = 0; c < C; c++) {
		chain[c] = (wt * C + c) * 64 + lane;
		base[c] = chain[c] << a.logS;
		len[c] = GUARD ? (base[c] >= a.n ? 0u : min(a.S, a.n - base[c])) : a.S;
		lead[c] = min(hb, base[c]);
		st[c] = (HALO && base[c] <= hb) ? init_of(a) : 0u;
		cnt[c] = 0;
		first[c] = kNoFirst;
		fb[c] = 0;
	}
	const uint32_t groups = (a.S + hb) >> 4;
	// (five named sets, picked by a branch on the wave-uniform g below: an array of them indexed by g
	// would live in scratch)
	uint4 p0[C], p1[C], p2[C], p3[C], p4[C];
	static_assert(kPreGroups == 5, "five register sets");
	if (PRE) {
		auto fetch = [&](int c, uint32_t gi) -> uint4 {
			const int64_t at = (int64_t)base[c] - hb + (int64_t)gi * 16;
			if (gi < groups && (!GUARD || (at >= 0 && at < (int64_t)a.n)))
				return a.text16[at >> 4];
			return make_uint4(0, 0, 0, 0);
		};
#pragma unroll
		for (int c = 0; c < C; c++) {
			p0[c] = fetch(c, 0);
			p1[c] = fetch(c, 1);
			p2[c] = fetch(c, 2);
			p3[c] = fetch(c, 3);
			p4[c] = fetch(c, 4);
			if (!HALO)   // speculative mode: the class of the chain's first byte, for the tile epilogue
				fb[c] = CLS ? (uint32_t)clsmap[p0[c].x & 0xFFu] : p0[c].x & 0xFFu;
		}
	}
	for (uint32_t g = 0; g < groups; g++) {
		// (prefetching the next group does not help: vector loads return in order, so
		// the first cold gather of this group would wait for the prefetch anyway)
		uint4 w[C];
		if (PRE) {   // (g is wave-uniform: scalar branches, no indexed registers)
			const uint32_t gu = __builtin_amdgcn_readfirstlane(g);
#pragma unroll
			for (int c = 0; c < C; c++) {
				if (gu == 0) w[c] = p0[c];
				else if (gu == 1) w[c] = p1[c];
				else if (gu == 2) w[c] = p2[c];
				else if (gu == 3) w[c] = p3[c];
				else w[c] = p4[c];
			}
		}
#pragma unroll
		for (int c = 0; c < C && !PRE; c++) {
			const int64_t at = (int64_t)base[c] - hb + (int64_t)g * 16;   // first byte of the group
			if (!GUARD || (at >= 0 && at < (int64_t)a.n))
				w[c] = a.text16[at >> 4];
			else
				w[c] = make_uint4(0, 0, 0, 0);
			if (!HALO && g == 0)
				fb[c] = CLS ? (uint32_t)clsmap[w[c].x & 0xFFu] : w[c].x & 0xFFu;
		}
#define ACM_STEP(K) step_all<C, K, GUARD, CLS, HALO>(a, hot, clsmap, ls, w, st, cnt, first, base, len, lead, hb, g, wcount, stage)
		ACM_STEP(0); ACM_STEP(1); ACM_STEP(2); ACM_STEP(3);
		ACM_STEP(4); ACM_STEP(5); ACM_STEP(6); ACM_STEP(7);
		ACM_STEP(8); ACM_STEP(9); ACM_STEP(10); ACM_STEP(11);
		ACM_STEP(12); ACM_STEP(13); ACM_STEP(14); ACM_STEP(15);
#undef ACM_STEP
	}
	if (HALO) {
		static_assert(!HALO || C * 64 == kBlock2, "halo mode: a wave tile is a scatter block");
		uint32_t total = 0;
#pragma unroll
		for (int c = 0; c < C; c++) {
			if (chain[c] < a.n_chains) {
				a.cnt[chain[c]] = (int32_t)cnt[c];
				total += cnt[c];
				if (chain[c] == a.n_chains - 1)
					a.misc[0] = st[c];   // the state after the last byte
			}
		}
#pragma unroll
		for (int o = 32; o > 0; o >>= 1)
			total += __shfl_xor(total, o, 64);
		if (lane == 0) {
			a.wave_cnt1[wt] = wcount;
			a.off[wt] = (int32_t)total;   // the scatter block's total (k_resolve's job otherwise)
		}
		if (lane < kBlock2 / 64)
			a.wave_cnt2[wt * (kBlock2 / 64) + lane] = 0;   // nothing staged by a resolve kernel
		return;
	}
#pragma unroll
	for (int c = 0; c < C; c++) {
		if (chain[c] < a.n_chains) {
			a.end_state[chain[c]] = st[c];
			a.c1f[chain[c]] = cnt[c] | (first[c] << 16);
		}
	}
	if (lane == 0)
		a.wave_cnt1[wt] = wcount;
	tile_epilogue<C>(a, hot, ls, wt, lane, st, cnt, chain, fb);
}

// K1: persistent workgroups (one per CU), the hot rows live in LDS for the
// whole launch, each wave takes wave tiles of C*64 chains round-robin.
template <int C, bool CLS, bool HALO>
__global__ __launch_bounds__(kBlock1) void k_spec_walk(ScanArgs a)
{
	extern __shared__ __attribute__((aligned(16))) uint16_t hot[];
	uint8_t *clsmap = (uint8_t *)hot + acm::kHotBytes;   // behind the rows: the byte classes (CLS only)
	if (CLS && threadIdx.x < 64)
		((uint32_t *)clsmap)[threadIdx.x] = ((const uint32_t *)a.cls)[threadIdx.x];
	{
		// every workgroup copies the same table: start each one at a different
		// offset so the CUs do not all ask the same L2 channel at the same time
		const uint4 *src = (const uint4 *)a.hot;
		uint4 *dst = (uint4 *)hot;
		const uint32_t n16 = ((a.H << a.ls) + 7) >> 3;  // uint4s: a row has 1 << ls cells of 2 bytes (the table is padded to 16)
		const uint32_t rot = n16 ? (blockIdx.x * 1021u) % n16 : 0u;
		for (uint32_t i = threadIdx.x; i < n16; i += kBlock1) {
			uint32_t j = i + rot;
			j = j >= n16 ? j - n16 : j;
			dst[j] = src[j];
		}
	}
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t wave = blockIdx.x * kWaves1 + (threadIdx.x >> 6);
	const uint32_t nwaves = gridDim.x * kWaves1;
	const uint32_t tile_bytes = (C * 64u) << a.logS;
	for (uint32_t wt = wave; wt < a.n_tiles; wt += nwaves) {
		// (the unguarded walk: every chain of the tile whole, and in halo mode with its whole halo)
		const bool full = (uint64_t)(wt + 1) * tile_bytes <= a.n && (!HALO || (uint64_t)wt * tile_bytes >= a.halo_bytes);
		if (full)
			walk_tile<C, false, CLS, HALO>(a, hot, clsmap, wt, lane);
		else
			walk_tile<C, true, CLS, HALO>(a, hot, clsmap, wt, lane);
	}
}

// Halo mode with the text loaded up front (walk_tile, PRE): the registers that takes are there for
// workgroups of 8 waves; with chains of 64 bytes a 32 MiB text has a tile per wave of them anyway.
constexpr int kBlockPre = 768;
// HALO = false: the speculative mode's chains loaded up front the same way (chains of up to 80 bytes; with the
// 64-byte chains long patterns get, a lane's four 16-byte loads per chain at a stride of one chain fetched every
// line of the text several times: 182 MB counted for a 32 MiB text).
// C = 2, BLOCK = 1024 (speculative mode): 16 waves of two chains per lane -- 512 Ki chains a round, which is what a
// 32 MiB text has at 64 bytes a chain: every lane busy, where 12 waves x 4 chains leave a third of them without work.
template <bool CLS, bool HALO = true, int C = 4, int BLOCK = kBlockPre>
__global__ __launch_bounds__(BLOCK) void k_halo_walk(ScanArgs a)
{
	extern __shared__ __attribute__((aligned(16))) uint16_t hot[];
	uint8_t *clsmap = (uint8_t *)hot + acm::kHotBytes;
	if (CLS && threadIdx.x < 64)
		((uint32_t *)clsmap)[threadIdx.x] = ((const uint32_t *)a.cls)[threadIdx.x];
	{
		const uint4 *src = (const uint4 *)a.hot;
		uint4 *dst = (uint4 *)hot;
		const uint32_t n16 = ((a.H << a.ls) + 7) >> 3;
		const uint32_t rot = n16 ? (blockIdx.x * 1021u) % n16 : 0u;
		for (uint32_t i = threadIdx.x; i < n16; i += BLOCK) {
			uint32_t j = i + rot;
			j = j >= n16 ? j - n16 : j;
			dst[j] = src[j];
		}
	}
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t wave = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
	const uint32_t nwaves = gridDim.x * (BLOCK / 64);
	const uint32_t tile_bytes = ((uint32_t)C * 64u) << a.logS;
	for (uint32_t wt = wave; wt < a.n_tiles; wt += nwaves) {
		const bool full = (uint64_t)(wt + 1) * tile_bytes <= a.n && (uint64_t)wt * tile_bytes >= a.halo_bytes;
		if (full)
			walk_tile<C, false, CLS, HALO, true>(a, hot, clsmap, wt, lane);
		else
			walk_tile<C, true, CLS, HALO, true>(a, hot, clsmap, wt, lane);
	}
}

// ---------------------------------------------------------------------------
// K2: deep walks
// ---------------------------------------------------------------------------

// K2a probe: lane c walks chain c from e[c-1] (the state chain c would start
// in if chain c-1 has merged -- the overwhelmingly common case) until the
// depth test says it has merged with chain c's own root walk.  It records
// whether it merged, the state at the end of the chain under that
// assumption (wend), and whether anything in the unmerged head needs an
// emission walk (a true hit there, or a K1 hit that must be dropped).
// Chains the walk kernel's epilogue already probed are skipped.
template <bool NOCASE = false>
__global__ __launch_bounds__(kBlock2) void k_probe(ScanArgs a)
{
	const uint32_t c = blockIdx.x * kBlock2 + threadIdx.x;
	if (c >= a.n_chains)
		return;
	if (a.probe[c] != kProbeTodo)
		return;
	Deep d;
	d.s = c == 0 ? init_of(a) : a.end_state[c - 1];
	d.depth = 0;
	d.run = 0;
	const uint32_t base = c << a.logS;
	const uint32_t len = min(a.S, a.n - base);
	const uint32_t f = a.c1f[c] >> 16;
	bool merged = (d.s == 0), work = false;
	if (!merged) {
		ChainText txt(a, base);
		for (uint32_t m = 1; m <= len; m++) {
			d = deep_step(a, d.s, txt.at(m));
			if (d.depth <= m) {
				merged = true;
				break;
			}
			work |= (d.s >= a.F) | (m >= f);
			if (d.run != 0 && d.s < a.F) {
				m += fast_forward<NOCASE>(a, d, base + m, len - m);
				work |= (m >= f);
			}
		}
	}
	a.wend[c] = merged ? a.end_state[c] : d.s;
	a.probe[c] = (uint8_t)((merged ? 1u : 0u) | (work ? 2u : 0u));
}

// K2b resolve: one lane per chain (see the file header).
template <bool NOCASE = false>
__global__ __launch_bounds__(kBlock2) void k_resolve(ScanArgs a)
{
	__shared__ uint32_t wave_fill[kBlock2 / 64];
	__shared__ uint32_t wave_sum[kBlock2 / 64];
	const uint32_t j = blockIdx.x * kBlock2 + threadIdx.x;
	const uint32_t wv = threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 0)
		wave_fill[wv] = 0;
	__syncthreads();
	const uint32_t gw = j >> 6;
	uint2 *stage = a.stage2 + (((size_t)gw * 64) << a.logS);
	uint32_t my_cnt = 0;

	if (j < a.n_chains && a.rflag[j]) {
		my_cnt = (uint32_t)a.cnt[j];   // resolved by the walk kernel's epilogue
		if (j == a.n_chains - 1)
			a.misc[0] = a.wend[j];
	} else if (j < a.n_chains) {
		const uint32_t info = a.c1f[j];
		const uint32_t c1 = info & 0xFFFFu, f = info >> 16;
		const uint32_t first = j < a.q ? 0u : j - a.q + 1;   // first chain the look-back walks
		// ---- fast path -----------------------------------------------------
		bool window_ok = true;
		for (uint32_t c = first; c + 1 < j; c++)            // chains first .. j-2 must have merged
			window_ok &= (a.probe[c] & 1u) != 0;
		const uint32_t pj = a.probe[j];
		const uint32_t assumed = j == 0 ? init_of(a) : a.end_state[j - 1];
		// q == 1 (S >= L): the window is empty and e[j-1] is already the true state
		uint32_t state = (j == 0 || first == j) ? assumed : a.wend[j - 1];
		if (window_ok && state == assumed && !(pj & 2u)) {
			a.k2info[j] = 0;
			my_cnt = c1;
			if (j == a.n_chains - 1)
				a.misc[0] = a.wend[j];
		} else {
			uint32_t m = 0;
			if (!window_ok) {
				// ---- general look-back: true state at the start of chain j ----
				uint32_t c = first;
				state = j < a.q ? init_of(a) : a.end_state[j - a.q];
				ChainText txt(a, first << a.logS);
				while (c < j) {
					if (m == 0 && state == 0) {  // root: merged with chain c's own walk
						state = a.end_state[c];
						c++;
						continue;
					}
					if (m == 0 && state == (c == 0 ? init_of(a) : a.end_state[c - 1])) {
						state = a.wend[c];       // exactly the walk the probe of chain c did
						c++;
						continue;
					}
					m++;
					// chains are adjacent: step m of chain c is byte (c - first) * S + m - 1
					Deep d = deep_step(a, state, txt.at(((c - first) << a.logS) + m));
					if (d.depth <= m) {
						state = a.end_state[c];
						c++;
						m = 0;
						continue;
					}
					if (d.run != 0 && d.s < a.F)
						m += fast_forward<NOCASE>(a, d, (c << a.logS) + m, a.S - m);
					state = d.s;
					if (m == a.S) {
						c++;
						m = 0;
					}
				}
			}
			// ---- head of the own chain, from the true state --------------------
			const uint32_t base = j << a.logS;
			const uint32_t len = min(a.S, a.n - base);
			uint32_t c2 = 0;
			bool killed = false, merged = (state == 0);
			if (!merged) {
				ChainText txt(a, base);
				for (m = 1; m <= len; m++) {
					Deep d = deep_step(a, state, txt.at(m));
					state = d.s;
					if (!killed && d.depth <= m) {
						merged = true;
						break;
					}
					if (state >= a.F && base + m - 1 >= a.drop_before) {
						const uint32_t slot = atomicAdd(&wave_fill[wv], 1u);
						stage[slot] = make_uint2(base + m - 1, state | (c2 << 24));
						c2++;
					}
					if (!killed && m >= f)
						killed = true;  // a K1 hit sits in the unmerged head: take the chain over
					if (d.run != 0 && state < a.F) {
						m += fast_forward<NOCASE>(a, d, base + m, len - m);
						state = d.s;
						if (!killed && m >= f)
							killed = true;
					}
				}
			}
			a.k2info[j] = c2 | (killed ? 0x10000u : 0u);
			my_cnt = c2 + (killed ? 0u : c1);
			if (j == a.n_chains - 1)
				a.misc[0] = merged ? a.end_state[j] : state;
		}
		a.cnt[j] = (int32_t)my_cnt;
	}
	// per-block total of the chain counts, scanned by k_scan_top
	uint32_t wsum = my_cnt;
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
		wsum += __shfl_down(wsum, o, 64);
	if ((threadIdx.x & 63) == 0)
		wave_sum[wv] = wsum;
	__syncthreads();
	if ((threadIdx.x & 63) == 0 && gw * 64 < a.n_chains)
		a.wave_cnt2[gw] = wave_fill[wv];
	if (threadIdx.x == 0) {
		uint32_t t = 0;
		for (int w = 0; w < kBlock2 / 64; w++)
			t += wave_sum[w];
		a.off[blockIdx.x] = (int32_t)t;
	}
}

// ---------------------------------------------------------------------------
// scan of the block totals + ordered scatter
// ---------------------------------------------------------------------------

// exclusive scan, in place, of the per-block totals by ONE workgroup: each
// thread owns a contiguous slice, the 1024 slice sums go through a Blelloch
// up-sweep / down-sweep in LDS.  Also publishes the grand total.
constexpr int kTopThreads = 1024;
constexpr uint32_t kTopMax = kTopThreads * 64;
constexpr uint32_t kFoldMax = 8192;   // block totals a scatter block still adds up by itself (64 MiB at S = 32)

__global__ __launch_bounds__(kTopThreads) void k_scan_top(ScanArgs a, uint32_t nb)
{
	__shared__ int32_t tree[kTopThreads + (kTopThreads >> 5) + 1];
	const int tid = threadIdx.x;
	const uint32_t per = (nb + kTopThreads - 1) / kTopThreads;
	const uint32_t lo = min(nb, (uint32_t)tid * per), hi = min(nb, lo + per);
	int32_t sum = 0;
	for (uint32_t i = lo; i < hi; i++)
		sum += a.off[i];
	auto pad = [](int i) { return i + (i >> 5); };
	tree[pad(tid)] = sum;
	int offset = 1;
	for (int d = kTopThreads >> 1; d > 0; d >>= 1) {
		__syncthreads();
		if (tid < d)
			tree[pad(offset * (2 * tid + 2) - 1)] += tree[pad(offset * (2 * tid + 1) - 1)];
		offset <<= 1;
	}
	__syncthreads();
	if (tid == 0) {
		a.misc[1] = (uint32_t)tree[pad(kTopThreads - 1)];
		tree[pad(kTopThreads - 1)] = 0;
	}
	for (int d = 1; d < kTopThreads; d <<= 1) {
		offset >>= 1;
		__syncthreads();
		if (tid < d) {
			const int ai = pad(offset * (2 * tid + 1) - 1), bi = pad(offset * (2 * tid + 2) - 1);
			const int32_t t = tree[ai];
			tree[ai] = tree[bi];
			tree[bi] += t;
		}
	}
	__syncthreads();
	int32_t run = tree[pad(tid)];
	for (uint32_t i = lo; i < hi; i++) {
		const int32_t v = a.off[i];
		a.off[i] = run;
		run += v;
	}
}

// Ordered scatter of both staging areas + header/trailer cells, one workgroup
// per 256 chains (the K2b block): scan the block's 256 counts in LDS on top
// of the block base, then every wave drains one K2 staging region and, while
// there are any, one K1 wave tile of this block.
template <int C>
__global__ __launch_bounds__(kBlock2) void k_scatter_all(ScanArgs a)
{
	__shared__ uint32_t off[kBlock2];
	__shared__ uint32_t wtot[kBlock2 / 64];
	const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const uint32_t j0 = blockIdx.x * kBlock2, j = j0 + tid;
	const uint32_t c = j < a.n_chains ? (uint32_t)a.cnt[j] : 0u;
	// in-wave inclusive scan by shuffles, then add the preceding waves
	uint32_t inc = c;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const uint32_t t = __shfl_up(inc, o, 64);
		if (lane >= (uint32_t)o)
			inc += t;
	}
	if (lane == 63)
		wtot[wv] = inc;
	__syncthreads();
	uint32_t before, total_records = 0;
	if (a.fold_blocks) {
		// no separate scan launch over the block totals: every block adds up the ones in front of
		// it (a few thousand L2-resident words), block 0 also all of them for the header cell
		__shared__ uint32_t part[kBlock2 / 64], part_all[kBlock2 / 64];
		uint32_t mine = 0, all = 0;
		const uint32_t upto = blockIdx.x == 0 ? a.fold_blocks : blockIdx.x;
		for (uint32_t i = tid; i < upto; i += kBlock2) {
			const uint32_t v = (uint32_t)a.off[i];
			all += v;
			mine += i < blockIdx.x ? v : 0u;
		}
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) {
			mine += __shfl_xor(mine, o, 64);
			all += __shfl_xor(all, o, 64);
		}
		if (lane == 0) {
			part[wv] = mine;
			part_all[wv] = all;
		}
		__syncthreads();
		before = 0;
		for (uint32_t w = 0; w < kBlock2 / 64; w++) {
			before += part[w];
			total_records += part_all[w];
		}
	} else {
		before = (uint32_t)a.off[blockIdx.x];
		if (blockIdx.x == 0 && tid == 0)
			total_records = a.misc[1];
	}
	for (uint32_t w = 0; w < wv; w++)
		before += wtot[w];
	off[tid] = before + inc - c;
	__syncthreads();

	auto drain = [&](const uint2 *stage, uint32_t nrec, bool from_k1) {
		for (uint32_t i = lane; i < nrec; i += 64) {
			const uint2 rec = stage[i];
			const uint32_t pos = rec.x, st = rec.y & 0xFFFFFFu, seq = rec.y >> 24;
			const uint32_t jj = pos >> a.logS;
			uint32_t d = off[jj - j0] + seq;
			if (from_k1 && !a.halo_mode) {   // (halo mode: nothing is ever dropped or staged by a resolve kernel)
				const uint32_t info = a.k2info[jj];
				if (info & 0x10000u)
					continue;
				d += info & 0xFFFFu;
			}
			if (d + 2 < a.plane_capacity) {
				a.pat_plane[1 + d] = a.out[st];
				a.off_plane[1 + d] = (int32_t)pos + a.off_shift;
			}
		}
	};
	const uint32_t gw = blockIdx.x * (kBlock2 / 64) + wv;            // K2 staging region
	if (gw * 64 < a.n_chains)
		drain(a.stage2 + (((size_t)gw * 64) << a.logS), a.wave_cnt2[gw], false);
	constexpr uint32_t kTilesPerBlock = kBlock2 / (C * 64);          // K1 wave tiles in this block
	if (wv < kTilesPerBlock) {
		const uint32_t wt = blockIdx.x * kTilesPerBlock + wv;
		if (wt < a.n_tiles)
			drain(a.stage1 + (((size_t)wt * C * 64) << a.logS), a.wave_cnt1[wt], true);
	}
	if (blockIdx.x == 0 && tid == 0) {   // header and trailer cells (compactarray.cl:49-55)
		const uint32_t total = total_records;
		const int32_t last_ref = (int32_t)a.dev2ref[a.misc[0]];
		a.misc[2] = (uint32_t)ACM_SCAN_MODE_CHAIN;   // acm_scan_path_taken
		uint32_t tail = total + 1;
		if (tail > a.plane_capacity - 1)
			tail = a.plane_capacity - 1;
		a.pat_plane[0] = (int32_t)total;
		a.off_plane[0] = (int32_t)total;
		a.pat_plane[tail] = last_ref;
		a.off_plane[tail] = last_ref;
	}
}

// A scan that continues another on the device (acm_scan_batch.d_init_plane): the final state of that scan is in the
// trailer cell of its pattern plane, behind the header cell that says where (compactarray.cl:49-55 layout;
// the reference hands it from round to round through the host, databuf.c:622).  One thread translates it
// into this device's numberings and leaves it in the workspace, where the kernels of the scan look for it.
__global__ void k_carry_init(const int32_t *plane, uint32_t capacity, const uint32_t *ref2dev, const uint32_t *ref2code,
    uint32_t states, uint32_t *dev_out, uint32_t *code_out)
{
	if (threadIdx.x != 0 || blockIdx.x != 0)
		return;
	const int32_t m = plane[0];
	uint32_t tail = (uint32_t)(m < 0 ? 0 : m) + 1;
	if (tail > capacity - 1)
		tail = capacity - 1;
	uint32_t ref = (uint32_t)plane[tail];
	if (ref >= states)
		ref = 0;   // (not a state: cannot happen with planes of this library)
	*dev_out = ref2dev[ref];
	*code_out = ref2code ? ref2code[ref] : 0u;
}

// empty text: header and trailer only
__global__ void k_finalize_empty(ScanArgs a)
{
	if (threadIdx.x != 0 || blockIdx.x != 0)
		return;
	const int32_t last_ref = (int32_t)a.dev2ref[init_of(a)];
	a.misc[2] = (uint32_t)ACM_SCAN_MODE_CHAIN;
	a.pat_plane[0] = 0;
	a.off_plane[0] = 0;
	a.pat_plane[1] = last_ref;
	a.off_plane[1] = last_ref;
}

// ---------------------------------------------------------------------------
// host side: the workspace layout and what the dispatcher enqueues (chain.h)
// ---------------------------------------------------------------------------

// geometry: enough chains to give every lane of every CU work, chains as long as that allows (longer chains = fewer look-back steps)
struct Geometry {
	int C;                // chains per lane
	uint32_t S;           // chain bytes
	bool wide_pre;        // speculative mode with 64-byte chains: two chains per lane, 16 waves per CU, text loaded up front
	uint32_t halo_mode, halo_bytes, halo_pre;   // halo mode (walk_tile): the longest pattern fits the chain -- no speculation to resolve
};

Geometry chain_geometry(const acm_dfa *d, size_t n)
{
	Geometry g = { d->chains_per_lane == 2 ? 2 : 4, (uint32_t)d->chain_bytes, false, 0, 0, 0 };
	const uint32_t hb = ((d->max_pattern_len > 1 ? d->max_pattern_len - 1 : 0u) + 15u) & ~15u;
	auto halo_fits = [&] { return d->use_halo && hb <= g.S; };   // a chain can walk the longest pattern's halo in front of its own bytes
	if (g.S == 0) {
		const size_t lanes = (size_t)d->num_cus * kBlock1 * g.C;
		g.S = 16;
		while (g.S < 256 && (size_t)g.S * 2 * lanes <= n)
			g.S *= 2;
		// halo mode walks L - 1 bytes per chain twice: with half the waves of every CU still busy a
		// chain of four halos is the better deal when batches are in flight side by side (sentiment
		// set, 32 MiB: 650 instead of 574 GB/s; alone the walk takes 89 instead of 56 us)
		uint32_t want = 16;
		while (want < 4 * hb)
			want *= 2;
		if (halo_fits() && g.C == 4 && hb > 0 && want > g.S && want <= 256 && (size_t)want * lanes <= 2 * n)
			g.S = want;
		// speculative mode (patterns longer than a chain): a chain's look-back window is ceil(L / S) chains, and
		// it is the probe and resolve kernels' slowest lanes -- chains of dependent loads through that window --
		// that those kernels take as long as.  Chains of a third of the longest pattern: half the chains of the
		// same text at 32 MiB, i.e. half of every CU's lanes idle in the walk kernel -- which batches in flight
		// side by side fill (ClamAV signatures, 3 streams: 635 instead of 489 GB/s; a batch alone 111 instead of
		// 98 us).  Large texts only: a small one is short of chains as it is.
		if (!halo_fits() && n >= ((size_t)16 << 20)) {
			while (g.S < 256 && (d->max_pattern_len + g.S - 1) / g.S > 3)
				g.S *= 2;
			static const bool no_wide = getenv("ACM_SCAN_NO_WIDE_PRE") != nullptr;   // debugging aid
			if (g.S == 64 && g.C == 4 && d->use_preload && !no_wide) {
				g.wide_pre = true;
				g.C = 2;
			}
		}
	}
	g.halo_mode = (halo_fits() && g.C == 4) ? 1u : 0u;
	g.halo_bytes = g.halo_mode ? hb : 0u;
	g.halo_pre = (g.halo_mode && ((g.S + hb) >> 4) <= (uint32_t)kPreGroups && d->use_preload) ? 1u : 0u;
	if (!g.halo_mode && g.S == 64 && d->use_preload && (g.C == 4 || g.wide_pre))
		g.halo_pre = 1u;   // (speculative mode, chains of 64 bytes: k_halo_walk<CLS, false, ...>)
	return g;
}

ScanArgs scan_args(const acm_dfa *d, const acm_scan_batch *b, const acm::ScanLayout &l, const Geometry &g, uint32_t init_dev,
    const uint32_t *init_ptr)
{
	char *ws = (char *)b->d_workspace;
	ScanArgs a;
	memset(&a, 0, sizeof(a));
	a.cold = d->d_cold;
	a.deep = d->d_deep;
	a.hot = d->d_hot;
	a.cls = d->d_class;
	a.ls = d->log_stride;
	a.halo_bytes = g.halo_bytes;
	a.halo_mode = g.halo_mode;
	a.halo_pre = g.halo_pre;
	// the plane value of a record is a per-state table lookup: the head pattern, or the state's
	// reference id when the caller wants to expand the whole match list afterwards
	a.out = b->report == ACM_REPORT_STATE ? (const int32_t *)d->d_dev2ref : d->d_out;
	a.dev2ref = d->d_dev2ref;
	a.in_byte = d->d_in_byte;
	a.text16 = (const uint4 *)b->d_text;
	a.text = (const uint8_t *)b->d_text;
	a.n = (uint32_t)b->n;
	a.n_pad = (uint32_t)((b->n + 15) & ~(size_t)15);
	a.S = g.S;
	while ((1u << a.logS) < g.S)
		a.logS++;
	a.n_chains = (uint32_t)((b->n + g.S - 1) >> a.logS);
	a.n_tiles = (a.n_chains + g.C * 64 - 1) / (g.C * 64);
	a.H = d->hot_rows;
	a.hot_depth1 = d->hot_depth1;
	a.F = d->first_final;
	a.L = d->max_pattern_len;
	a.q = std::max(1u, (a.L + g.S - 1) / g.S);
	a.init_state = init_dev;
	a.init_ptr = init_ptr;
	a.drop_before = (uint32_t)b->halo;
	a.off_shift = (int32_t)b->offset_shift;
	a.end_state = (uint32_t *)(ws + l.end_state);
	a.c1f = (uint32_t *)(ws + l.c1f);
	a.k2info = (uint32_t *)(ws + l.k2info);
	a.wend = (uint32_t *)(ws + l.wend);
	a.probe = (uint8_t *)(ws + l.probe);
	a.rflag = (uint8_t *)(ws + l.rflag);
	a.cnt = (int32_t *)(ws + l.cnt);
	a.off = (int32_t *)(ws + l.off);
	a.wave_cnt1 = (uint32_t *)(ws + l.wave_cnt1);
	a.wave_cnt2 = (uint32_t *)(ws + l.wave_cnt2);
	a.misc = (uint32_t *)(ws + l.misc);
	a.stage1 = (uint2 *)(ws + l.stage1);
	a.stage2 = (uint2 *)(ws + l.stage2);
	a.pat_plane = b->d_pat_plane;
	a.off_plane = b->d_off_plane;
	a.plane_capacity = (uint32_t)std::min<size_t>(b->plane_capacity, 0xFFFFFFFFul);
	return a;
}

template <int C>
int launch_spec_walk(const ScanArgs &a, int num_cus, hipStream_t s)
{
	const size_t lds = acm::kHotBytes + 256;   // rows + class map; above 48 KiB: allowed by acm::scan_prepare
	const bool cls = a.ls != 8;
	void (*walk)(ScanArgs);
	uint32_t block = kBlock1;
	if (C == 2 && a.halo_pre && !a.halo_mode) {   // (speculative mode, 64-byte chains: 16 waves of two chains per lane)
		walk = cls ? k_halo_walk<true, false, 2, 1024> : k_halo_walk<false, false, 2, 1024>;
		block = 1024;
	} else if (C == 4 && a.halo_pre) {
		walk = a.halo_mode ? (cls ? k_halo_walk<true, true> : k_halo_walk<false, true>)
		                   : (cls ? k_halo_walk<true, false> : k_halo_walk<false, false>);
		block = kBlockPre;
	} else if (a.halo_mode && C == 4) {
		walk = cls ? k_spec_walk<4, true, true> : k_spec_walk<4, false, true>;
	} else {
		walk = cls ? k_spec_walk<C, true, false> : k_spec_walk<C, false, false>;
	}
	const uint32_t blocks = std::min((a.n_tiles + block / 64 - 1) / (block / 64), (uint32_t)num_cus);   // a wave per tile, a workgroup per CU
	hipLaunchKernelGGL(walk, dim3(blocks), dim3(block), lds, s, a);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}

}  // namespace

namespace acm {

// sized for the smallest chain length (16 B) so any geometry fits
ScanLayout scan_layout(const acm_dfa *d, size_t max_text)
{
	ScanLayout l;
	const size_t chains = max_text / 16 + 64 * 4 + 64;
	const size_t waves = chains / 64 + 2;
	const size_t stage_recs = max_text + (size_t)4 * 64 * 256;
	size_t o = 0;
	auto take = [&](size_t bytes) {
		size_t at = o;
		o = (o + bytes + 255) / 256 * 256;
		return at;
	};
	l.end_state = take(chains * 4);
	l.c1f = take(chains * 4);
	l.k2info = take(chains * 4);
	l.wend = take(chains * 4);
	l.probe = take(chains);
	l.rflag = take(chains);
	l.cnt = take(chains * 4);
	l.off = take(chains * 4);
	l.wave_cnt1 = take(waves * 4);
	l.wave_cnt2 = take(waves * 4);
	l.misc = take(64);
	l.stage1 = take(stage_recs * 8);
	l.stage2 = take(stage_recs * 8);
	l.scan_ws_bytes = acm_exclusive_scan_workspace_bytes(chains / kBlock2 + 2);
	l.scan_ws = take(l.scan_ws_bytes);
	l.sparse = take(d ? acm::sparse_workspace_bytes(d, max_text) : 0);
	l.total = o;
	return l;
}

int scan_prepare(const acm_dfa *)
{
	const void *walks[] = { (const void *)k_spec_walk<4, false, false>, (const void *)k_spec_walk<4, true, false>,
		(const void *)k_spec_walk<2, false, false>, (const void *)k_spec_walk<2, true, false>,
		(const void *)k_spec_walk<4, false, true>, (const void *)k_spec_walk<4, true, true>,
		(const void *)k_halo_walk<false, true>, (const void *)k_halo_walk<true, true>,
		(const void *)k_halo_walk<false, false>, (const void *)k_halo_walk<true, false>,
		(const void *)k_halo_walk<false, false, 2, 1024>, (const void *)k_halo_walk<true, false, 2, 1024> };
	for (const void *k : walks)
		ACM_HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(acm::kHotBytes + 256)));
	return ACM_OK;
}

int carry_init_enqueue(const acm_dfa *d, const acm_scan_batch *b, uint32_t *misc, hipStream_t s)
{
	hipLaunchKernelGGL(k_carry_init, dim3(1), dim3(64), 0, s, (const int32_t *)b->d_init_plane,
	    (uint32_t)std::min<size_t>(b->init_plane_capacity, 0xFFFFFFFFul), (const uint32_t *)d->d_ref2dev,
	    (const uint32_t *)(d->lds_ok ? d->d_lds_ref2code : nullptr), d->num_states, misc + kMiscInitDev, misc + kMiscInitCode);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}

int empty_scan_enqueue(const acm_dfa *d, const acm_scan_batch *b, const ScanLayout &l, uint32_t init_dev, const uint32_t *init_ptr,
    hipStream_t s)
{
	hipLaunchKernelGGL(k_finalize_empty, dim3(1), dim3(64), 0, s, scan_args(d, b, l, chain_geometry(d, 0), init_dev, init_ptr));
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}

int chain_scan_enqueue(const acm_dfa *d, const acm_scan_batch *b, const ScanLayout &l, uint32_t init_dev, const uint32_t *init_ptr,
    hipStream_t s, hipEvent_t after_walk, hipEvent_t after_walk2)
{
	const Geometry g = chain_geometry(d, b->n);
	ScanArgs a = scan_args(d, b, l, g, init_dev, init_ptr);
	int rc = g.C == 4 ? launch_spec_walk<4>(a, d->num_cus, s) : launch_spec_walk<2>(a, d->num_cus, s);
	if (rc != ACM_OK)
		return rc;
	for (hipEvent_t e : { (hipEvent_t)b->record_after_walk, after_walk, after_walk2 })
		if (e)
			ACM_HIP_TRY(hipEventRecord(e, s));
	const uint32_t nb = (a.n_chains + kBlock2 - 1) / kBlock2;   // K2 blocks == scatter blocks
	if (!a.halo_mode) {
		if (d->nocase) {
			hipLaunchKernelGGL(k_probe<true>, dim3(nb), dim3(kBlock2), 0, s, a);
			hipLaunchKernelGGL(k_resolve<true>, dim3(nb), dim3(kBlock2), 0, s, a);
		} else {
			hipLaunchKernelGGL(k_probe<false>, dim3(nb), dim3(kBlock2), 0, s, a);
			hipLaunchKernelGGL(k_resolve<false>, dim3(nb), dim3(kBlock2), 0, s, a);
		}
		ACM_HIP_TRY(hipGetLastError());
	}
	if (nb <= kFoldMax) {
		a.fold_blocks = nb;   // the scatter kernel sums the block totals itself: one launch less
	} else if (nb <= kTopMax) {
		hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(kTopThreads), 0, s, a, nb);
	} else {  // > 16M chains: generic multi-level scan of the block totals
		rc = acm_exclusive_scan_i32(a.off, a.off, nb, (int32_t *)(a.misc + 1), (char *)b->d_workspace + l.scan_ws,
		    l.scan_ws_bytes, s);
		if (rc != ACM_OK)
			return rc;
	}
	static_assert(kBlock2 % (4 * 64) == 0, "a scatter block must hold whole K1 wave tiles");
	hipLaunchKernelGGL(g.C == 4 ? k_scatter_all<4> : k_scatter_all<2>, dim3(nb), dim3(kBlock2), 0, s, a);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}

}  // namespace acm

extern "C" size_t acm_scan_workspace_bytes(const acm_dfa *d, size_t max_text)
{
	return acm::scan_layout(d, max_text).total;
}

extern "C" int acm_scan_set_chain_bytes(acm_dfa *d, int chain_bytes)
{
	if (!d)
		return 0;
	if (chain_bytes == 0 || (chain_bytes >= 16 && chain_bytes <= 256 && (chain_bytes & (chain_bytes - 1)) == 0))
		d->chain_bytes = chain_bytes;
	return d->chain_bytes;
}

extern "C" int acm_scan_set_chains_per_lane(acm_dfa *d, int chains)
{
	if (!d)
		return 0;
	if (chains == 2 || chains == 4)
		d->chains_per_lane = chains;
	return d->chains_per_lane;
}

extern "C" int acm_scan_kernel_count(void) { return 4; }
