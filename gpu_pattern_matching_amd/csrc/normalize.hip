// Normalised scanning: the text with percent triples decoded and blanks squeezed or stripped, the map from
// the normalised text back to the bytes the caller has, and the pass that carries records through that map.
// gfx950 only.  No automaton is involved in the normalise call.  DESIGN.md 6u.
//
// The contract is acmatch.h's (acm_normalize_async).  In short: a text is cut into UNITS (a triple %XX of length
// 3 whose value is the decoded byte, else a byte); a unit whose value is in the blank set is BLANK; squeeze emits
// the first blank unit of a run as blank_byte, strip emits none; every other unit emits its value.  Whether byte i
// starts a unit and whether that unit emits depends on bytes i - 3 .. i + 2 and the text starts among them only.
//
// Launches, on the fixed grid of lines.hip (four blocks a CU, a block owning a contiguous run of 16 KiB tiles of
// the INPUT by share_of):
//   k_norm_starts (segments > 0, behind a memset) a bit per text start, in the workspace
//   k_norm_mask   a lane per 64 bytes: four 16-byte loads in flight, the '%' and hex-digit tests as carry-free
//                 SWAR per dword (exact per byte), the blank test as a lookup in a 256-byte LDS table; the
//                 context (4 bytes in front, 2 behind) comes straight from global memory, which the lane beside
//                 has just loaded.  64-bit masks then give the keep word in a handful of shifts.  Per block the
//                 emitted bytes, the dropped units, the triples and the blank units emitted.
//   k_norm_write  blocks_before over the emitted counts, then per tile: a thread per keep word ranks the tile
//                 (block_prefix), writes the d_block cells, and leaves the words and their ranks in LDS; a
//                 thread per DWORD of the tile (sixteen rows) then puts the dword's kept bytes into the LDS tile
//                 at their rank: lanes beside each other write at most 4 bytes apart.  Only a kept '%' looks
//                 further (is it a head?), only squeeze looks a value up.  The tile is laid out at the output's
//                 own 16-byte phase and streamed out in aligned 16-byte stores; the pieces at the two ends of a
//                 tile's output range, which it shares with the tiles beside it, are written bytewise by the
//                 owner of each byte.  Block 0 writes d_info and the last d_block cell.
//   k_norm_seg    (segments > 0) a thread per start: d_block and the keep words in front of it
// LDS of k_norm_write: the tile (16 KiB + 16 for the phase), 3 KiB of words and ranks, the table: under 20 KiB.
// Occupancy: the grid is four workgroups a CU, and the registers allow no more: k_norm_mask takes 122 VGPRs and
// k_norm_write 120, four waves a SIMD, which is four 256-thread workgroups a CU.  LDS (160 KiB) would hold eight.
//
// acm_normalize_remap_async: a thread per record; a search on d_block, at most 16 popcounts, the k-th set bit of
// one word, and for `last` the bytes at `first`.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "acm_internal.h"
#include "device_dfa.h"
#include "place64.h"
#include "record_pass.h"

namespace {

using namespace acm_rp;

constexpr uint32_t kTileWords = kThreads;          // keep words per tile: 16 KiB of text
constexpr uint32_t kWordsPerCell = ACM_NORM_BLOCK / 64;
constexpr int kRows = kTileBytes / 4 / kThreads;   // dwords a thread places per tile: 16
constexpr unsigned kKnownFlags = ACM_NORM_PERCENT | ACM_NORM_SQUEEZE | ACM_NORM_STRIP;
static_assert(kTileWords * 64 == kTileBytes, "a tile is kThreads keep words");

struct BlankSet {
	uint32_t w[8];
};

struct NormArgs {
	const uint8_t *text;
	uint32_t n, words;             // bytes; 64-bit keep words
	int64_t origin;
	uint32_t percent, squeeze, blanks, blank_byte;
	BlankSet set;                  // all 0 without blanks
	const int32_t *seg_start;
	uint32_t segments;
	const uint32_t *start_bits;    // bit 32 + i: a text starts at byte i >= 1; null without segments
	// workspace
	int32_t *blk;                  // [4][kMaxBlocks] per block: emitted, dropped, triples, blanks emitted
	// output
	uint64_t *keep;
	int32_t *block;
	uint8_t *out;
	uint32_t cap;
	int32_t *seg_out;
	int32_t *info;
};

// 4 bits: byte j of w equals the byte every byte of pat repeats.  No carry crosses a byte: exact.  (lines.hip)
__device__ __forceinline__ uint32_t eq4(uint32_t w, uint32_t pat)
{
	const uint32_t x = w ^ pat;
	const uint32_t t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
	return (((t >> 7) * 0x00204081u) >> 21) & 0xFu;
}

// 4 bits: byte j of w is in [0-9A-Fa-f].  x: the low seven bits; x + (0x80 - lo) sets a byte's top bit iff x >= lo,
// and no sum leaves its byte.
__device__ __forceinline__ uint32_t hex4(uint32_t w)
{
	const uint32_t x = w & 0x7F7F7F7Fu, y = x | 0x20202020u;
	const uint32_t digit = (x + 0x50505050u) & ~(x + 0x46464646u);    // 0x30 <= x < 0x3A
	const uint32_t letter = (y + 0x1F1F1F1Fu) & ~(y + 0x19191919u);   // 0x61 <= y < 0x67
	const uint32_t t = (digit | letter) & ~w & 0x80808080u;
	return (((t >> 7) * 0x00204081u) >> 21) & 0xFu;
}

__device__ __forceinline__ bool is_hex(uint32_t b)
{
	return (b - '0') < 10u || ((b | 0x20) - 'a') < 6u;
}

__device__ __forceinline__ uint32_t hex_val(uint32_t b) { return b <= '9' ? b - '0' : (b | 0x20) - 'a' + 10; }

__device__ __forceinline__ uint32_t decode(uint32_t hi, uint32_t lo) { return hex_val(hi) << 4 | hex_val(lo); }

// a text starts at byte i (0 < i)
__device__ __forceinline__ bool start_at(const uint32_t *start_bits, uint32_t i)
{
	return start_bits && (start_bits[(i >> 5) + 1] >> (i & 31) & 1);
}

// byte p < n is '%': is it a triple head?
__device__ __forceinline__ bool is_head(const uint8_t *text, uint32_t n, const uint32_t *start_bits, uint32_t p)
{
	return p + 2 < n && is_hex(text[p + 1]) && is_hex(text[p + 2]) && !start_at(start_bits, p + 1) && !start_at(start_bits, p + 2);
}

__device__ __forceinline__ void fill_table(const BlankSet &set, uint8_t *btab)
{
	uint32_t w = 0;
#pragma unroll
	for (uint32_t k = 0; k < 8; k++)
		w = threadIdx.x >> 5 == k ? set.w[k] : w;
	btab[threadIdx.x] = (uint8_t)(w >> (threadIdx.x & 31) & 1);
}

__device__ __forceinline__ uint32_t blank4(const uint8_t *btab, uint32_t w)
{
	return (uint32_t)btab[w & 0xFF] | (uint32_t)btab[w >> 8 & 0xFF] << 1 | (uint32_t)btab[w >> 16 & 0xFF] << 2 |
	    (uint32_t)btab[w >> 24] << 3;
}

struct Words {
	uint32_t w_begin, w_end;   // the block's keep words
};

__device__ __forceinline__ Words words_of(uint32_t words)
{
	const Share sh = share_of((words + kTileWords - 1) / kTileWords);
	return Words{ sh.t_begin * kTileWords, min(sh.t_end * kTileWords, words) };
}

// ------------------------------------------------------------------ starts

__global__ __launch_bounds__(kThreads) void k_norm_starts(NormArgs g, uint32_t *start_bits)
{
	for (uint32_t k = blockIdx.x * kThreads + threadIdx.x; k < g.segments; k += gridDim.x * kThreads) {
		const int64_t x = max(g.origin, min((int64_t)g.seg_start[k], g.origin + (int64_t)g.n)) - g.origin;   // in [0, n]
		if (x > 0 && x < (int64_t)g.n)   // (byte 0 starts a text anyway; a start at n cuts nothing)
			atomicOr(&start_bits[((uint32_t)x >> 5) + 1], 1u << ((uint32_t)x & 31));   // a set of bits: no order
	}
}

// ------------------------------------------------------------------ mask

struct Kept {
	uint64_t emit, ustart, head, ublank;
};

// keep word w < words: the classification of bytes [64 w, 64 w + 64)
__device__ __forceinline__ Kept classify(const NormArgs &g, const uint8_t *btab, uint32_t w, const uint4 (&v)[4])
{
	const uint32_t b0 = w * 64;
	const uint32_t left = g.n - b0;   // >= 1
	const uint64_t V = left >= 64 ? ~0ull : (1ull << left) - 1;
	const uint32_t d[16] = { v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w,
		                     v[2].x, v[2].y, v[2].z, v[2].w, v[3].x, v[3].y, v[3].z, v[3].w };
	// the text starts: bit i of ST: a text starts at byte b0 + i; 32 bits in front and behind
	uint64_t ST = w == 0 ? 1 : 0;
	uint32_t st_prev = 0, st_next = 0;
	if (g.start_bits) {
		const uint32_t *sb = g.start_bits + 2 * w;   // (bit 32 + i: the cell in front of word 0 is 0)
		st_prev = sb[0];
		ST |= (uint64_t)sb[1] | (uint64_t)sb[2] << 32;
		st_next = sb[3];
	}
	uint64_t P = 0, H = 0, B = 0;
	uint32_t prev = 0;   // the dword in front: bytes b0 - 4 .. b0 - 1
	if (w > 0)
		prev = *(const uint32_t *)(g.text + b0 - 4);
	if (g.percent) {
#pragma unroll
		for (int k = 0; k < 16; k++)
			P |= (uint64_t)eq4(d[k], 0x25252525u) << (4 * k);
		P &= V;
	}
	uint32_t p_prev = 0, h_prev = 0, h_next = 0;   // bits 0..3: bytes b0 - 4 .. b0 - 1; bits 0..1: bytes b0 + 64, b0 + 65
	if (g.percent)
		p_prev = eq4(prev, 0x25252525u);
	if (P | p_prev) {   // (hex digits matter only behind a '%')
#pragma unroll
		for (int k = 0; k < 16; k++)
			H |= (uint64_t)hex4(d[k]) << (4 * k);
		H &= V;
		h_prev = hex4(prev);
		if (left > 64) {
			h_next = hex4(*(const uint32_t *)(g.text + b0 + 64)) & 3;   // (inside round16(n): readable)
			if (left < 66)
				h_next &= 1;   // the byte at n is no digit
		}
	}
	uint64_t HEAD = 0;
	uint32_t head_prev = 0;   // bit 0: a head at b0 - 3, bit 1: at b0 - 2, bit 2: at b0 - 1
	if (P | p_prev) {
		const uint64_t H1 = H >> 1 | (uint64_t)h_next << 63, H2 = H >> 2 | (uint64_t)h_next << 62;
		const uint64_t S1 = ST >> 1 | (uint64_t)st_next << 63, S2 = ST >> 2 | (uint64_t)st_next << 62;
		HEAD = P & H1 & H2 & ~S1 & ~S2;
		const uint32_t Pw = p_prev | ((uint32_t)P & 0xF) << 4, Hw = h_prev | ((uint32_t)H & 0xF) << 4;
		const uint32_t Sw = st_prev >> 28 | ((uint32_t)ST & 0xF) << 4;
		head_prev = (Pw & Hw >> 1 & Hw >> 2 & ~(Sw >> 1) & ~(Sw >> 2)) >> 1 & 7;
	}
	uint64_t BDEC = 0;        // a head whose value is blank
	uint32_t b_prev = 0, bdec_prev = 0;   // byte b0 - 1 is blank; bit k: the head at b0 - 3 + k decodes to a blank
	if (g.blanks) {
#pragma unroll
		for (int k = 0; k < 16; k++)
			B |= (uint64_t)blank4(btab, d[k]) << (4 * k);
		B &= V;
		if (w > 0)
			b_prev = btab[prev >> 24];
		for (uint64_t h = HEAD; h; h &= h - 1) {
			const uint32_t i = (uint32_t)__ffsll((long long)h) - 1;
			const uint8_t *t = g.text + b0 + i;   // (a head: t[1], t[2] lie inside n)
			BDEC |= (uint64_t)btab[decode(t[1], t[2])] << i;
		}
		for (uint32_t k = 0; k < 3; k++)   // (the digits of the heads at b0 - 2 and b0 - 1 lie in this word)
			if (head_prev >> k & 1) {
				const uint8_t *t = g.text + b0 - 3 + k;
				bdec_prev |= (uint32_t)btab[decode(t[1], t[2])] << k;
			}
	}
	Kept r;
	r.head = HEAD;
	const uint64_t inside = HEAD << 1 | head_prev >> 2 | HEAD << 2 | head_prev >> 1;
	r.ustart = ~inside & V;
	r.ublank = r.ustart & ((~HEAD & B) | BDEC);
	if (g.squeeze) {
		// the unit in front of a unit start i, inside its text: the triple headed at i - 3, else the byte i - 1
		const uint64_t head3 = HEAD << 3 | head_prev;
		const uint64_t prev_blank = ~ST & ((BDEC << 3 | bdec_prev) | (~head3 & (B << 1 | b_prev)));
		r.emit = r.ustart & (~r.ublank | ~prev_blank);
	} else {
		r.emit = r.ustart & ~r.ublank;
	}
	return r;
}

__global__ __launch_bounds__(kThreads) void k_norm_mask(NormArgs g)
{
	__shared__ uint32_t red[kWaves];
	__shared__ uint8_t btab[256];
	fill_table(g.set, btab);
	__syncthreads();
	const Words sh = words_of(g.words);
	const uint32_t groups = (g.n + 15) / 16;
	uint32_t emitted = 0, dropped = 0, triples = 0, blanks = 0;
	for (uint32_t w = sh.w_begin + threadIdx.x; w < sh.w_end; w += kThreads) {
		uint4 v[4];
#pragma unroll
		for (int q = 0; q < 4; q++)
			v[q] = 4 * w + q < groups ? ((const uint4 *)g.text)[4 * w + q] : make_uint4(0, 0, 0, 0);
		const Kept k = classify(g, btab, w, v);
		g.keep[w] = k.emit;
		emitted += (uint32_t)__popcll(k.emit);
		dropped += (uint32_t)__popcll(k.ustart & ~k.emit);
		triples += (uint32_t)__popcll(k.head);
		blanks += (uint32_t)__popcll(k.emit & k.ublank);
	}
	emitted = block_sum(emitted, red);
	dropped = block_sum(dropped, red);
	triples = block_sum(triples, red);
	blanks = block_sum(blanks, red);
	if (threadIdx.x == 0) {
		g.blk[blockIdx.x] = (int32_t)emitted;
		g.blk[kMaxBlocks + blockIdx.x] = (int32_t)dropped;
		g.blk[2 * kMaxBlocks + blockIdx.x] = (int32_t)triples;
		g.blk[3 * kMaxBlocks + blockIdx.x] = (int32_t)blanks;
	}
}

// ------------------------------------------------------------------ write

__global__ __launch_bounds__(kThreads) void k_norm_write(NormArgs g)
{
	__shared__ __attribute__((aligned(16))) uint8_t tile[kTileBytes + 16];
	__shared__ uint64_t wbits[kTileWords];
	__shared__ uint32_t wpre[kTileWords];
	__shared__ uint8_t btab[256];
	__shared__ uint32_t red[2 * kWaves];

	const uint32_t tid = threadIdx.x;
	fill_table(g.set, btab);
	uint32_t m;
	uint32_t base = blocks_before(g.blk, red, m);
	if (blockIdx.x == 0) {
		uint32_t dropped, triples, blanks;
		blocks_before(g.blk + kMaxBlocks, red, dropped);
		blocks_before(g.blk + 2 * kMaxBlocks, red, triples);
		blocks_before(g.blk + 3 * kMaxBlocks, red, blanks);
		if (tid == 0) {
			g.block[(g.n + ACM_NORM_BLOCK - 1) / ACM_NORM_BLOCK] = (int32_t)m;   // (no word's cell: see below)
			g.info[0] = (int32_t)m;
			g.info[1] = (int32_t)dropped;
			g.info[2] = (int32_t)triples;
			g.info[3] = (int32_t)blanks;
			g.info[4] = (g.out && m > g.cap) ? 1 : 0;
			g.info[5] = g.info[6] = g.info[7] = 0;
		}
	}
	const uint32_t limit = g.out ? min(m, g.cap) : 0;
	const Words sh = words_of(g.words);
	const uint32_t *text32 = (const uint32_t *)g.text;
	for (uint32_t w0 = sh.w_begin; w0 < sh.w_end; w0 += kTileWords) {
		const uint32_t w = w0 + tid;
		const uint64_t bits = w < sh.w_end ? g.keep[w] : 0;
		uint32_t tile_total;
		const uint32_t pre = block_prefix((uint32_t)__popcll(bits), red, tile_total);
		// cell j: the output in front of byte 1024 j; the cell behind the text (n a multiple of 1024 or not) is block 0's
		if (w < sh.w_end && w % kWordsPerCell == 0)
			g.block[w / kWordsPerCell] = (int32_t)(base + pre);
		if (base < limit && tile_total > 0) {   // (uniform)
			wbits[tid] = bits;
			wpre[tid] = pre;
			__syncthreads();
			const uint32_t phase = base & 15;   // the tile lies at the output's 16-byte phase
			uint32_t v[kRows];
#pragma unroll
			for (int r = 0; r < kRows; r++) {
				const uint32_t j = (uint32_t)r * kThreads + tid;   // the dword of the tile
				const uint32_t nib = (uint32_t)(wbits[j >> 4] >> (4 * (j & 15))) & 0xF;
				v[r] = nib ? text32[w0 * 16 + j] : 0;   // (a kept byte lies in front of n)
			}
#pragma unroll
			for (int r = 0; r < kRows; r++) {
				const uint32_t j = (uint32_t)r * kThreads + tid;
				const uint64_t word = wbits[j >> 4];
				const uint32_t sh4 = 4 * (j & 15);
				const uint32_t nib = (uint32_t)(word >> sh4) & 0xF;
				if (!nib)
					continue;
				uint32_t at = phase + wpre[j >> 4] + (uint32_t)__popcll(word & ((1ull << sh4) - 1));
#pragma unroll
				for (int c = 0; c < 4; c++) {
					if (!(nib >> c & 1))
						continue;
					uint32_t b = v[r] >> (8 * c) & 0xFF;
					if (g.percent && b == '%') {
						const uint32_t p = (w0 * 16 + j) * 4 + c;
						if (is_head(g.text, g.n, g.start_bits, p))
							b = decode(g.text[p + 1], g.text[p + 2]);
					}
					if (g.squeeze && btab[b])
						b = g.blank_byte;
					tile[at++] = (uint8_t)b;
				}
			}
			__syncthreads();
			// the tile's bytes are output [base, base + tile_total), in LDS from `phase` on
			const uint32_t a0 = base - phase, o1 = min(base + tile_total, limit);
			for (uint32_t x0 = a0 + tid * 16; x0 < o1; x0 += kThreads * 16) {
				if (x0 >= base && x0 + 16 <= o1) {
					*(uint4 *)(g.out + x0) = *(const uint4 *)(tile + (x0 - a0));
				} else {
					for (uint32_t c = 0; c < 16; c++)
						if (x0 + c >= base && x0 + c < o1)
							g.out[x0 + c] = tile[x0 - a0 + c];
				}
			}
			__syncthreads();   // (the tile and the words are no longer read)
		}
		base += tile_total;
	}
}

// ------------------------------------------------------------------ the output in front of a byte

// output bytes emitted by the input in front of byte x <= n
__device__ __forceinline__ uint32_t emitted_before(const uint64_t *keep, const int32_t *block, uint32_t x)
{
	const uint32_t cell = x / ACM_NORM_BLOCK;
	uint32_t c = (uint32_t)block[cell];
	const uint32_t w_x = x / 64;
	for (uint32_t w = cell * kWordsPerCell; w < w_x; w++)
		c += (uint32_t)__popcll(keep[w]);
	if (x % 64)
		c += (uint32_t)__popcll(keep[w_x] & ((1ull << (x % 64)) - 1));
	return c;
}

__global__ __launch_bounds__(kThreads) void k_norm_seg(NormArgs g)
{
	const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
	if (k >= g.segments)
		return;
	const int64_t x = max(g.origin, min((int64_t)g.seg_start[k], g.origin + (int64_t)g.n)) - g.origin;   // in [0, n]
	g.seg_out[k] = (int32_t)emitted_before(g.keep, g.block, (uint32_t)x);
}

// ------------------------------------------------------------------ remap

struct RemapArgs {
	const uint8_t *text;
	uint32_t n, words, cells;      // bytes; keep words; d_block cells
	int64_t origin;
	uint32_t percent;
	const uint64_t *keep;
	const int32_t *block;
	const int32_t *pat_plane, *off_plane;
	uint32_t R;
	const uint32_t *pat_len;
	const int4 *wild_ent;
	uint32_t num_patterns;
	int32_t *off_out, *start_out;
	int32_t *info;
};

// the k-th set bit of x (k < popcount)
__device__ __forceinline__ uint32_t select64(uint64_t x, uint32_t k)
{
	uint32_t pos = 0;
#pragma unroll
	for (uint32_t s = 32; s > 0; s >>= 1) {
		const uint32_t c = (uint32_t)__popcll(x & ((1ull << s) - 1));
		if (k >= c) {
			k -= c;
			x >>= s;
			pos += s;
		}
	}
	return pos;
}

// the input byte that emitted output byte o, 0 <= o < m; n when the map does not hold it (planes that are not the
// normalise call's)
__device__ __forceinline__ uint32_t emitter(const RemapArgs &g, uint32_t o)
{
	const uint32_t ub = upper_bound_i32(g.block, g.cells, (int32_t)o);   // >= 1: cell 0 is 0
	if (ub == 0 || ub >= g.cells)
		return g.n;
	const uint32_t cell = ub - 1;
	uint32_t r = o - (uint32_t)g.block[cell];
	const uint32_t w_end = min((cell + 1) * kWordsPerCell, g.words);
	for (uint32_t w = cell * kWordsPerCell; w < w_end; w++) {
		const uint64_t bits = g.keep[w];
		const uint32_t c = (uint32_t)__popcll(bits);
		if (r < c)
			return min(w * 64 + select64(bits, r), g.n);
		r -= c;
	}
	return g.n;
}

__global__ __launch_bounds__(kThreads) void k_norm_remap(RemapArgs g)
{
	const uint32_t cnt = (uint32_t)min((int64_t)max(g.off_plane[0], 0), (int64_t)g.R);
	const uint32_t m = (uint32_t)max(g.block[g.cells - 1], 0);
	uint32_t bad = 0;
	for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < cnt; i += gridDim.x * kThreads) {
		const int32_t o = g.off_plane[1 + i];
		int32_t last = -1, first = -1;
		bool ok = false;
		if (o >= 0 && (uint32_t)o < m) {
			const uint32_t p = emitter(g, (uint32_t)o);
			if (p < g.n) {
				// a triple's digits emit nothing; a '%' in front of two digits that are units would have them kept
				uint32_t len = 1;
				if (g.percent && g.text[p] == '%' && p + 2 < g.n && is_hex(g.text[p + 1]) && is_hex(g.text[p + 2]) &&
				    !(g.keep[(p + 1) / 64] >> ((p + 1) % 64) & 1) && !(g.keep[(p + 2) / 64] >> ((p + 2) % 64) & 1))
					len = 3;
				last = sat32(g.origin + p + len - 1);
				ok = true;
			}
		}
		if (g.start_out) {
			bool got_first = false;
			const Span sp = span_of(g.pat_len, g.wild_ent, g.num_patterns, (uint32_t)g.pat_plane[1 + i], o);
			if (sp.ok && sp.s >= 0 && sp.s < (int64_t)m) {
				const uint32_t p = emitter(g, (uint32_t)sp.s);
				if (p < g.n) {
					first = sat32(g.origin + p);
					got_first = true;
				}
			}
			ok = ok && got_first;
			g.start_out[1 + i] = first;
		}
		g.off_out[1 + i] = last;
		bad += ok ? 0 : 1;
	}
	// a sum: no order is decided here
	for (int s = 32; s > 0; s >>= 1)
		bad += __shfl_xor(bad, s, 64);
	if (lane_id() == 0 && bad)
		atomicAdd(&g.info[1], (int32_t)bad);
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		atomicAdd(&g.info[0], (int32_t)cnt);
		if (g.off_out != g.off_plane)   // (in place the count cell stays what it is: an overflow stays visible)
			g.off_out[0] = (int32_t)cnt;
		if (g.start_out)
			g.start_out[0] = (int32_t)cnt;
	}
}

// ------------------------------------------------------------------ host side

// blocks of the fixed grid: four per CU of the current device, kMaxBlocks at most (as lines.hip)
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

constexpr size_t kBlkBytes = 4 * kMaxBlocks * sizeof(int32_t);

// the start bits: bit 32 + i, 32 bits of room in front of byte 0 and behind the last word
size_t start_bit_bytes(size_t n) { return (2 * ((n + 63) / 64) + 2) * sizeof(uint32_t); }

}  // namespace

extern "C" size_t acm_normalize_workspace_bytes(size_t max_text, size_t segments)
{
	return round256(kBlkBytes) + (segments ? round256(start_bit_bytes(max_text)) : 0);
}

extern "C" int acm_normalize_async(const void *d_text, size_t n, long text_origin, unsigned flags, const uint8_t *blank_mask,
    int blank_byte, void *d_out, size_t out_capacity, uint64_t *d_keep, int32_t *d_block, const int32_t *d_seg_start,
    size_t segments, int32_t *d_seg_out, int32_t *d_info, void *d_workspace, size_t workspace_bytes, void *stream)
{
	if (!d_info || !d_keep || !d_block || (!d_text && n > 0) || ((uintptr_t)d_text & 15) || ((uintptr_t)d_out & 15) ||
	    ((uintptr_t)d_keep & 7) || n > kMaxBytes || out_capacity > kMaxBytes || (!d_out && out_capacity > 0) ||
	    segments > 0x7FFFFFFFul || text_origin < (long)INT32_MIN || text_origin > (long)INT32_MAX)
		return acm::fail(ACM_ERR_ARG, "acm_normalize_async: bad arguments");
	if ((segments > 0) != (d_seg_start != nullptr) || (segments > 0) != (d_seg_out != nullptr))
		return acm::fail(ACM_ERR_ARG, "acm_normalize_async: segments without both arrays, or arrays without segments");
	if (flags & ~kKnownFlags)
		return acm::fail(ACM_ERR_ARG, "acm_normalize_async: unknown flag bits 0x%x", flags);
	if ((flags & ACM_NORM_SQUEEZE) && (flags & ACM_NORM_STRIP))
		return acm::fail(ACM_ERR_ARG, "acm_normalize_async: squeeze and strip exclude each other");
	if ((flags & ACM_NORM_SQUEEZE) && (blank_byte < 0 || blank_byte > 255))
		return acm::fail(ACM_ERR_ARG, "acm_normalize_async: blank_byte %d outside 0..255", blank_byte);
	const size_t need = acm_normalize_workspace_bytes(n, segments);
	if (!d_workspace || workspace_bytes < need)
		return acm::fail(ACM_ERR_ARG, "acm_normalize_async: workspace %zu B < required %zu B", workspace_bytes, need);
	hipStream_t s = (hipStream_t)stream;
	uint32_t blocks = 0;
	if (int rc = fixed_grid(&blocks))
		return rc;

	NormArgs g{};
	g.text = (const uint8_t *)d_text;
	g.n = (uint32_t)n;
	g.words = (uint32_t)((n + 63) / 64);
	g.origin = (int64_t)text_origin;
	g.percent = (flags & ACM_NORM_PERCENT) ? 1 : 0;
	g.squeeze = (flags & ACM_NORM_SQUEEZE) ? 1 : 0;
	g.blanks = (flags & (ACM_NORM_SQUEEZE | ACM_NORM_STRIP)) ? 1 : 0;
	g.blank_byte = g.squeeze ? (uint32_t)blank_byte : 0;
	if (g.blanks) {
		static const uint8_t kDefault[32] = { 0x00, 0x3E, 0x00, 0x00, 0x01 };   // 09 0a 0b 0c 0d 20
		const uint8_t *mask = blank_mask ? blank_mask : kDefault;
		for (int i = 0; i < 32; i++)
			g.set.w[i / 4] |= (uint32_t)mask[i] << (8 * (i % 4));
	}
	g.seg_start = d_seg_start;
	g.segments = (uint32_t)segments;
	g.blk = (int32_t *)d_workspace;
	uint32_t *start_bits = segments ? (uint32_t *)((char *)d_workspace + round256(kBlkBytes)) : nullptr;
	g.start_bits = start_bits;
	g.keep = d_keep;
	g.block = d_block;
	g.out = (uint8_t *)d_out;
	g.cap = (uint32_t)out_capacity;
	g.seg_out = d_seg_out;
	g.info = d_info;

	const dim3 grid(blocks), block(kThreads);
	if (segments > 0) {
		ACM_HIP_TRY(hipMemsetAsync(start_bits, 0, start_bit_bytes(n), s));
		const uint32_t sb = (uint32_t)std::max<size_t>(1, std::min<size_t>(blocks, (segments + kThreads - 1) / kThreads));
		hipLaunchKernelGGL(k_norm_starts, dim3(sb), block, 0, s, g, start_bits);
		ACM_HIP_TRY(hipGetLastError());
	}
	hipLaunchKernelGGL(k_norm_mask, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_norm_write, grid, block, 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	if (segments > 0) {
		hipLaunchKernelGGL(k_norm_seg, dim3((uint32_t)((segments + kThreads - 1) / kThreads)), block, 0, s, g);
		ACM_HIP_TRY(hipGetLastError());
	}
	return ACM_OK;
}

extern "C" int acm_normalize_remap_async(const acm_dfa *d, const void *d_text, size_t n, long text_origin, unsigned flags,
    const uint64_t *d_keep, const int32_t *d_block, const int32_t *d_pat_plane, const int32_t *d_off_plane, size_t max_records,
    int32_t *d_off_out, int32_t *d_start_out, int32_t *d_info, void *stream)
{
	if (!d_keep || !d_block || !d_off_plane || !d_off_out || !d_info || (!d_text && n > 0) || n > kMaxBytes ||
	    ((uintptr_t)d_keep & 7) || max_records > 0x7FFFFFFEul || text_origin < (long)INT32_MIN || text_origin > (long)INT32_MAX ||
	    (flags & ~kKnownFlags) || ((flags & ACM_NORM_SQUEEZE) && (flags & ACM_NORM_STRIP)))
		return acm::fail(ACM_ERR_ARG, "acm_normalize_remap_async: bad arguments");
	if ((d_start_out && !d_pat_plane) || (d_pat_plane && !d))
		return acm::fail(ACM_ERR_ARG, "acm_normalize_remap_async: starts need the pattern plane and the automaton");
	if (d && ((d->num_patterns && !d->d_pat_len) || (d->wild && !d->d_wild_ent)))
		return acm::fail(ACM_ERR_ARG, "acm_normalize_remap_async: automaton without its span tables");
	uint32_t blocks = 0;
	if (int rc = fixed_grid(&blocks))
		return rc;
	RemapArgs g{};
	g.text = (const uint8_t *)d_text;
	g.n = (uint32_t)n;
	g.words = (uint32_t)((n + 63) / 64);
	g.cells = (uint32_t)((n + ACM_NORM_BLOCK - 1) / ACM_NORM_BLOCK + 1);
	g.origin = (int64_t)text_origin;
	g.percent = (flags & ACM_NORM_PERCENT) ? 1 : 0;
	g.keep = d_keep;
	g.block = d_block;
	g.pat_plane = d_pat_plane;
	g.off_plane = d_off_plane;
	g.R = (uint32_t)max_records;
	if (d) {
		g.pat_len = d->d_pat_len;
		g.wild_ent = d->wild ? (const int4 *)d->d_wild_ent : nullptr;
		g.num_patterns = d->num_patterns;
	}
	g.off_out = d_off_out;
	g.start_out = d_pat_plane ? d_start_out : nullptr;
	g.info = d_info;
	hipStream_t s = (hipStream_t)stream;
	ACM_HIP_TRY(hipMemsetAsync(d_info, 0, 8 * sizeof(int32_t), s));
	blocks = (uint32_t)std::max<size_t>(1, std::min<size_t>(blocks, (max_records + kThreads - 1) / kThreads));
	hipLaunchKernelGGL(k_norm_remap, dim3(blocks), dim3(kThreads), 0, s, g);
	ACM_HIP_TRY(hipGetLastError());
	return ACM_OK;
}
