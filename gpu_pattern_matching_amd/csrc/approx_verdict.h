// The Hamming verdict of an approximate pattern's piece: rules 2 - 4 of acm_approx_matches_async, shared by the
// approx pass (approx.hip, which describes the compare) and the edit pass (edit.hip, for the Hamming patterns of a
// set that also holds edit patterns).  Internal to the library, gfx950 only.
#pragma once

#include "case_fold.h"
#include "entry_pass.h"

namespace acm_rp {

constexpr int64_t kEndUnknown = INT64_MIN;

enum { kDrop = 0, kKeep = 1, kUndecided = 2 };

// the pieces of one pattern while its span is walked from the left
struct Pieces {
	int32_t q, r, k, j;
	int32_t pi, pe;        // the open piece and where it ends
	uint32_t m, sum;       // mismatches of the open piece, and of everything so far
	bool dead;

	__device__ __forceinline__ int32_t begin_of(int32_t i) const { return i * q + min(i, r); }

	// cnt <= 4 bytes from pattern position i on: bit 8 t + 7 of nz set = byte t differs
	__device__ __forceinline__ void take(uint32_t nz, int32_t cnt, int32_t i)
	{
		while (cnt > 0) {
			const int32_t t = min(cnt, pe - i);
			const uint32_t c = (uint32_t)__popc(t >= 4 ? nz : nz & ((1u << (8 * t)) - 1u));
			m += c;
			sum += c;
			nz = t >= 4 ? 0u : nz >> (8 * t);
			i += t;
			cnt -= t;
			if (sum > (uint32_t)k || (pi == j && m != 0)) {
				dead = true;
				return;
			}
			if (i == pe) {
				if (pi < j && m == 0) {
					dead = true;
					return;
				}
				pi++;
				pe = begin_of(pi + 1);
				m = 0;
			}
		}
	}
};

// bit 7 of every byte of x that is not 0
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x)
{
	return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}

// entry (p, o) in the text [T0, Tend) (Tend: kEndUnknown); dist: its distance where it is kept.  Reads text only
// inside before ++ text, and of the pool the words of p's pattern and the one behind them.  Args: the pass's
// arguments, with e (EntryArgs), w (TextWindow), ent and pool.
template <class Args>
__device__ __forceinline__ int verdict(const Args &g, uint32_t p, int32_t o, int64_t T0, int64_t Tend, uint32_t &dist)
{
	dist = 0;
	if (p >= g.e.num_patterns)   // (a cell of a HEAD plane may hold anything)
		return kDrop;
	if (g.e.pat_len[p] == 0)
		return kDrop;
	if (!g.ent)
		return kKeep;
	const int4 e = g.ent[p];   // {pool word, n, k | j << 8 | folds << 16, 0}
	if (e.x < 0)
		return kKeep;
	const int32_t n = e.y;
	const bool folds = (e.z >> 16) & 1;
	Pieces ps;
	ps.k = e.z & 0xFF;
	ps.j = (e.z >> 8) & 0xFF;
	ps.q = n / (ps.k + 1);
	ps.r = n % (ps.k + 1);
	const int32_t bj = ps.begin_of(ps.j), ej = ps.begin_of(ps.j + 1);
	const int64_t first = (int64_t)o + 1 - (int64_t)(ej - bj) - (int64_t)bj;   // the span's first byte
	const int64_t last = first + n - 1;                                         // and its last
	if (first < T0 || (Tend != kEndUnknown && last >= Tend))
		return kDrop;
	if (first < g.w.text_origin - g.w.before_len || last >= g.w.text_end)
		return kUndecided;
	ps.pi = 0;
	ps.pe = ps.begin_of(1);
	ps.m = ps.sum = 0;
	ps.dead = false;

	const TextWindow &w = g.w;
	const uint32_t *pw = g.pool + e.x;
	const uint8_t *pb = (const uint8_t *)pw;
	int32_t i = 0;
	// bytes in `before`, then text bytes up to the first aligned text word
	for (; i < n && first + i < w.text_origin && !ps.dead; i++) {
		const uint32_t t = w.before[first + i - (w.text_origin - w.before_len)];
		ps.take(((folds ? acm::fold_byte(t) : t) != pb[i]) ? 0x80u : 0u, 1, i);
	}
	if (ps.dead)
		return kDrop;
	if (i < n) {
		const uint8_t *tp = w.text + (first + i - w.text_origin);
		for (; i < n && ((uintptr_t)tp & 3) && !ps.dead; i++, tp++) {
			const uint32_t t = *tp;
			ps.take(((folds ? acm::fold_byte(t) : t) != pb[i]) ? 0x80u : 0u, 1, i);
		}
		if (i + 4 <= n && !ps.dead) {
			uint32_t wi = (uint32_t)i >> 2;
			const uint32_t shift = (uint32_t)i & 3;
			uint32_t lo = pw[wi];
			auto diff = [&](uint32_t t, uint32_t hi, uint32_t lo) {
				return nonzero_bytes((folds ? acm::fold32(t) : t) ^ __builtin_amdgcn_alignbyte(hi, lo, shift));
			};
			// four words a step: their eight loads do not wait for each other, only the counting is a chain (a
			// pattern that matches is walked to its end by one lane while its wave waits)
			for (; i + 16 <= n && !ps.dead; i += 16, tp += 16, wi += 4) {
				const uint32_t h0 = pw[wi + 1], h1 = pw[wi + 2], h2 = pw[wi + 3], h3 = pw[wi + 4];   // (at most the spare word)
				const uint32_t *tw = (const uint32_t *)tp;
				const uint32_t t0 = tw[0], t1 = tw[1], t2 = tw[2], t3 = tw[3];
				ps.take(diff(t0, h0, lo), 4, i);
				if (!ps.dead)
					ps.take(diff(t1, h1, h0), 4, i + 4);
				if (!ps.dead)
					ps.take(diff(t2, h2, h1), 4, i + 8);
				if (!ps.dead)
					ps.take(diff(t3, h3, h2), 4, i + 12);
				lo = h3;
			}
			for (; i + 4 <= n && !ps.dead; i += 4, tp += 4) {
				const uint32_t hi = pw[++wi];   // (at most the spare word behind the pattern's own)
				ps.take(diff(*(const uint32_t *)tp, hi, lo), 4, i);
				lo = hi;
			}
		}
		for (; i < n && !ps.dead; i++, tp++) {
			const uint32_t t = *tp;
			ps.take(((folds ? acm::fold_byte(t) : t) != pb[i]) ? 0x80u : 0u, 1, i);
		}
	}
	if (ps.dead)
		return kDrop;
	dist = ps.sum;
	return kKeep;
}

}  // namespace acm_rp
