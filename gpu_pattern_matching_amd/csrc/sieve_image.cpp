// Construction of the sparse pipeline's tables (sieve_image.h) and their self-test.  Host code only.
#include "sieve_image.h"

#include "case_fold.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <unordered_map>

namespace acm {

// in_byte as uploaded: the byte on the trie edge into each state, device numbering, and 224 bytes of room behind
// (the followers read up to 192 bytes past a state's own)
std::vector<uint8_t> device_in_byte(const acm_automaton &a)
{
	std::vector<uint8_t> inb((size_t)a.num_states + 224, 0);
	for (uint32_t s = 0; s < a.num_states; s++)
		inb[s] = a.in_byte[a.dev2ref[s]];
	return inb;
}

// sparse stays off (applies / ok false) for sets the pipeline does not apply to: a pattern shorter
// than 3 bytes, none at all, or more edges than a record can index.
void build_sieve_image(const acm_automaton &a, SieveImage &img)
{
	img = SieveImage();
	size_t shortest = SIZE_MAX;
	for (const auto &p : a.patterns)
		shortest = std::min(shortest, p.bytes.size());
	if (a.patterns.empty() || shortest < 3)
		return;
	img.applies = true;
	const uint32_t n = a.num_states;
	uint32_t W = acm::sieve_stride((uint32_t)std::min<size_t>(shortest, 64));
	if (const char *e = getenv("ACM_SIEVE_STRIDE")) {   // debugging aid: a smaller stride than the set allows
		const uint32_t v = (uint32_t)atoi(e);
		if ((v == 1 || v == 2 || v == 4 || v == 8) && v <= W)
			W = v;
	}
	const uint32_t D = (uint32_t)std::min<size_t>(shortest, acm::kSieveMaxPrefix);
	img.W = W;
	img.D = D;
	// runs of one byte that can start a pattern: D copies of b down the trie
	for (uint32_t b = 0; b < 256; b++) {
		uint32_t s = 0, k = 0;
		for (; k < D; k++) {
			uint32_t next = UINT32_MAX;
			for (uint32_t e = a.child_begin[s]; e < a.child_begin[s + 1]; e++)
				if (a.child_list[e].byte == b)
					next = a.child_list[e].to;
			if (next == UINT32_MAX)
				break;
			s = next;
		}
		if (k == D)
			img.run_ok[b >> 5] |= 1u << (b & 31);
	}
	if (a.nocase)   // (the bulk kernel tests a run of raw bytes: a run of 'a' is one of 'A')
		for (uint32_t b = 'a'; b <= 'z'; b++)
			if ((img.run_ok[acm::fold_byte(b) >> 5] >> (acm::fold_byte(b) & 31)) & 1u)
				img.run_ok[b >> 5] |= 1u << (b & 31);

	// 3-grams at offsets < W of every pattern, with the offsets they occur at
	std::unordered_map<uint32_t, uint32_t> grams;
	grams.reserve(a.patterns.size() * W * 2);
	for (const auto &p : a.patterns)
		for (uint32_t o = 0; o < W; o++) {
			const uint32_t g = (uint32_t)p.bytes[o] | ((uint32_t)p.bytes[o + 1] << 8) | ((uint32_t)p.bytes[o + 2] << 16);
			grams[g] |= 1u << o;
		}
	img.num_grams = (uint32_t)grams.size();
	// the filter's keys: the 3-grams, or the 6 bytes at the sampled offsets where every pattern has them
	const uint32_t LG = (W + 5 <= shortest && W >= 4) ? 6u : 3u;
	img.LG = LG;
	std::unordered_map<uint64_t, bool> fkeys;
	for (const auto &p : a.patterns)
		for (uint32_t o = 0; o < W; o++) {
			const uint64_t g3 = (uint32_t)p.bytes[o] | ((uint32_t)p.bytes[o + 1] << 8) | ((uint32_t)p.bytes[o + 2] << 16);
			const uint64_t m3 = LG == 6 ? (uint32_t)p.bytes[o + 3] | ((uint32_t)p.bytes[o + 4] << 8) | ((uint32_t)p.bytes[o + 5] << 16) : 0u;
			fkeys[g3 | (m3 << 24)] = true;
		}
	img.num_keys = (uint32_t)fkeys.size();
	uint32_t lw = acm::kSieveMinLogWords;
	while (lw < acm::kSieveMaxLogWords && ((size_t)1 << lw) < fkeys.size())
		lw++;
	if (const char *e = getenv("ACM_BLOOM_LOG_WORDS")) {   // debugging aid
		const int v = atoi(e);
		if (v >= (int)acm::kSieveMinLogWords && v <= (int)acm::kSieveMaxLogWords)
			lw = (uint32_t)v;
	}
	img.bloom_log_words = lw;
	std::vector<uint32_t> &bloom = img.bloom;
	bloom.assign((size_t)1 << lw, 0);
	for (const auto &kv : fkeys) {
		const uint32_t g3 = (uint32_t)(kv.first & 0xFFFFFFu), m3 = (uint32_t)(kv.first >> 24);
		const uint32_t blk = acm::sieve_bloom_block(g3, m3, lw);
		const uint64_t bits = acm::sieve_bloom_bits(g3, m3);
		bloom[2 * blk] |= (uint32_t)bits;
		bloom[2 * blk + 1] |= (uint32_t)(bits >> 32);
	}

	// gram table: buckets of four, one gram per bucket on average (a full bucket costs the
	// lookup a second, dependent load: 2 % of the buckets)
	uint32_t lb = 4;
	while (((size_t)1 << lb) < grams.size())
		lb++;
	std::vector<uint32_t> &gt = img.gram;
	gt.assign((size_t)4 << lb, 0);
	uint32_t gprobes = 1;
	for (const auto &kv : grams) {
		uint32_t b = acm::sieve_gram_bucket(kv.first, lb), probes = 1;
		for (;; b = (b + 1) & ((1u << lb) - 1), probes++) {
			uint32_t *slot = &gt[(size_t)b * 4];
			int k = 0;
			while (k < 4 && slot[k] != 0)
				k++;
			if (k < 4) {
				slot[k] = kv.first | (kv.second << 24);
				break;
			}
		}
		gprobes = std::max(gprobes, probes);
	}
	img.gram_log_buckets = lb;
	img.gram_probes = gprobes;

	// prefix table: every depth-D node under its D path bytes
	std::vector<uint32_t> nodes;
	for (uint32_t r = 0; r < n; r++)
		if (a.depth[r] == D)
			nodes.push_back(r);
	uint32_t ls = 4;   // an eighth full: a lookup ends at the first slot it reads, nearly always
	while (((size_t)1 << ls) < 8 * nodes.size())
		ls++;
	std::vector<uint32_t> &pt = img.prefix;
	pt.assign((size_t)4 << ls, 0);
	uint32_t pprobes = 1;
	for (uint32_t r : nodes) {
		uint8_t key[12] = { 0 };
		uint32_t s = r;
		for (uint32_t k = D; k-- > 0; s = a.parent[s])
			key[k] = a.in_byte[s];
		uint32_t k0, k1, k2;
		memcpy(&k0, key, 4);
		memcpy(&k1, key + 4, 4);
		memcpy(&k2, key + 8, 4);
		const uint32_t dev = a.ref2dev[r];
		uint32_t at = acm::sieve_prefix_slot(k0, k1, k2, ls), probes = 1;
		while (pt[(size_t)at * 4 + 3] != 0) {
			at = (at + 1) & ((1u << ls) - 1);
			probes++;
		}
		pt[(size_t)at * 4 + 0] = k0;
		pt[(size_t)at * 4 + 1] = k1;
		pt[(size_t)at * 4 + 2] = k2 | ((uint32_t)a.dev_run[dev] << 16);
		pt[(size_t)at * 4 + 3] = dev;
		pprobes = std::max(pprobes, probes);
	}
	img.prefix_log_slots = ls;
	img.prefix_probes = pprobes;

	// node records and edges
	std::vector<acm::SieveRec> &rec = img.rec, &edges = img.edges;
	rec.assign(n, acm::sieve_rec(0, 0, 0, false, 0, 0, 0));
	for (uint32_t dev = 0; dev < n; dev++) {
		const uint32_t r = a.dev2ref[dev];
		const uint32_t cb = a.child_begin[r], ce = a.child_begin[r + 1], nc = ce - cb;
		auto leaf = [&](uint32_t child_ref) { return a.child_begin[child_ref + 1] == a.child_begin[child_ref]; };
		auto outp = [&](uint32_t child_ref) { return a.is_final_ref(child_ref) ? (uint32_t)a.head_of(child_ref) : 0xFFFFFFFFu; };
		if (nc == 1) {
			const uint32_t c = a.child_list[cb].to, cd = a.ref2dev[c];
			rec[dev] = acm::sieve_rec(cd, a.child_list[cb].byte, 1, leaf(c), a.dev_run[cd], outp(c), c);
		} else if (nc >= 2) {
			rec[dev] = acm::sieve_rec((uint32_t)edges.size(), 0, nc, false, 0, 0, 0);
			for (uint32_t e = cb; e < ce; e++) {
				const uint32_t c = a.child_list[e].to, cd = a.ref2dev[c];
				edges.push_back(acm::sieve_edge(a.child_list[e].byte, cd, leaf(c), a.dev_run[cd], outp(c), c));
			}
		}
	}
	if (edges.size() >= (1u << 24))
		return;   // edge index does not fit a record: the set stays on the chain pipeline
	edges.push_back(acm::sieve_edge(0, 0, false, 0, 0, 0));
	img.ok = true;
}

namespace {

// ---- the lookups restated: plain serial code over the image, by the layout sieve_tables.h documents
// and the probe bounds the image records (what the kernels of sparse.hip are given) ----

// offset mask of a 3-gram, 0: not in the table
uint32_t gram_lookup(const SieveImage &t, uint32_t gram)
{
	const uint32_t mask = (1u << t.gram_log_buckets) - 1u;
	uint32_t b = t.gram_log_buckets ? (uint32_t)(((uint64_t)(gram & 0xFFFFFFu) * kSieveMulC) & 0xFFFFFFFFu) >> (32 - t.gram_log_buckets) : 0u;
	for (uint32_t probe = 0; probe < t.gram_probes; probe++, b = (b + 1) & mask) {
		bool room = false;
		for (uint32_t k = 0; k < 4; k++) {
			const uint32_t e = t.gram[(size_t)b * 4 + k];
			if (e == 0)
				room = true;
			else if ((e & 0xFFFFFFu) == gram)
				return e >> 24;
		}
		if (room)
			return 0;
	}
	return 0;
}

// slot index of a key (its bytes beyond D zero), -1: not in the table
long prefix_lookup(const SieveImage &t, const uint8_t key[12])
{
	uint32_t k0, k1, k2;
	memcpy(&k0, key, 4);
	memcpy(&k1, key + 4, 4);
	memcpy(&k2, key + 8, 4);
	uint32_t h = k0 * 0x9E3779B1u;
	h = (h ^ (h >> 15) ^ k1) * 0x85EBCA6Bu;
	h = (h ^ (h >> 13) ^ k2) * 0xC2B2AE35u;
	const uint32_t mask = (1u << t.prefix_log_slots) - 1u;
	uint32_t at = t.prefix_log_slots ? h >> (32 - t.prefix_log_slots) : 0u;
	for (uint32_t probe = 0; probe < t.prefix_probes; probe++, at = (at + 1) & mask) {
		const uint32_t *s = &t.prefix[(size_t)at * 4];
		if (s[3] == 0)
			return -1;
		if (s[0] == k0 && s[1] == k1 && (s[2] & 0xFFFFu) == k2)
			return (long)at;
	}
	return -1;
}

// block index and the four bits of a filter key
uint32_t mul24_plain(uint32_t a, uint32_t b) { return (uint32_t)((uint64_t)(a & 0xFFFFFFu) * (b & 0xFFFFFFu)); }
uint32_t bloom_block_of(uint32_t gram, uint32_t more, uint32_t log_words)
{
	return (mul24_plain(gram, 0x9E3779u) + mul24_plain(more, 0xB5297Bu)) >> (33 - log_words);
}
uint64_t bloom_bits_of(uint32_t gram, uint32_t more)
{
	const uint32_t p = mul24_plain(gram, 0x85EBCAu) + mul24_plain(more, 0x68E31Du);
	const uint64_t lo = (1ull << (p >> 27)) | (1ull << ((p >> 22) & 31)), hi = (1ull << ((p >> 17) & 31)) | (1ull << ((p >> 12) & 31));
	return lo | (hi << 32);
}

uint32_t fnv1a(const void *p, size_t bytes)
{
	uint32_t h = 2166136261u;
	for (size_t i = 0; i < bytes; i++)
		h = (h ^ ((const uint8_t *)p)[i]) * 16777619u;
	return h;
}

#define SV_FAIL(...)                                  \
	do {                                          \
		acm::fail(ACM_ERR_LIMIT, __VA_ARGS__); \
		return -1;                            \
	} while (0)

int check_image(const acm_automaton &a, const SieveImage &t, uint32_t *max_fan, uint32_t *max_run)
{
	const std::vector<uint8_t> inb = device_in_byte(a);   // what acm_dfa_upload uploads as in_byte
	const uint32_t W = t.W, D = t.D, n = a.num_states;
	// grams: every pattern's at every offset, and nothing else
	std::map<uint32_t, uint32_t> want;
	for (const auto &p : a.patterns)
		for (uint32_t o = 0; o < W; o++)
			want[(uint32_t)p.bytes[o] | ((uint32_t)p.bytes[o + 1] << 8) | ((uint32_t)p.bytes[o + 2] << 16)] |= 1u << o;
	for (size_t pi = 0; pi < a.patterns.size(); pi++)
		for (uint32_t o = 0; o < W; o++) {
			const auto &p = a.patterns[pi].bytes;
			const uint32_t g = (uint32_t)p[o] | ((uint32_t)p[o + 1] << 8) | ((uint32_t)p[o + 2] << 16);
			const uint32_t m = gram_lookup(t, g);
			if (!((m >> o) & 1u))
				SV_FAIL("sieve tables: gram table: 3-gram %06x of pattern %zu at offset %u: mask %02x found within %u buckets",
				    g, pi, o, m, t.gram_probes);
		}
	size_t entries = 0;
	for (uint32_t e : t.gram) {
		if (!e)
			continue;
		entries++;
		const auto it = want.find(e & 0xFFFFFFu);
		if (it == want.end() || it->second != (e >> 24))
			SV_FAIL("sieve tables: gram table: entry %08x has offset bits no pattern justifies (want mask %02x)", e,
			    it == want.end() ? 0u : it->second);
	}
	if (entries != want.size() || t.num_grams != want.size())
		SV_FAIL("sieve tables: gram table: %zu entries for %zu 3-grams", entries, want.size());
	// filter keys
	std::set<uint64_t> keys;
	for (size_t pi = 0; pi < a.patterns.size(); pi++)
		for (uint32_t o = 0; o < W; o++) {
			const auto &p = a.patterns[pi].bytes;
			const uint32_t g3 = (uint32_t)p[o] | ((uint32_t)p[o + 1] << 8) | ((uint32_t)p[o + 2] << 16);
			const uint32_t m3 = t.LG == 6 ? (uint32_t)p[o + 3] | ((uint32_t)p[o + 4] << 8) | ((uint32_t)p[o + 5] << 16) : 0u;
			keys.insert((uint64_t)g3 | ((uint64_t)m3 << 24));
			const uint32_t blk = bloom_block_of(g3, m3, t.bloom_log_words);
			const uint64_t bits = bloom_bits_of(g3, m3);
			const uint64_t have = (uint64_t)t.bloom[2 * (size_t)blk] | ((uint64_t)t.bloom[2 * (size_t)blk + 1] << 32);
			if ((have & bits) != bits)
				SV_FAIL("sieve tables: filter: key %06x:%06x of pattern %zu at offset %u lacks a bit in block %u", g3, m3, pi, o, blk);
		}
	if (keys.size() != t.num_keys)
		SV_FAIL("sieve tables: filter: %u keys recorded, the patterns have %zu", t.num_keys, keys.size());
	// prefix table
	size_t nodes = 0, occupied = 0;
	for (uint32_t r = 0; r < n; r++) {
		if (a.depth[r] != D)
			continue;
		nodes++;
		uint8_t key[12] = { 0 };
		uint32_t s = r;
		for (uint32_t k = D; k-- > 0; s = a.parent[s])
			key[k] = a.in_byte[s];
		const long at = prefix_lookup(t, key);
		if (at < 0)
			SV_FAIL("sieve tables: prefix table: node %u not found within %u slots", r, t.prefix_probes);
		const uint32_t dev = a.ref2dev[r];
		if (t.prefix[(size_t)at * 4 + 3] != dev)
			SV_FAIL("sieve tables: prefix table: node %u: slot %ld names state %u, not %u", r, at, t.prefix[(size_t)at * 4 + 3], dev);
		if ((t.prefix[(size_t)at * 4 + 2] >> 16) != a.dev_run[dev])
			SV_FAIL("sieve tables: prefix table: node %u: run %u, the automaton says %u", r, t.prefix[(size_t)at * 4 + 2] >> 16,
			    (uint32_t)a.dev_run[dev]);
	}
	for (size_t i = 0; i < t.prefix.size(); i += 4)
		occupied += t.prefix[i + 3] != 0;
	if (occupied != nodes)
		SV_FAIL("sieve tables: prefix table: %zu slots taken for %zu nodes", occupied, nodes);
	// records, edges, runs
	*max_fan = *max_run = 0;
	if (t.rec.size() != n)
		SV_FAIL("sieve tables: %zu records for %u states", t.rec.size(), n);
	for (uint32_t dev = 0; dev < n; dev++) {
		const uint32_t r = a.dev2ref[dev];
		const uint32_t cb = a.child_begin[r], nc = a.child_begin[r + 1] - cb;
		const SieveRec &q = t.rec[dev];
		if (a.depth[r] >= D) {
			*max_fan = std::max(*max_fan, nc);
			*max_run = std::max<uint32_t>(*max_run, a.dev_run[dev]);
		}
		if ((q.w1 & 0x1FFu) != nc)
			SV_FAIL("sieve tables: rec of state %u: %u children, the trie has %u", dev, q.w1 & 0x1FFu, nc);
		const uint32_t eb = q.w0 & 0xFFFFFFu;
		if (nc >= 2 && (size_t)eb + nc + 1 > t.edges.size())
			SV_FAIL("sieve tables: rec of state %u: edges %u.. beyond the edge list", dev, eb);
		for (uint32_t i = 0; i < nc; i++) {
			const uint32_t c = a.child_list[cb + i].to, cd = a.ref2dev[c];
			const bool leaf = a.child_begin[c + 1] == a.child_begin[c];
			const uint32_t out = a.is_final_ref(c) ? (uint32_t)a.head_of(c) : 0xFFFFFFFFu;
			uint32_t byte, child, run, w2, w3;
			bool lf;
			if (nc == 1) {
				byte = q.w0 >> 24, child = q.w0 & 0xFFFFFFu, run = q.w1 >> 16, lf = (q.w1 >> 9) & 1u, w2 = q.w2, w3 = q.w3;
			} else {
				const SieveRec &e = t.edges[(size_t)eb + i];
				byte = e.w0 & 0xFFu, child = e.w0 >> 8, run = e.w1 & 0xFFFFu, lf = (e.w1 >> 16) & 1u, w2 = e.w2, w3 = e.w3;
				if (i && byte <= (t.edges[(size_t)eb + i - 1].w0 & 0xFFu))
					SV_FAIL("sieve tables: edges of state %u: not sorted by byte at edge %u", dev, i);
			}
			if (byte != a.child_list[cb + i].byte || child != cd || lf != leaf || run != a.dev_run[cd] || w2 != out || w3 != c)
				SV_FAIL("sieve tables: %s of state %u, child %u: byte %u child %u leaf %d run %u out %d ref %u; the trie says %u %u %d %u %d %u",
				    nc == 1 ? "rec" : "edge", dev, i, byte, child, (int)lf, run, (int)w2, w3, (uint32_t)a.child_list[cb + i].byte, cd,
				    (int)leaf, (uint32_t)a.dev_run[cd], (int)out, c);
		}
		// a unary run (prefix slot, rec and edge say how long): the follower compares the text with the uploaded
		// in_byte of dev + 1, dev + 2, ... -- dev + 1 must be the only child, not final, its in_byte the byte on
		// that trie edge; the rest of the run follows from dev + 1's own, one step shorter
		if (a.dev_run[dev]) {
			const uint32_t c = nc == 1 ? a.child_list[cb].to : UINT32_MAX;
			if (c == UINT32_MAX || a.ref2dev[c] != dev + 1 || a.is_final_ref(c) || inb[dev + 1] != a.child_list[cb].byte ||
			    a.dev_run[dev + 1] + 1u != a.dev_run[dev])
				SV_FAIL("sieve tables: in_byte along the run of state %u does not follow the trie", dev);
		}
	}
	return 1;
}

}  // namespace

}  // namespace acm

// Debugging / test entry point (no device needed): see include/acmatch.h.
extern "C" int acm_sieve_selftest(const acm_automaton *a, uint32_t *stats)
{
	if (!a || !a->compiled)
		return acm::fail(ACM_ERR_ARG, "acm_sieve_selftest: automaton not compiled");
	acm::SieveImage t;
	acm::build_sieve_image(*a, t);
	if (stats)
		memset(stats, 0, ACM_SIEVE_STATS * sizeof(uint32_t));
	if (!t.ok)
		return 0;
	uint32_t max_fan = 0, max_run = 0;
	const int rc = acm::check_image(*a, t, &max_fan, &max_run);
	if (stats) {
		uint32_t pop = 0, full = 0, occupied = 0;
		for (uint32_t w : t.bloom)
			pop += (uint32_t)__builtin_popcount(w);
		for (size_t i = 0; i < t.gram.size(); i += 4)
			full += t.gram[i] && t.gram[i + 1] && t.gram[i + 2] && t.gram[i + 3];
		for (size_t i = 0; i < t.prefix.size(); i += 4)
			occupied += t.prefix[i + 3] != 0;
		const uint32_t v[ACM_SIEVE_STATS] = { t.W, t.D, t.LG, t.bloom_log_words, pop, t.num_keys, t.num_grams, t.gram_log_buckets, full,
			t.gram_probes, t.prefix_log_slots, occupied, t.prefix_probes, max_fan, max_run, (uint32_t)t.edges.size() - 1u,
			acm::fnv1a(t.bloom.data(), t.bloom.size() * 4), acm::fnv1a(t.gram.data(), t.gram.size() * 4),
			acm::fnv1a(t.prefix.data(), t.prefix.size() * 4), acm::fnv1a(t.rec.data(), t.rec.size() * sizeof(acm::SieveRec)),
			acm::fnv1a(t.edges.data(), t.edges.size() * sizeof(acm::SieveRec)) };
		memcpy(stats, v, sizeof(v));
	}
	return rc;
}
