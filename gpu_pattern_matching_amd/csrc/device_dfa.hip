// Device-resident DFA: HBM/LDS layout + upload.
//
// Replaces the d_trans half of acsm_gen_state_table (acsmx.c:618-666).  The
// reference ships one int32 [state][2][256] table (2 KiB per state, final
// transitions stored negated, pattern index in a second plane).  Here, in the
// device numbering of acm_internal.h (hot rows, other non-finals in reference
// order, finals last):
//
//   cold   u32 [states][256]    1 KiB rows, next state; "the transition is
//                               final" is  next >= first_final  -- no flag
//                               bits.  The walk kernel reads only this plane.
//   deep   u64 [states][256]    next | depth(next) << 32 | run(next) << 48: what
//                               the exact walks (boundary resolve, sparse
//                               walkers) need about the state they enter
//                               (merge test, fast-forward) comes back in the
//                               same load as the state -- one load, one TLB
//                               entry per step on a latency-bound path.  Costs
//                               2 KiB per state next to the 1 KiB cold row;
//                               HBM is not what this path is short of.
//   hot    u16 [H][256]         rows of the first H (<= 256) non-final states
//                               in BFS order (root, depth 1, ...): copied to
//                               LDS by the walk kernel.  A cell holds the next
//                               state, or 0xFFFF when it does not fit or is
//                               final (the lane then reads the cold plane).
//   out    i32 [states]         pattern index a final state reports (the head
//                               of its match list, acsmx.c:650), -1 otherwise
//   dev2ref u32 [states]        back to the reference's numbering (last_state)
//   in_byte u8 [states + 224]    byte on the trie edge into each state; along
//                               a unary path the states ahead are d+1, d+2, ...
//                               so 16 expected bytes are one contiguous load
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <new>

#include "acm_internal.h"
#include "case_fold.h"
#include "device_dfa.h"
#include "lds_walk.h"
#include "sieve_image.h"
#include "sieve_tables.h"
#include "sparse.h"

extern "C" int acm_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess)
		return 0;
	return n;
}

namespace {

template <typename T>
int upload(T **dptr, const T *src, size_t count, size_t *total)
{
	size_t bytes = (count ? count : 1) * sizeof(T);
	ACM_HIP_TRY(hipMalloc((void **)dptr, bytes));
	if (count)
		ACM_HIP_TRY(hipMemcpy(*dptr, src, count * sizeof(T), hipMemcpyHostToDevice));
	*total += bytes;
	return ACM_OK;
}

// The small tables the latency-bound lookups touch (node records, hash tables, per-state
// arrays) share ONE allocation: a lookup that lands on a page nobody touched lately pays an
// address translation on top of the access, and separate hipMallocs are separate small pages.
template <typename T>
int upload_small(acm_dfa *d, T **dptr, const T *src, size_t count)
{
	const size_t bytes = ((count ? count : 1) * sizeof(T) + 255) & ~(size_t)255;
	if (d->arena && d->arena_used + bytes <= d->arena_bytes) {
		*dptr = (T *)((char *)d->arena + d->arena_used);
		d->arena_used += bytes;
		if (count)
			ACM_HIP_TRY(hipMemcpy(*dptr, src, count * sizeof(T), hipMemcpyHostToDevice));
		return ACM_OK;
	}
	return upload(dptr, src, count, &d->device_bytes);
}

void free_small(acm_dfa *d, void *p)
{
	if (p && !(d->arena && (char *)p >= (char *)d->arena && (char *)p < (char *)d->arena + d->arena_bytes))
		hipFree(p);
}

// Tables of the sparse pipeline, built on the host (sieve_image.cpp) and uploaded as they are.  sparse_ok
// stays false for sets the pipeline does not apply to (a pattern shorter than 3 bytes, or none at all).
int build_sieve(const acm_automaton &a, acm_dfa *d)
{
	d->sparse_ok = false;
	acm::SieveImage img;
	acm::build_sieve_image(a, img);
	if (!img.applies)
		return ACM_OK;
	d->sv_stride = img.W;
	d->sv_prefix_len = img.D;
	memcpy(d->sv_run_ok, img.run_ok, sizeof(d->sv_run_ok));
	d->sv_gram_len = img.LG;
	d->sv_bloom_log_words = img.bloom_log_words;
	d->sv_gram_log_buckets = img.gram_log_buckets;
	d->sv_gram_probes = img.gram_probes;
	d->sv_prefix_log_slots = img.prefix_log_slots;
	d->sv_prefix_probes = img.prefix_probes;
	if (!img.ok)
		return ACM_OK;   // edge index does not fit a record: the set stays on the chain pipeline

	int rc = upload_small(d, &d->d_sv_bloom, img.bloom.data(), img.bloom.size());
	if (rc == ACM_OK) rc = upload_small(d, &d->d_sv_gram, img.gram.data(), img.gram.size());
	if (rc == ACM_OK) rc = upload_small(d, &d->d_sv_prefix, img.prefix.data(), img.prefix.size());
	acm::SieveRec *drec = nullptr, *dedges = nullptr;
	if (rc == ACM_OK) rc = upload_small(d, &drec, img.rec.data(), img.rec.size());
	if (rc == ACM_OK) rc = upload_small(d, &dedges, img.edges.data(), img.edges.size());
	d->d_sv_rec = drec;
	d->d_sv_edges = dedges;
	if (rc == ACM_OK)
		d->sparse_ok = true;
	return rc;
}

}  // namespace

extern "C" int acm_dfa_upload(const acm_automaton *a, int device, acm_dfa **out)
{
	if (!a || !a->compiled || !out)
		return acm::fail(ACM_ERR_ARG, "acm_dfa_upload: automaton not compiled");
	int ndev = acm_device_count();
	if (ndev <= 0)
		return acm::fail(ACM_ERR_NODEV, "acm_dfa_upload: no HIP device visible");
	if (device < 0 || device >= ndev)
		return acm::fail(ACM_ERR_NODEV, "acm_dfa_upload: device %d not in [0,%d)", device, ndev);
	ACM_HIP_TRY(hipSetDevice(device));

	acm_dfa *d = new (std::nothrow) acm_dfa();
	if (!d)
		return acm::fail(ACM_ERR_NOMEM, "acm_dfa_upload: out of host memory");
	d->device = device;
	d->num_states = a->num_states;
	d->first_final = a->first_final;
	d->hot_rows = a->hot_count;
	d->hot_depth1 = a->hot_depth1;
	d->max_pattern_len = (uint32_t)a->max_pattern_len;
	d->nocase = a->nocase;
	d->ref2dev = a->ref2dev;

	int rc = ACM_OK;
	{
		// 48 B per state for the tables below, 8 more for the segment pass's {fail, depth} records, 4 per
		// pattern for the word pass's lengths
		const size_t want = (((size_t)a->num_states * 56 + a->patterns.size() * 4 + (8u << 20)) + (2u << 20) - 1) &
		                    ~(size_t)((2u << 20) - 1);
		if (hipMalloc(&d->arena, want) == hipSuccess) {
			d->arena_bytes = want;
			d->device_bytes += want;
		} else {
			d->arena = nullptr;
			(void)hipGetLastError();
		}
	}
	try {
		const std::vector<uint64_t> &rows = a->dense_rows();
		const uint32_t n = a->num_states, H = a->hot_count, F = a->first_final;

		// the planes of the chain pipeline, one column per byte class (automaton: byte_classes)
		const uint32_t ls = a->log_stride, stride = 1u << ls;
		d->log_stride = ls;
		std::vector<uint64_t> packed;
		if (ls != 8) {
			packed.assign((size_t)n << ls, 0);
			for (uint32_t s = 0; s < n; s++)
				for (uint32_t c = 0; c < stride; c++)
					packed[((size_t)s << ls) | c] = rows[((size_t)s << 8) | a->class_byte[c]];
		}
		const std::vector<uint64_t> &cells = ls != 8 ? packed : rows;
		std::vector<uint16_t> hot((((size_t)H << ls) + 7) & ~(size_t)7, (uint16_t)acm::kHotSentinel);   // whole uint4s
		for (size_t i = 0; i < ((size_t)H << ls); i++) {
			const uint32_t t = (uint32_t)cells[i];
			hot[i] = (uint16_t)((t < acm::kHotSentinel && t < F) ? t : acm::kHotSentinel);
		}
		std::vector<int32_t> outp(n);
		const std::vector<uint8_t> inb = acm::device_in_byte(*a);   // [n + 224] (sieve_image.cpp: the self-test reads the same)
		for (uint32_t s = 0; s < n; s++) {
			const uint32_t r = a->dev2ref[s];
			outp[s] = a->is_final_ref(r) ? a->head_of(r) : -1;
		}
		{
			std::vector<uint32_t> plane(cells.size());
			for (size_t i = 0; i < cells.size(); i++)
				plane[i] = (uint32_t)cells[i];
			rc = upload(&d->d_cold, plane.data(), plane.size(), &d->device_bytes);
			if (rc == ACM_OK)
				rc = upload(&d->d_deep, cells.data(), cells.size(), &d->device_bytes);
			if (rc == ACM_OK)
				rc = upload_small(d, &d->d_class, (const uint8_t *)a->byte_class, (size_t)256);
		}
		if (rc == ACM_OK) rc = upload(&d->d_hot, hot.data(), hot.size(), &d->device_bytes);
		if (rc == ACM_OK) rc = upload_small(d, &d->d_out, outp.data(), outp.size());
		if (rc == ACM_OK)
			rc = upload_small(d, &d->d_dev2ref, a->dev2ref.data(), a->dev2ref.size());
		if (rc == ACM_OK) rc = upload_small(d, &d->d_in_byte, inb.data(), inb.size());
		if (rc == ACM_OK) rc = upload_small(d, &d->d_ref2dev, a->ref2dev.data(), a->ref2dev.size());

		if (rc == ACM_OK) {
			std::vector<uint16_t> dep(n);
			for (uint32_t s = 0; s < n; s++)
				dep[s] = a->depth[a->dev2ref[s]];
			rc = upload_small(d, &d->d_depth, dep.data(), dep.size());
		}
		if (rc == ACM_OK)
			rc = build_sieve(*a, d);
		if (rc == ACM_OK)
			rc = acm::lds_walk_prepare(a, d);
		// match lists, for all-patterns reporting (post.hip, acm_expand_matches_async)
		std::vector<uint32_t> lbegin(n, 0), llen(n, 0);
		for (uint32_t r = 0; r < n; r++)
			if (a->is_final_ref(r)) {
				lbegin[r] = (uint32_t)a->list_begin[r];
				llen[r] = (uint32_t)a->list_len[r];
				d->max_list_len = std::max(d->max_list_len, llen[r]);
			}
		if (rc == ACM_OK) rc = upload(&d->d_list_begin, lbegin.data(), lbegin.size(), &d->device_bytes);
		if (rc == ACM_OK) rc = upload(&d->d_list_len, llen.data(), llen.size(), &d->device_bytes);
		if (rc == ACM_OK) rc = upload(&d->d_list_pool, a->list_pool.data(), a->list_pool.size(), &d->device_bytes);
		// fail link and trie depth of every state, reference numbering: the segment pass clamps a state to
		// the longest suffix that lies inside its segment by walking fail links (segment.hip)
		std::vector<uint32_t> fd((size_t)n * 2);
		for (uint32_t r = 0; r < n; r++) {
			fd[2 * (size_t)r] = a->fail[r];
			fd[2 * (size_t)r + 1] = a->depth[r];
		}
		if (rc == ACM_OK) rc = upload_small(d, &d->d_fail_depth, fd.data(), fd.size());
		// length of every pattern: the word pass finds where a list entry starts (word.hip)
		std::vector<uint32_t> plen(a->patterns.size());
		for (size_t i = 0; i < plen.size(); i++)
			plen[i] = (uint32_t)a->patterns[i].bytes.size();
		d->num_patterns = (uint32_t)plen.size();
		if (rc == ACM_OK) rc = upload_small(d, &d->d_pat_len, plen.data(), plen.size());
		// a mixed automaton: what the case pass needs per pattern (case.hip).  Allocations of their own, so
		// that the arena of a set that is not mixed is used as before.
		d->mixed = a->mixed;
		if (rc == ACM_OK && a->mixed) {
			std::vector<uint32_t> ent(2 * a->patterns.size()), pool;
			for (size_t i = 0; i < a->patterns.size(); i++) {
				const std::vector<unsigned char> &b = a->original[i];
				ent[2 * i + 1] = (uint32_t)b.size();
				if (b.empty()) {
					ent[2 * i] = acm::kCaseNever;
				} else if (a->patterns[i].flags & ACM_PATTERN_NOCASE) {
					ent[2 * i] = acm::kCaseAny;
				} else {
					ent[2 * i] = (uint32_t)pool.size();
					pool.resize(pool.size() + (b.size() + 3) / 4, 0);
					memcpy(&pool[ent[2 * i]], b.data(), b.size());
				}
			}
			pool.push_back(0);   // the word behind the last pattern: the compare loads one word ahead
			rc = upload(&d->d_case_ent, ent.data(), ent.size(), &d->device_bytes);
			if (rc == ACM_OK) rc = upload(&d->d_case_pool, pool.data(), pool.size(), &d->device_bytes);
		}
		// a positioned automaton (acm_automaton_positioned): every pattern's window and length, one 16-byte
		// load per entry of the position pass (position.hip).  An allocation of its own, as above.
		d->positioned = acm_automaton_positioned(a) != 0;
		if (rc == ACM_OK && d->positioned) {
			std::vector<int32_t> ent(4 * a->patterns.size());
			for (size_t i = 0; i < a->patterns.size(); i++) {
				const acm_automaton::Pattern &p = a->patterns[i];
				ent[4 * i] = p.pos_lo;
				ent[4 * i + 1] = p.pos_hi;
				ent[4 * i + 2] = (int32_t)p.pos_flags;
				// (a wildcard pattern's window counts from its first position: acmatch.h)
				ent[4 * i + 3] = p.bytes.empty() ? 0 : (int32_t)p.bytes.size() + p.wild_pre;
			}
			rc = upload(&d->d_pos_ent, ent.data(), ent.size(), &d->device_bytes);
		}
		// an automaton with sequences (acm_automaton_add_sequence): every part is a slot, numbered level by
		// level; per pattern its slot, the gap in front of it and its length, per slot the part in front and,
		// for a last part, the sequence (sequence.hip).  Allocations of their own, as above.
		if (rc == ACM_OK && !a->sequences.empty()) {
			std::vector<int32_t> ent(4 * a->patterns.size()), slot;
			std::vector<int32_t> slot_of(a->patterns.size(), -1);
			for (size_t i = 0; i < a->patterns.size(); i++) {
				ent[4 * i] = -1;
				ent[4 * i + 1] = ent[4 * i + 2] = 0;
				ent[4 * i + 3] = (int32_t)a->patterns[i].bytes.size();
			}
			uint32_t levels = 0;
			for (const auto &s : a->sequences)
				levels = std::max<uint32_t>(levels, (uint32_t)s.parts.size());
			for (uint32_t j = 0; j < levels; j++) {
				d->seq_level_base[j] = (uint32_t)(slot.size() / 2);
				for (size_t q = 0; q < a->sequences.size(); q++) {
					const auto &s = a->sequences[q];
					if (j >= s.parts.size())
						continue;
					const int32_t p = s.parts[j], me = (int32_t)(slot.size() / 2);
					slot_of[p] = me;
					ent[4 * (size_t)p] = me;
					// a wildcard part: the join works on full spans while the records keep the anchors' ends, so
					// the length reaches from the part's first position over the post context of the part in front
					ent[4 * (size_t)p + 3] += a->patterns[p].wild_pre;
					if (j > 0) {
						ent[4 * (size_t)p + 1] = s.gap_lo[j - 1];
						ent[4 * (size_t)p + 2] = s.gap_hi[j - 1];
						ent[4 * (size_t)p + 3] += a->patterns[s.parts[j - 1]].wild_post;
					}
					slot.push_back(j > 0 ? slot_of[s.parts[j - 1]] : -1);
					slot.push_back(j + 1 == s.parts.size() ? (int32_t)q : -1);
				}
			}
			d->seq_levels = levels;
			d->seq_slots = (uint32_t)(slot.size() / 2);
			for (uint32_t j = levels; j <= ACM_SEQ_MAX_PARTS; j++)
				d->seq_level_base[j] = d->seq_slots;
			rc = upload(&d->d_seq_ent, ent.data(), ent.size(), &d->device_bytes);
			if (rc == ACM_OK) rc = upload(&d->d_seq_slot, slot.data(), slot.size(), &d->device_bytes);
		}
		// an automaton with rules (acm_automaton_add_rule): every operand is a slot, numbered rule by rule; per
		// sequence its slot, per slot its rule and operand, per rule its slots and its program (rule.hip).
		// Allocations of their own, as above.
		if (rc == ACM_OK && !a->rules.empty()) {
			std::vector<int32_t> ent(a->sequences.size(), -1), slot, tab, prog;
			for (size_t r = 0; r < a->rules.size(); r++) {
				const auto &rule = a->rules[r];
				tab.insert(tab.end(), { (int32_t)(slot.size() / 2), (int32_t)rule.sequences.size(), (int32_t)(prog.size() / 2),
				                          (int32_t)(rule.code.size() / 2) });
				for (size_t j = 0; j < rule.sequences.size(); j++) {
					ent[rule.sequences[j]] = (int32_t)(slot.size() / 2);
					slot.push_back((int32_t)r);
					slot.push_back((int32_t)j);
				}
				prog.insert(prog.end(), rule.code.begin(), rule.code.end());
			}
			d->rule_slots = (uint32_t)(slot.size() / 2);
			d->num_rules = (uint32_t)a->rules.size();
			d->rule_sequences = (uint32_t)ent.size();
			d->rule_prog_cells = (uint32_t)(prog.size() / 2);
			rc = upload(&d->d_rule_ent, ent.data(), ent.size(), &d->device_bytes);
			if (rc == ACM_OK) rc = upload(&d->d_rule_slot, slot.data(), slot.size(), &d->device_bytes);
			if (rc == ACM_OK) rc = upload(&d->d_rule_tab, tab.data(), tab.size(), &d->device_bytes);
			if (rc == ACM_OK) rc = upload(&d->d_rule_prog, prog.data(), prog.size(), &d->device_bytes);
		}
		// an automaton with wildcard contexts (acm_automaton_wildcards): per pattern where its context cells lie,
		// the cells, and the interned sets as words (wildcard.hip).  Allocations of their own, as above.
		d->wild = acm_automaton_wildcards(a) != 0;
		if (rc == ACM_OK && d->wild) {
			std::vector<int32_t> ent(4 * a->patterns.size());
			std::vector<uint16_t> pool;
			for (size_t i = 0; i < a->patterns.size(); i++) {
				const acm_automaton::Pattern &p = a->patterns[i];
				ent[4 * i] = (int32_t)pool.size();
				ent[4 * i + 1] = p.wild_pre;
				ent[4 * i + 2] = p.wild_post;
				ent[4 * i + 3] = (int32_t)p.bytes.size();
				pool.insert(pool.end(), p.wild_cells.begin(), p.wild_cells.end());
				if (pool.size() & 1)
					pool.push_back(0);
			}
			pool.resize(pool.size() + 2, 0);
			std::vector<uint32_t> sets(8 * std::max<size_t>(a->wild_classes.size(), 1), 0);
			for (size_t c = 0; c < a->wild_classes.size(); c++)
				for (int k = 0; k < 32; k++)
					sets[8 * c + k / 4] |= (uint32_t)a->wild_classes[c][k] << (8 * (k % 4));
			d->wild_classes = (uint32_t)a->wild_classes.size();
			rc = upload(&d->d_wild_ent, ent.data(), ent.size(), &d->device_bytes);
			if (rc == ACM_OK) rc = upload(&d->d_wild_pool, pool.data(), pool.size(), &d->device_bytes);
			if (rc == ACM_OK) rc = upload(&d->d_wild_sets, sets.data(), sets.size(), &d->device_bytes);
		}
		// an automaton with groups (acm_automaton_groups): per pattern its groups, per group where it lies in
		// the span and its strings, each padded with zeros to whole words (wildcard.hip).  Allocations of their
		// own, as above.
		d->groups = acm_automaton_groups(a) != 0;
		if (rc == ACM_OK && d->groups) {
			std::vector<int32_t> ent(2 * a->patterns.size()), grp;
			std::vector<uint32_t> pool;
			for (size_t i = 0; i < a->patterns.size(); i++) {
				const acm_automaton::Pattern &p = a->patterns[i];
				ent[2 * i] = (int32_t)(grp.size() / 4);
				ent[2 * i + 1] = (int32_t)p.wild_groups.size();
				for (const auto &g : p.wild_groups) {
					const size_t count = g.bytes.size() / (size_t)g.width, words = ((size_t)g.width + 3) / 4;
					grp.insert(grp.end(), { g.at, g.width, (int32_t)((uint32_t)count | (g.negated ? 0x80000000u : 0u)),
					                          (int32_t)pool.size() });
					for (size_t c = 0; c < count; c++) {
						pool.resize(pool.size() + words, 0);
						memcpy(&pool[pool.size() - words], &g.bytes[c * (size_t)g.width], (size_t)g.width);
					}
				}
			}
			rc = upload(&d->d_grp_ent, ent.data(), ent.size(), &d->device_bytes);
			if (rc == ACM_OK) rc = upload(&d->d_grp, grp.data(), grp.size(), &d->device_bytes);
			if (rc == ACM_OK) rc = upload(&d->d_grp_pool, pool.data(), pool.size(), &d->device_bytes);
		}
		// an automaton with replacements (acm_automaton_has_replacements): per pattern what a match becomes, and
		// the replacements' bytes in one blob (rewrite.hip).  Allocations of their own, as above.
		d->replacements = acm_automaton_has_replacements(a) != 0;
		if (rc == ACM_OK && d->replacements) {
			std::vector<int32_t> ent(4 * a->patterns.size());
			std::vector<uint8_t> blob;
			for (size_t i = 0; i < a->patterns.size(); i++) {
				const acm_automaton::Pattern &p = a->patterns[i];
				ent[4 * i] = p.repl_kind;
				ent[4 * i + 1] = p.repl_kind == acm::kReplBytes ? (int32_t)p.repl.size() : 0;
				ent[4 * i + 2] = (int32_t)blob.size();
				ent[4 * i + 3] = p.repl_kind == acm::kReplFill ? (int32_t)p.repl[0] : 0;
				if (p.repl_kind == acm::kReplBytes)
					blob.insert(blob.end(), p.repl.begin(), p.repl.end());
			}
			rc = upload(&d->d_repl_ent, ent.data(), ent.size(), &d->device_bytes);
			if (rc == ACM_OK) rc = upload(&d->d_repl_blob, blob.data(), blob.size(), &d->device_bytes);
		}
		// an automaton with approximate patterns (acm_automaton_add_approx): per pattern whether it is a piece,
		// and then of what; the whole patterns' bytes, folded where the compare folds (approx.hip).  Where piece i
		// begins follows from n and k.  Allocations of their own, as above.
		d->approx = !a->approx.empty();
		if (rc == ACM_OK && d->approx) {
			std::vector<int32_t> ent(4 * a->patterns.size(), 0);
			std::vector<uint32_t> pool, where(a->approx.size());
			for (size_t x = 0; x < a->approx.size(); x++) {
				const acm_automaton::Approx &q = a->approx[x];
				std::vector<unsigned char> b = q.bytes;
				if ((q.flags & ACM_PATTERN_NOCASE) || a->want_nocase)
					for (unsigned char &c : b)
						c = (unsigned char)acm::fold_byte(c);
				where[x] = (uint32_t)pool.size();
				pool.resize(pool.size() + (b.size() + 3) / 4, 0);
				memcpy(&pool[where[x]], b.data(), b.size());
			}
			pool.push_back(0);   // the word behind the last pattern: the compare loads one word ahead
			for (size_t i = 0; i < a->patterns.size(); i++) {
				const acm_automaton::Pattern &p = a->patterns[i];
				ent[4 * i] = -1;
				if (p.approx >= 0) {
					const acm_automaton::Approx &q = a->approx[p.approx];
					const bool folds = (q.flags & ACM_PATTERN_NOCASE) || a->want_nocase;
					ent[4 * i] = (int32_t)where[p.approx];
					ent[4 * i + 1] = q.n;
					ent[4 * i + 2] = q.k | p.approx_piece << 8 | (folds ? 1 << 16 : 0);
					ent[4 * i + 3] = q.mode;
					d->edit = d->edit || q.mode != 0;
				}
			}
			rc = upload(&d->d_approx_ent, ent.data(), ent.size(), &d->device_bytes);
			if (rc == ACM_OK) rc = upload(&d->d_approx_pool, pool.data(), pool.size(), &d->device_bytes);
		}
	} catch (const std::bad_alloc &) {
		rc = acm::fail(ACM_ERR_NOMEM, "acm_dfa_upload: out of host memory");
	}
	if (rc != ACM_OK) {
		acm_dfa_release(d);
		return rc;
	}
	if (acm::scan_prepare(d) != ACM_OK || (d->sparse_ok && acm::sparse_prepare(d) != ACM_OK)) {
		acm_dfa_release(d);
		return ACM_ERR_HIP;
	}
	if (d->sparse_ok && hipHostMalloc((void **)&d->h_giveups, 64, hipHostMallocMapped) == hipSuccess) {
		memset(d->h_giveups, 0, 64);
		if (hipHostGetDevicePointer((void **)&d->d_giveups, d->h_giveups, 0) != hipSuccess)
			d->d_giveups = nullptr;
	}
	if (!d->d_giveups && d->h_giveups) {   // no adaptive mode without the counter
		hipHostFree(d->h_giveups);
		d->h_giveups = nullptr;
	}
	(void)hipGetLastError();
	if (const char *m = getenv("ACM_SCAN_MODE")) {   // debugging aid: same as acm_scan_set_mode
		if (!strcmp(m, "chain")) d->scan_mode = ACM_SCAN_MODE_CHAIN;
		else if (!strcmp(m, "sparse")) d->scan_mode = ACM_SCAN_MODE_SPARSE;
	}
	if (const char *h = getenv("ACM_SCAN_HALO"))   // debugging aid: 0 = always speculate and resolve
		d->use_halo = atoi(h) != 0;
	if (getenv("ACM_SCAN_NO_PRELOAD"))               // debugging aid: halo mode without the up-front text loads
		d->use_preload = false;
	if (const char *g = getenv("ACM_SCAN_GRAPHS"))
		d->use_graphs = atoi(g) != 0;
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) == hipSuccess)
		d->num_cus = prop.multiProcessorCount;
	*out = d;
	return ACM_OK;
}

extern "C" void acm_dfa_release(acm_dfa *d)
{
	if (!d)
		return;
	if (hipSetDevice(d->device) == hipSuccess) {
		hipFree(d->d_cold);
		hipFree(d->d_deep);
		hipFree(d->d_hot);
		free_small(d, d->d_out);
		free_small(d, d->d_dev2ref);
		free_small(d, d->d_in_byte);
		free_small(d, d->d_ref2dev);
		hipFree(d->d_list_begin);
		hipFree(d->d_list_len);
		hipFree(d->d_list_pool);
		free_small(d, d->d_fail_depth);
		free_small(d, d->d_pat_len);
		hipFree(d->d_case_ent);
		hipFree(d->d_case_pool);
		hipFree(d->d_pos_ent);
		hipFree(d->d_seq_ent);
		hipFree(d->d_seq_slot);
		hipFree(d->d_rule_ent);
		hipFree(d->d_rule_slot);
		hipFree(d->d_rule_tab);
		hipFree(d->d_rule_prog);
		hipFree(d->d_wild_ent);
		hipFree(d->d_wild_pool);
		hipFree(d->d_wild_sets);
		hipFree(d->d_grp_ent);
		hipFree(d->d_grp);
		hipFree(d->d_grp_pool);
		hipFree(d->d_repl_ent);
		hipFree(d->d_repl_blob);
		hipFree(d->d_approx_ent);
		hipFree(d->d_approx_pool);
		free_small(d, d->d_depth);
		free_small(d, d->d_class);
		free_small(d, d->d_sv_bloom);
		free_small(d, d->d_sv_gram);
		free_small(d, d->d_sv_prefix);
		free_small(d, d->d_sv_rec);
		free_small(d, d->d_sv_edges);
		hipFree(d->arena);
		acm::lds_walk_release(d);
		if (d->h_giveups)
			hipHostFree(d->h_giveups);
		(void)hipDeviceSynchronize();   // no exec is destroyed under a launch
		for (auto &g : d->graphs)
			if (g.exec)
				hipGraphExecDestroy((hipGraphExec_t)g.exec);
		for (void *e : d->parked_graphs)
			hipGraphExecDestroy((hipGraphExec_t)e);
		for (void *e : d->profile_events)
			hipEventDestroy((hipEvent_t)e);
		for (void *e : d->profile_pool)
			hipEventDestroy((hipEvent_t)e);
	}
	delete d;
}

extern "C" size_t acm_dfa_device_bytes(const acm_dfa *d) { return d ? d->device_bytes : 0; }
extern "C" int acm_dfa_hot_rows(const acm_dfa *d) { return d ? (int)d->hot_rows : 0; }
extern "C" int acm_dfa_device(const acm_dfa *d) { return d ? d->device : -1; }
