// acm_dfa: the device-resident automaton (layout described in device_dfa.hip).
#pragma once

#include <atomic>
#include <cstdint>
#include <mutex>
#include <type_traits>
#include <vector>

#include "acmatch.h"

namespace acm {
constexpr uint32_t kCaseAny = 0xFFFFFFFFu, kCaseNever = 0xFFFFFFFEu;   // acm_dfa::d_case_ent
}

struct acm_dfa {
	int device = 0;
	int num_cus = 256;
	uint32_t num_states = 0;
	uint32_t first_final = 0;
	uint32_t hot_rows = 0;
	uint32_t hot_depth1 = 1;             // hot ids below this have depth <= 1
	uint32_t max_pattern_len = 0;
	bool nocase = false;                 // acm_automaton_set_nocase: the kernels that compare text with pattern bytes, or hash it, fold it (case_fold.h)

	uint32_t log_stride = 8;             // cells per row of the planes below = 1 << log_stride (byte classes; 8: bytes)
	uint8_t *d_class = nullptr;          // [256] byte -> class (the identity when log_stride == 8)
	uint32_t *d_cold = nullptr;          // [states][stride] target id
	uint64_t *d_deep = nullptr;          // [states][stride] target id | depth(target) << 32 | run(target) << 48
	uint16_t *d_hot = nullptr;           // [hot_rows][stride]
	int32_t *d_out = nullptr;            // [states] reported pattern index
	uint32_t *d_dev2ref = nullptr;       // [states]
	uint32_t *d_ref2dev = nullptr;       // [states] the other way: a final state handed over on the device (acm_scan_batch.d_init_plane)
	uint8_t *d_in_byte = nullptr;        // [states + 224] byte on the edge into dev state
	uint16_t *d_depth = nullptr;         // [states] trie depth of each state (carried-state walker of the sparse pipeline)

	// sparse ("sieve") pipeline tables, sieve_tables.h
	uint32_t sv_stride = 0;              // W: one text position in W is sampled
	uint32_t sv_gram_len = 3;            // bytes of a sample the filter looks at: 3, or 6 where every pattern has W + 5 bytes
	uint32_t sv_run_ok[8] = { 0 };       // bit b: D copies of byte b are a trie path
	uint32_t sv_prefix_len = 0;          // D: bytes of a pattern checked exactly before a follower starts
	uint32_t *d_sv_bloom = nullptr;      // [1 << sv_bloom_log_words] Bloom filter over the 3-grams at offsets < W, copied to LDS
	uint32_t sv_bloom_log_words = 0;
	uint32_t *d_sv_gram = nullptr;       // [4 << sv_gram_log_buckets] gram | offset mask << 24, four per bucket
	uint32_t sv_gram_log_buckets = 0, sv_gram_probes = 1;
	uint32_t *d_sv_prefix = nullptr;     // [4 << sv_prefix_log_slots] 16-byte slots: key, run, node
	uint32_t sv_prefix_log_slots = 0, sv_prefix_probes = 1;
	void *d_sv_rec = nullptr;            // [states] node records (acm::SieveRec, 16 bytes)
	void *d_sv_edges = nullptr;          // edges of the nodes with two or more children
	uint32_t *d_list_begin = nullptr;    // [states, reference numbering] offset of the state's match list in d_list_pool
	uint32_t *d_list_len = nullptr;      // [states] its length (0: not final)
	int32_t *d_list_pool = nullptr;      // pattern indices, list order
	uint32_t *d_fail_depth = nullptr;    // [states, reference numbering][2] {fail link, trie depth}: segmented scans (segment.hip)
	uint32_t *d_pat_len = nullptr;       // [patterns] bytes of each pattern: where a list entry starts (word.hip)
	uint32_t num_patterns = 0;
	// a mixed automaton only (acm_automaton_mixed_case), for the case pass (case.hip); null otherwise
	bool mixed = false;
	uint32_t *d_case_ent = nullptr;      // [patterns][2] {word index of the pattern in d_case_pool, or kCaseAny: ignores case, or
	                                     // kCaseNever: length 0; length}: one 8-byte load per list entry
	uint32_t *d_case_pool = nullptr;     // the exact patterns' bytes as added, each padded to whole words, one spare word behind
	// a positioned automaton only (acm_automaton_positioned at upload), for the position pass (position.hip); null otherwise
	bool positioned = false;
	int32_t *d_pos_ent = nullptr;        // [patterns][4] {lo, hi, flags, length}: one 16-byte load per entry
	// an automaton with sequences only (acm_automaton_add_sequence before upload), for the sequence pass
	// (sequence.hip); null otherwise.  A SLOT is a part of a sequence; slots are numbered level-major (every
	// level-0 part, then every level-1 part, ...), so that records ordered by slot lie level by level.
	int32_t *d_seq_ent = nullptr;        // [patterns][4] {slot or -1, lo, hi of the gap in front, length}
	int32_t *d_seq_slot = nullptr;       // [slots][2] {slot of the part in front or -1, sequence index or -1: not the last part}
	uint32_t seq_slots = 0, seq_levels = 0;
	uint32_t seq_level_base[ACM_SEQ_MAX_PARTS + 1] = { 0 };   // slots [base[j], base[j + 1]) are level j
	// an automaton with rules only (acm_automaton_add_rule before upload), for the rule pass (rule.hip); null
	// otherwise.  A SLOT is an operand of a rule; slots are numbered rule-major.
	int32_t *d_rule_ent = nullptr;       // [rule_sequences] slot of the sequence, or -1: no operand
	int32_t *d_rule_slot = nullptr;      // [slots][2] {rule, operand}
	int32_t *d_rule_tab = nullptr;       // [rules][4] {first slot, operands, first cell of the program in d_rule_prog, its cells}
	int32_t *d_rule_prog = nullptr;      // [rule_prog_cells][2] the postfix programs: {acm::RuleOp, argument}
	uint32_t rule_slots = 0, num_rules = 0, rule_sequences = 0, rule_prog_cells = 0;
	// an automaton with wildcard contexts only (acm_automaton_wildcards at upload), for the wildcard pass
	// (wildcard.hip); null otherwise.  The position and sequence tables above then hold the folded lengths.
	bool wild = false;
	int32_t *d_wild_ent = nullptr;       // [patterns][4] {cell index of the context in d_wild_pool, pre, post, length}
	uint16_t *d_wild_pool = nullptr;     // per context position an exact byte, or 0x100 | class; a pattern's cells start on a word
	uint32_t *d_wild_sets = nullptr;     // [wild_classes][8] the interned sets, bit b & 31 of word b / 32
	uint32_t wild_classes = 0;
	size_t device_bytes = 0;
	void *arena = nullptr;               // one allocation for the small tables (device_dfa.hip, upload_small)
	size_t arena_bytes = 0, arena_used = 0;

	// adaptive AUTO mode (dispatch.cpp, pick_sparse): sparse batches that turned out dense in matches,
	// counted by the device in pinned host memory
	uint32_t *h_giveups = nullptr, *d_giveups = nullptr;
	mutable std::atomic<uint32_t> sparse_batches{0}, giveups_seen{0}, chain_hold{0};
	mutable std::atomic<uint32_t> auto_window{16}, auto_next_hold{64};   // batches per look at the counter; chain batches after a bad look

	// the automaton whole in LDS (lds_walk.hip, compact_tables.h): small alphabets, <= 16384 states
	bool lds_ok = false;
	uint8_t *d_lds_image = nullptr;      // what the walk kernel copies to LDS
	int32_t *d_lds_out = nullptr;        // [compact id] reported pattern index
	uint32_t *d_lds_cid2ref = nullptr;   // [compact id] reference id
	uint32_t *d_lds_ref2code = nullptr;  // [reference id] state code (a state handed over on the device)
	uint32_t lds_image_bytes = 0, lds_off_rec = 0, lds_halo = 0, lds_rows = 0, lds_root_code = 0, lds_final_code = 0;
	std::vector<uint16_t> lds_ref2code;  // host: state code of a reference id (init_state)

	bool sparse_ok = false;              // every pattern has >= 3 bytes: the sparse pipeline applies
	int scan_mode = ACM_SCAN_MODE_AUTO;

	std::vector<uint32_t> ref2dev;       // host copy for init_state

	int chain_bytes = 0;                 // 0 = pick automatically
	int chains_per_lane = 4;             // 2 or 4 independent chains per lane in the walk

	// HIP graphs of batches that repeat (dispatch.cpp, acm_scan_batch_async)
	struct GraphKey {
		acm_scan_batch batch;   // stream null (no event fields, not timed: such batches are not captured)
		int mode, chain_bytes, chains_per_lane, zero;
	};
	// Keys are compared with memcmp, so neither struct may have padding; and a field added to acm_scan_batch
	// that does not change what is enqueued has to be cleared in graph_key, or every lookup misses.
	static_assert(std::has_unique_object_representations_v<GraphKey>, "GraphKey must have no padding");
	struct GraphEntry {
		GraphKey key;
		void *exec;          // hipGraphExec_t, null until the key has been seen twice
		uint64_t last_use;
	};
	static constexpr size_t kMaxGraphs = 32;
	bool use_preload = true;             // halo mode: k_halo_walk (text loaded up front) where the chains are short enough
	bool use_halo = true;                // chain pipeline: halo mode where the longest pattern fits a chain (scan.hip)
	int max_group = 16;                   // batches acm_scan_batches_async puts into one set of sparse launches
	mutable bool use_graphs = false;     // opt-in: measured neutral on this stack
	mutable std::vector<GraphEntry> graphs;
	mutable std::vector<void *> parked_graphs;   // evicted execs, destroyed by acm_dfa_release
	mutable std::mutex graph_mutex;
	mutable uint64_t graph_tick = 0;
	mutable std::atomic<uint64_t> graphs_captured{0}, graphs_launched{0};   // acm_scan_graph_stats: instantiated, hipGraphLaunch calls

	// optional in-line timing (acm_scan_profile_*): event quadruples
	// {before the first kernel, after the first stage, after the second, after the last kernel} per recorded launch
	mutable bool profile = false;
	mutable std::vector<void *> profile_events;
	mutable std::vector<void *> profile_pool;   // idle events, reused
	mutable std::mutex profile_mutex;

	// an automaton with groups only (acm_automaton_groups at upload; wild is then set too), for the wildcard pass;
	// null otherwise.  Behind everything else: the fields the scan paths touch lie where they lay without these.
	bool groups = false;
	int32_t *d_grp_ent = nullptr;        // [patterns][2] {first group in d_grp, groups}
	int32_t *d_grp = nullptr;            // [groups][4] {first byte counted from the span's, width, count | negated << 31, word index in d_grp_pool}
	uint32_t *d_grp_pool = nullptr;      // the strings, each zero-padded to whole words

	// an automaton with replacements only (acm_automaton_has_replacements at upload), for the rewrite pass
	// (rewrite.hip); null otherwise: every span is then copied as it is
	bool replacements = false;
	int32_t *d_repl_ent = nullptr;       // [patterns][4] {acm::ReplKind, bytes of the replacement, where they begin in d_repl_blob, the fill byte}
	uint8_t *d_repl_blob = nullptr;      // the replacements' bytes, back to back

	// an automaton with approximate patterns only (acm_automaton_num_approx at upload), for the approx pass
	// (approx.hip); null otherwise: every entry is then kept with distance 0
	bool approx = false;
	int32_t *d_approx_ent = nullptr;     // [patterns][4] {word index of the whole pattern in d_approx_pool, or -1: not a piece; n;
	                                     // k | piece << 8 | folds << 16; the mode, 0 Hamming or 1 edit}: one 16-byte load per entry
	uint32_t *d_approx_pool = nullptr;   // the approximate patterns' bytes (folded for one that folds), each padded to whole words, one spare word behind
	bool edit = false;                   // some approximate pattern is an edit pattern (acm_automaton_add_edit): the edit pass (edit.hip) is the one to call
	uint32_t max_list_len = 0;           // the longest match list: the candidates a record can give (edit.hip sizes its workspace by it)
};
