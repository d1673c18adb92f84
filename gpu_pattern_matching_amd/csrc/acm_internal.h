// Internal declarations shared by the translation units of libacmatch.so.
// Nothing here is part of the ABI (see include/acmatch.h for that).
#pragma once

#include <array>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "acmatch.h"

namespace acm {

// ---- error plumbing -------------------------------------------------------
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void clear_error();

#define ACM_HIP_TRY(expr)                                                      \
	do {                                                                   \
		hipError_t e_ = (expr);                                        \
		if (e_ != hipSuccess)                                          \
			return acm::fail(ACM_ERR_HIP, "%s: %s (%s:%d)", #expr, \
			    hipGetErrorString(e_), __FILE__, __LINE__);        \
	} while (0)

// ---- design limits --------------------------------------------------------
constexpr uint32_t kMaxStates = 1u << 24;     // state id packed in 24 bits of a staged record
constexpr int kMaxPatternLine = 4096;         // utils.h:14 MAX_PAT_SIZE
constexpr uint32_t kHotRowsMax = 256;         // rows of 256 cells staged in LDS (256 * 512 B = 128 KiB); more with byte classes
constexpr uint32_t kHotBytes = kHotRowsMax * 512;
constexpr uint32_t kHotSentinel = 0xFFFFu;    // hot cell value meaning "look in the cold plane"
constexpr uint32_t kNoPattern = 0xFFFFFFFFu;

// the postfix program of a rule (acm_automaton_add_rule; run by rule.hip): {op, argument} pairs.  A program of
// nesting d needs a stack of d + 2 entries: binary operators, left to right.
enum RuleOp : int32_t {
	kRulePush = 0,   // push operand `argument`: its count, and count > 0
	kRuleAnd = 1,    // pop b, a; push {a.count + b.count, a.truth && b.truth}
	kRuleOr = 2,     //                                  ... a.truth || b.truth
	kRuleEq = 3,     // the top's truth becomes count == argument
	kRuleGt = 4,     //                         count > argument
	kRuleLt = 5,     //                         count < argument
};
constexpr int kRuleStack = ACM_RULE_MAX_NESTING + 2;

// a pattern's replacement (acm_automaton_set_replacement), host and acm_dfa::d_repl_ent
enum ReplKind : int {
	kReplNone = 0,    // the span is copied as it is
	kReplBytes = 1,   // the span becomes the replacement's bytes
	kReplFill = 2,    // every byte of the span becomes the fill byte
};

}  // namespace acm

// Host automaton.  States carry two numberings:
//   ref id : the reference's creation order (acsmx.c:339-344), used at the
//            API boundary (last_state, acsm_get_states, table export)
//   dev id : [0, hot_count)        the first non-final states in BFS order
//                                  (root, depth 1, ...): the rows the walk
//                                  kernel keeps in LDS;
//            [hot_count, first_final)  every other non-final state, in ref
//                                  order -- states created by one pattern
//                                  insertion are consecutive, so a unary trie
//                                  path is a run of consecutive dev ids;
//            [first_final, n)      final states, in ref order.
//            "final" == id >= first_final.  Root is dev id 0.
struct acm_automaton {
	struct Pattern {
		std::vector<unsigned char> bytes;
		int iid;
		unsigned flags = 0;                    // ACM_PATTERN_* as added (acm_automaton_add_ex)
		// where in its text the pattern may start (acm_automaton_set_position); the default is no constraint.
		// compile never reads these: acm_dfa_upload copies them for the position pass (position.hip)
		int32_t pos_lo = 0, pos_hi = INT32_MAX;
		unsigned pos_flags = 0;
		bool positioned() const { return pos_lo != 0 || pos_hi != INT32_MAX || pos_flags != 0; }
		// the sequence this pattern is a part of (acm_automaton_add_sequence) and its level there, or -1
		int32_t seq = -1, seq_level = 0;
		// a wildcard pattern (acm_automaton_add_wildcard): bytes is its anchor, and the positions in front of
		// and behind the anchor are its context: wild_sets holds their pre + post sets of 32 bytes, wild_cells
		// one cell each (an exact byte, or 0x100 | index into acm_automaton::wild_classes).  compile never
		// reads these: acm_dfa_upload copies them for the wildcard pass (wildcard.hip)
		int32_t wild_pre = 0, wild_post = 0;
		std::vector<uint8_t> wild_sets;
		std::vector<uint16_t> wild_cells;
		// its groups (acm_automaton_add_wildcard_groups), ascending: at counts from the pattern's first position,
		// bytes holds the distinct strings of width bytes each.  Covered positions carry the full set above
		struct Group {
			int32_t at, width, negated;
			std::vector<uint8_t> bytes;
		};
		std::vector<Group> wild_groups;
		// what a match of this pattern becomes in a rewrite (acm_automaton_set_replacement); the default is none:
		// the span is copied.  compile never reads these: acm_dfa_upload copies them for the rewrite pass
		// (rewrite.hip)
		int repl_kind = acm::kReplNone;
		std::vector<unsigned char> repl;       // kReplBytes: the bytes (none: delete); kReplFill: the one fill byte
		// a piece of an approximate pattern (acm_automaton_add_approx): which one in acm_automaton::approx, and
		// which of its k + 1 pieces; -1: a pattern of its own
		int32_t approx = -1, approx_piece = 0;
	};
	// approximate patterns (acm_automaton_add_approx): the whole pattern as added; its pieces are the patterns
	// [first_piece, first_piece + k].  compile never reads these: acm_dfa_upload copies them for the approx pass
	// (approx.hip)
	struct Approx {
		int first_piece, n, k, iid;
		unsigned flags;
		std::vector<unsigned char> bytes;
		int mode = 0;   // 0: Hamming distance (add_approx), 1: edit distance (add_edit, edit.hip)
	};
	std::vector<Approx> approx;
	// the distinct context sets of two or more bytes, interned: at most 256
	std::vector<std::array<uint8_t, 32>> wild_classes;
	// ordered multi-part signatures (acm_automaton_add_sequence).  compile never reads these:
	// acm_dfa_upload copies them for the sequence pass (sequence.hip)
	struct Sequence {
		int iid;
		std::vector<int32_t> parts, gap_lo, gap_hi;   // gaps: parts.size() - 1 cells, gap j - 1 in front of part j
		int32_t rule = -1, rule_op = 0;               // the rule this sequence is an operand of (acm_automaton_add_rule), or -1
	};
	std::vector<Sequence> sequences;
	// conditions over the sequences that hit one text (acm_automaton_add_rule).  compile never reads these:
	// acm_dfa_upload copies them for the rule pass (rule.hip)
	struct Rule {
		int iid;
		std::vector<int32_t> sequences;   // the operands
		std::string expr;                 // as given
		std::vector<int32_t> code;        // the postfix program: {op, argument} pairs (acm::RuleOp)
	};
	std::vector<Rule> rules;
	std::vector<Pattern> patterns;         // bytes folded by compile when nocase: every table is built from these
	int max_pattern_len = 0;
	bool compiled = false;
	// acm_automaton_set_nocase: patterns and text compared ASCII case-insensitively (case_fold.h).
	// compile folds the pattern bytes and keeps the originals for acm_automaton_pattern; the column
	// of every lowercase letter repeats its uppercase letter's (byte classes, dense rows), so a walk
	// over raw text is case-folded by its table lookups alone.
	//
	// nocase is the INTERNAL switch: "the tables are built from folded patterns and the kernels fold the
	// text".  compile derives it from what the caller asked for: want_nocase (acm_automaton_set_nocase), or
	// per-pattern ACM_PATTERN_NOCASE flags.  All patterns of length >= 1 flagged: the nocase automaton.
	// Some flagged, some not: a MIXED automaton, built exactly as the nocase automaton of the same patterns
	// (nocase on, mixed on); its scans report candidates and the case pass (case.hip) keeps the unflagged
	// (exact) patterns only where the text equals `original`.  The public getter acm_automaton_nocase is
	// nocase && !mixed.
	bool nocase = false;
	bool want_nocase = false;              // acm_automaton_set_nocase, as asked
	bool mixed = false;                    // compiled, some patterns ignore case and some do not
	std::vector<std::vector<unsigned char>> original;   // [pattern] bytes as added (nocase only)

	uint32_t num_states = 0;               // highest ref id + 1
	std::vector<uint32_t> parent;          // [ref]
	std::vector<uint8_t> in_byte;          // [ref] byte on the edge from parent
	std::vector<uint16_t> depth;           // [ref]
	std::vector<uint32_t> fail;            // [ref] -> ref
	std::vector<uint32_t> child_begin;     // [ref+1] CSR into child_list
	struct Edge {
		uint8_t byte;
		uint32_t to;
	};
	std::vector<Edge> child_list;          // children sorted by byte
	std::vector<uint32_t> bfs_order;       // ref ids in BFS order (byte order per node)

	// match lists (pattern indices, head first) for states that have one
	std::vector<int32_t> list_begin;       // [ref] offset into list_pool or -1
	std::vector<int32_t> list_len;         // [ref]
	std::vector<int32_t> list_pool;

	// Byte classes: bytes that occur in no pattern all lead to the root from every state, so
	// they share one column of the DFA (class 0); every other byte has a class of its own.  A
	// set over a small alphabet (26 letters -> 27 classes) has rows of 32 cells instead of 256:
	// eight times as many states fit the LDS rows, and the planes of the chain pipeline shrink
	// to L2 size.  log_stride = 8: no compression (every byte its own class, identity map).
	uint8_t byte_class[256];
	uint8_t class_byte[256];               // a byte of each class
	uint32_t num_classes = 256, log_stride = 8;

	std::vector<uint32_t> ref2dev, dev2ref;
	uint32_t hot_count = 0;                // dev ids below this are the LDS rows
	uint32_t hot_depth1 = 1;               // hot dev ids below this have depth <= 1
	uint32_t first_final = 0;              // dev ids >= this are final
	std::vector<int32_t> next_chained;     // [pattern] acsm_get_patterns_table chain
	// dev_run[d]: how many steps d -> d+1 -> ... follow the trie: d+1 is the
	// ONLY child of d and is not final.  Along such a run the walk only has
	// to compare text with in_byte of the states ahead -- 16 bytes per load.
	std::vector<uint16_t> dev_run;         // [dev]

	// dense DFA, dev numbering, [num_states][256] cells; built on first use.
	// cell = target dev id | depth(target) << 32 | dev_run[target] << 48
	mutable std::vector<uint64_t> dense;
	const std::vector<uint64_t> &dense_rows() const;
	void drop_dense() const { std::vector<uint64_t>().swap(dense); }

	int head_of(uint32_t ref) const
	{
		return list_begin[ref] < 0 ? -1 : list_pool[list_begin[ref]];
	}
	bool is_final_ref(uint32_t ref) const { return ref != 0 && list_begin[ref] >= 0; }
};
