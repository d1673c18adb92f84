/*
 * acmatch.h -- C ABI of libacmatch.so, the MI355X-native (gfx950, HIP)
 * Aho-Corasick matcher.
 *
 * Two layers live in this one header:
 *
 *  (1) acm_*  : the native boundary.  Plain pointers and sizes, explicit
 *               device pointers + stream, integer status codes.  This is
 *               what an FFI (ctypes, cgo, JNI) binds, and what bench.py uses.
 *
 *  (2) the reference's own names (acsm_*, databuf_*, ocl_aho_match*,
 *      ocl_prefix_sum*, ocl_compact_array*, ocl_bitonic_sort*, clinitctx):
 *               same names, arity, argument meaning and error behaviour as
 *               the OpenCL library they replace, so ocl_worker.c /
 *               ocl_aho_grep.c recompile against include/compat/ unchanged.
 *               Each declaration cites the reference interface it replaces.
 *
 * Handle mapping for layer (2):  cl_mem = HIP device pointer,
 * cl_command_queue = hipStream_t, cl_context = opaque per-device context,
 * cl_device_id / cl_platform_id = HIP device ordinal + 1 cast to a pointer.
 */
#ifndef ACMATCH_H_
#define ACMATCH_H_

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ====================================================================== */
/* (1) native boundary                                                    */
/* ====================================================================== */

enum {
	ACM_OK = 0,
	ACM_ERR_ARG = -1,	/* bad argument / misuse                       */
	ACM_ERR_NOMEM = -2,	/* host or device allocation failed            */
	ACM_ERR_HIP = -3,	/* a HIP runtime call failed                   */
	ACM_ERR_NODEV = -4,	/* no usable gfx950 device                     */
	ACM_ERR_LIMIT = -5,	/* automaton / buffer exceeds a design limit   */
	ACM_ERR_IO = -6,	/* pattern file could not be opened            */
	ACM_ERR_PARSE = -7,	/* malformed pattern line                      */
	ACM_ERR_CAPACITY = -8	/* result planes too small for the matches     */
};

/* text of the last error raised on the calling thread ("" if none) */
const char *acm_last_error(void);
const char *acm_strerror(int code);
/* library version / build string, e.g. "acmatch 0.1 gfx950" */
const char *acm_version(void);
/* number of visible HIP devices (0 when there is none, never an error) */
int acm_device_count(void);

/* ---------------------------------------------------------------------- */
/* host-side automaton: pattern list -> acsmx-compatible DFA               */
/* replaces acsm_new/add_pattern/compile/gen_state_table (acsmx.h:96-141)  */
/* ---------------------------------------------------------------------- */
typedef struct acm_automaton acm_automaton;

acm_automaton *acm_automaton_new(void);
void acm_automaton_free(acm_automaton *);

/* append one pattern; its index is the number of patterns added before it
 * (acsmx.c:535).  n may be 0 (an empty pattern never reports). */
int acm_automaton_add(acm_automaton *, const unsigned char *bytes, int n,
    int iid);

/* pattern-file parser of ocl_worker.c:74-145: one pattern per line, optional
 * "ID pattern" categorical form decided on the first line, one pair of
 * surrounding double quotes stripped, hex => printable hex (utils.c:32-54),
 * max_len = -m limit in bytes or -1.  Returns patterns added or an error. */
int acm_automaton_load_file(acm_automaton *, const char *path, int hex,
    int max_len);

/* Case sensitivity per pattern.  acm_automaton_add_ex is acm_automaton_add plus
 * flags (acm_automaton_add is add_ex with flags 0): ACM_PATTERN_NOCASE makes
 * this pattern ignore ASCII case (the fold of acm_automaton_set_nocase below);
 * a pattern without it is exact.  Unknown flag bits are ACM_ERR_ARG.
 * acm_automaton_load_file_ex is the parser above with every pattern of the file
 * added with flags; it may be called after other patterns were added (pattern
 * indices continue).  acm_automaton_pattern_flags returns the flags as added,
 * or ACM_ERR_ARG.  What acm_automaton_compile makes of the flags:
 *   set_nocase(1)             every pattern ignores case, the flags do not
 *                             matter, the automaton is not mixed: as without
 *                             the flags, bit for bit
 *   off, no pattern flagged   nothing changes
 *   off, every pattern of length >= 1 flagged
 *                             the automaton set_nocase(1) gives on the same
 *                             patterns: same tables, self-test digests and
 *                             reference table, acm_automaton_nocase() = 1, not
 *                             mixed
 *   otherwise                 a MIXED automaton.  It is built exactly as the
 *                             nocase automaton of the same patterns (patterns
 *                             folded, lowercase columns alias uppercase ones,
 *                             the bytes as added kept), and every pipeline
 *                             scans it as it scans that automaton.
 *                             acm_automaton_nocase() = 0,
 *                             acm_automaton_mixed_case() = 1 (1 only for a
 *                             compiled automaton in which at least one pattern
 *                             ignores case and one does not, else 0), and
 *                             acm_automaton_pattern returns the bytes as added.
 * The records of ANY scan of a mixed automaton are CANDIDATES: the nocase
 * automaton's records, a superset of the wanted ones (an exact pattern is also
 * reported where the text differs from it in case).  acm_case_matches_async
 * makes them exact. */
enum { ACM_PATTERN_NOCASE = 1 };
int acm_automaton_add_ex(acm_automaton *, const unsigned char *bytes, int n,
    int iid, unsigned flags);
int acm_automaton_load_file_ex(acm_automaton *, const char *path, int hex,
    int max_len, unsigned flags);
int acm_automaton_pattern_flags(const acm_automaton *, int index);
int acm_automaton_mixed_case(const acm_automaton *);

/* Position constraints: where in its text a pattern may match.  Pattern p of length L >= 1 that ends
 * at offset o starts at a = o - L + 1; its text occupies [T0, Tend).  With the window (lo, hi, flags):
 *   flags 0            p is kept iff lo <= a - T0 <= hi    (counted from the start of the text)
 *   ACM_POS_FROM_END   p is kept iff lo <= Tend - a <= hi  (counted back from the end of the text)
 * hi == ACM_POS_UNBOUNDED: no upper bound.  All arithmetic is in int64.  The default (0,
 * ACM_POS_UNBOUNDED, 0) is "no constraint"; any other triple is a constraint, and an automaton with one
 * is POSITIONED (acm_automaton_positioned = 1).  lo > hi is legal and never matches; lo < 0, hi < 0,
 * unknown flag bits or a bad index are ACM_ERR_ARG.  A pattern of length 0 is never kept.
 * acm_automaton_pattern_position returns the window as set (any of the three pointers may be NULL).
 * Windows do not enter acm_automaton_compile: tables, digests, self-tests and acm_dfa_device_bytes of an
 * automaton without constraints are what they were, and no scan looks at a window.  The records of a
 * scan are made to obey them by acm_position_matches_async, which reads a copy that acm_dfa_upload
 * takes: windows may be set before or after acm_automaton_compile, but a window set after
 * acm_dfa_upload does not reach that acm_dfa.
 * How the usual source forms map to windows (no parser for them is provided):
 *   Snort offset, depth     lo = offset, hi = offset + depth - L       flags 0
 *   ^                       (0, 0, 0)
 *   $                       (L, L, ACM_POS_FROM_END)
 *   ClamAV n,ms             (n, n + ms, 0)
 *   ClamAV EOF-n,ms         (n - ms, n, ACM_POS_FROM_END)
 * The reference-named layer is unchanged: acsm_add_pattern keeps ignoring its offset and depth
 * arguments, as the reference's search does.
 * acm_automaton_load_position_file reads one constraint per line, "<pattern index> <lo> <hi or *> [end]"
 * (decimal; * = ACM_POS_UNBOUNDED; end = ACM_POS_FROM_END).  A line whose first non-blank byte is '#' and
 * blank lines are skipped.  A malformed line or an index out of range is ACM_ERR_PARSE and
 * acm_last_error names the line; nothing is applied then.  Returns the number of constraints applied. */
enum { ACM_POS_FROM_END = 1 };
#define ACM_POS_UNBOUNDED INT32_MAX
int acm_automaton_set_position(acm_automaton *, int index, int32_t lo, int32_t hi, unsigned flags);
int acm_automaton_pattern_position(const acm_automaton *, int index, int32_t *lo, int32_t *hi,
    unsigned *flags);
int acm_automaton_positioned(const acm_automaton *);
int acm_automaton_load_position_file(acm_automaton *, const char *path);

/* Replacements: what a match of a pattern becomes in a rewrite (acm_rewrite_async).  The span [s, e] of a
 * match is the select pass's: wildcard contexts included.
 *   flags 0          the whole span becomes bytes[0, n); n == 0 (bytes may then be NULL) deletes it.  n up to
 *                    ACM_REPLACEMENT_MAX_LEN, above it ACM_ERR_LIMIT
 *   ACM_REPL_FILL    n must be 1: every byte of the span becomes bytes[0] and the length is kept (a mask)
 *   none set         the default: the span is copied as it is (the pattern still takes part in the selection);
 *                    acm_automaton_clear_replacement returns to it
 * A bad index, unknown flag bits, n < 0, a NULL bytes with n > 0 or a fill with n != 1 are ACM_ERR_ARG.
 * acm_automaton_pattern_replacement returns 1 if pattern `index` has a replacement, else 0 (negative: a bad
 * index), and the replacement as set: a borrowed pointer, its length and flags (any pointer may be NULL).
 * acm_automaton_has_replacements is 1 if some pattern has one; acm_automaton_max_replacement_len is the length of
 * the longest replacement that is no fill (0 without one): less one, the most bytes a match can add to a rewrite.
 * Replacements do not enter acm_automaton_compile: tables, digests, self-tests and acm_dfa_device_bytes of an
 * automaton without replacements are what they were, and no scan looks at one.  They may be set before or
 * after compile; acm_dfa_upload takes a copy (an entry per pattern and one blob of bytes, only when at least
 * one is set), so one set later does not reach that acm_dfa.
 * acm_automaton_load_replacement_file reads one replacement per line: "<pattern index> <hex bytes or empty>"
 * or "<pattern index> fill <hh>" (decimal index; hex digit pairs without blanks between them).  A line whose
 * first non-blank byte is '#' and blank lines are skipped.  A malformed line or an index out of range is
 * ACM_ERR_PARSE and acm_last_error names the line; nothing is applied then.  Returns the number applied.
 * Not provided: replacements that refer to the matched bytes (case-preserving, back-references). */
enum { ACM_REPL_FILL = 1 };
#define ACM_REPLACEMENT_MAX_LEN 65535
int acm_automaton_set_replacement(acm_automaton *, int index, const unsigned char *bytes, int n,
    unsigned flags);
int acm_automaton_clear_replacement(acm_automaton *, int index);
int acm_automaton_pattern_replacement(const acm_automaton *, int index, const unsigned char **bytes,
    int *n, unsigned *flags);
int acm_automaton_has_replacements(const acm_automaton *);
int acm_automaton_max_replacement_len(const acm_automaton *);
int acm_automaton_load_replacement_file(acm_automaton *, const char *path);

/* Ordered multi-part signatures: the relation BETWEEN patterns.  A SEQUENCE is k parts, 1 <= k <=
 * ACM_SEQ_MAX_PARTS: pattern indices p_0 .. p_{k-1}, k - 1 gaps (lo_j, hi_j), j = 1 .. k-1, and a user id
 * iid.  A gap has lo >= 0 and hi >= 0, or hi == ACM_GAP_UNBOUNDED; lo > hi is legal and never matches (as
 * a position window).
 * An occurrence of pattern p (length L >= 1) that ends at offset e starts at a = e - L + 1 and lies in the
 * text [T0, Tend) its offset belongs to (found as the position pass finds it; Tend is not needed).  A
 * sequence MATCHES ENDING AT o iff there are occurrences of its parts with ends e_0 < ... < e_{k-1} = o
 * such that
 *   a_0 >= T0, and
 *   for j >= 1:  lo_j <= a_j - e_{j-1} - 1 <= hi_j  and  e_{j-1} >= T0 of part j's text.
 * The gap is the number of bytes strictly between two parts, so parts never overlap, and no chain crosses
 * a text start.  Level by level: a level-0 record is ALIVE iff a >= T0; a level-j record is alive iff some
 * alive level-(j-1) record of the same sequence ends in [max(a - 1 - hi, T0), a - 1 - lo] (no lower bound
 * but T0 when hi is unbounded).  All arithmetic is in int64.
 * How the usual source forms map to gaps:
 *   ClamAV {n-m}  (n, m)      {n}  (n, n)      {-m}  (0, m)      {n-}  (n, unbounded)      *  (0, unbounded)
 *   ClamAV ??     (1, 1); adjacent gap tokens add, a sum with an unbounded term is unbounded
 *   Snort distance d          lo = d  (d >= 0)
 *   Snort within w            hi = w - L_j
 * A pattern index may be a part of at most one sequence, at one level; to use the same bytes twice, add
 * the pattern twice (the automaton keeps duplicates and the all-patterns forms report every list entry).
 * A 1-part sequence has no gaps: plain patterns and multi-part signatures come out under one id space.
 * Sequences do not enter acm_automaton_compile: tables, digests, self-tests and acm_dfa_device_bytes of an
 * automaton without sequences are what they were, and no scan looks at a sequence.  They may be added
 * before or after compile; acm_dfa_upload takes a copy, so one added later does not reach that acm_dfa.
 * acm_sequence_matches_async joins the records of a scan on the device.
 *   acm_automaton_add_sequence       returns the sequence index.  gap_lo / gap_hi have nparts - 1 cells
 *                                    (ignored when nparts == 1).  ACM_ERR_ARG: a bad index, a part already
 *                                    used (also twice in this call), a part of length 0, a negative bound,
 *                                    nparts < 1; ACM_ERR_LIMIT above ACM_SEQ_MAX_PARTS.  On an error
 *                                    nothing is applied.
 *   acm_automaton_sequence           sequence i: iid, nparts and borrowed pointers (any may be NULL)
 *   acm_automaton_pattern_sequence   1 and (sequence, level) if the pattern is a part, else 0
 *   acm_automaton_add_signature      parses a ClamAV-style hex body -- hex byte pairs, ??, *, {n}, {n-m},
 *                                    {-m}, {n-} -- adds each fixed part with acm_automaton_add_ex(..., iid,
 *                                    flags) and registers the sequence; returns the sequence index.  The
 *                                    body begins and ends with a fixed part.  Anything else (a nibble
 *                                    wildcard a?, alternatives (..|..), !, an odd hex digit, an empty part,
 *                                    a gap sum of INT32_MAX or more) is ACM_ERR_PARSE and acm_last_error
 *                                    names the column (from 1).  The body is parsed completely before
 *                                    anything is added.  Only before compile: it adds patterns.
 *   acm_automaton_load_signature_file  one signature per line, with an optional leading "<decimal iid>:",
 *                                    otherwise the iid is the sequence index; lines whose first non-blank
 *                                    byte is '#' and blank lines are skipped.  A bad line is ACM_ERR_PARSE
 *                                    naming the line, and nothing of the file is applied.  Returns the
 *                                    number of sequences added.  A pure hex line is a 1-part sequence.
 * Not provided: sequences whose parts lie in different calls (a stream cut inside a signature is not
 * joined: scan whole texts), negative distances or overlapping parts, alternatives of unequal length,
 * where a match begins.  Nibble wildcards and alternatives: the extended syntax below.  The
 * reference-named layer is unchanged. */
#define ACM_SEQ_MAX_PARTS 32
#define ACM_GAP_UNBOUNDED INT32_MAX
int acm_automaton_add_sequence(acm_automaton *, const int32_t *parts, const int32_t *gap_lo,
    const int32_t *gap_hi, int nparts, int iid);
int acm_automaton_num_sequences(const acm_automaton *);
int acm_automaton_sequence(const acm_automaton *, int index, int *iid, int *nparts,
    const int32_t **parts, const int32_t **gap_lo, const int32_t **gap_hi);
int acm_automaton_pattern_sequence(const acm_automaton *, int pattern, int *sequence, int *level);
int acm_automaton_add_signature(acm_automaton *, const char *body, int iid, unsigned flags);
int acm_automaton_load_signature_file(acm_automaton *, const char *path, unsigned flags);

/* Wildcard patterns: literal + confirm.  A WILDCARD PATTERN is n positions, 1 <= n <=
 * ACM_WILDCARD_MAX_POSITIONS, each a set of byte values: 32 bytes, bit b & 7 of byte b / 8 set = byte b is
 * in the set (the layout of acm_word_matches_async's word_set).  It matches where every position holds a
 * byte of its set.
 * The ANCHOR is the longest run of positions whose set holds exactly one byte, the leftmost among equal
 * runs.  Only its L bytes enter the automaton, added with acm_automaton_add_ex(..., iid, flags);
 * acm_automaton_add_wildcard returns that pattern's index.  The pre positions in front of the anchor are the
 * pattern's PRE context, the post positions behind it its POST context; acm_wildcard_matches_async checks
 * them where the anchor matched.  ACM_PATTERN_NOCASE applies to the anchor only: context sets are compared
 * with raw text bytes (a case-blind context position is the set {A, a}).  A pattern whose positions are all
 * one-byte sets is a plain pattern (pre = post = 0), and an automaton without any context is bit for bit
 * what it is without this interface: tables, digests, self-tests and acm_dfa_device_bytes.
 * Context sets of two or more bytes are interned per automaton: at most 256 distinct ones (a one-byte set in
 * a context does not count).  Contexts do not enter acm_automaton_compile; acm_dfa_upload takes a copy.
 *   acm_automaton_add_wildcard      ACM_ERR_ARG: no position with a one-byte set, an empty set, n < 1, unknown
 *                                   flags, a compiled automaton (it adds a pattern); ACM_ERR_LIMIT: n above
 *                                   the maximum, or a 257th distinct set.  On an error nothing is applied.
 *   acm_automaton_pattern_wildcard  1 if pattern `index` has a context, else 0 (negative: a bad index); pre and
 *                                   post, and borrowed pointers to their pre * 32 and post * 32 bytes of sets
 *                                   (any pointer may be NULL)
 *   acm_automaton_wildcards         1 if some pattern has a context
 *   acm_automaton_wildcard_reach    over the patterns that have a context: back = the largest pre + L (bytes
 *                                   from a pattern's first position to its anchor's end), ahead = the largest
 *                                   post.  What a streaming caller keeps of the piece in front, and how far
 *                                   behind an anchor a match can end.  Both 0 without contexts.
 * How the other per-pattern rules see a wildcard pattern (folded into their tables at upload):
 *   position windows   count from the pattern's FIRST POSITION (a = o - L - pre + 1), for both window kinds
 *   sequences          gaps count between the parts' full spans: from the last position of the part in front
 *                      to the first position of this part.  Exact for records that went through
 *                      acm_wildcard_matches_async with the same starts.  The sequence pass keeps reporting
 *                      the end of the last part's ANCHOR; the match ends post bytes behind it (the caller
 *                      adds that after the fetch: acm_automaton_pattern_wildcard of the last part)
 *   whole words        NOT composed: the word pass looks at the bytes next to the anchor
 * Extended body syntax: acm_automaton_add_signature_ex and acm_automaton_load_signature_file_ex are the two
 * entry points above with a syntax argument.  syntax 0 is exactly those (a?, (..|..) and ! stay
 * ACM_ERR_PARSE); unknown syntax bits are ACM_ERR_ARG.  With ACM_SIG_EXTENDED a body is POSITIONS and gaps:
 *   HH            an exact byte                H? or ?H      the 16 bytes with that nibble
 *   ??            any byte (a position here, not a gap of one)
 *   (HH|HH|...)   the listed bytes (one entry: an exact byte)        !(HH|...)   every other byte
 * and only * and {...} separate parts.  Every part needs an exact byte and is added with
 * acm_automaton_add_wildcard.  The body begins and ends with a position that is not ??.  Alternatives of more
 * than one byte ((aabb|ccdd): without ACM_SIG_GROUPS, below), a ! that no ( follows, a part of more than
 * ACM_WILDCARD_MAX_POSITIONS positions and everything syntax 0 rejects in gap tokens are ACM_ERR_PARSE with
 * the column (a part without an exact byte: the column it begins at).  A body is parsed completely, and the room for its sets checked,
 * before anything is added; a bad line (or a file that needs a 257th set: ACM_ERR_LIMIT) leaves nothing of
 * its file applied.  For a body that holds neither ?? nor a new token both syntaxes add the same patterns
 * and sequence.
 * Groups: alternatives of more than one byte.  A wildcard pattern may carry up to ACM_PATTERN_MAX_GROUPS
 * GROUPS.  A group is a first position `at` (counted from the pattern's first position), a width w,
 * 2 <= w <= ACM_GROUP_MAX_WIDTH, `count` strings of exactly w bytes each, 1 <= count <=
 * ACM_GROUP_MAX_ALTERNATIVES (bytes: count * width bytes, string after string), and a negated flag (0 or 1).
 * It HOLDS at an occurrence iff the w text bytes under the positions [at, at + w) equal one of the strings
 * (negated: equal none of them).  Groups are ascending and disjoint and lie inside [0, n), and every position
 * a group covers carries the full set (??): the anchor stays a function of the sets alone, a covered position
 * is never part of it, and a pattern with a group always has a context.  The pattern matches where every
 * position holds a byte of its set AND every group holds.  Groups compare raw text bytes (ACM_PATTERN_NOCASE
 * applies to the anchor alone).  The span keeps its fixed length, so position windows and sequence gaps see a
 * pattern with groups exactly as above.  Groups do not enter acm_automaton_compile, and an automaton without
 * any is bit for bit what it is without this interface.
 *   acm_automaton_add_wildcard_groups  acm_automaton_add_wildcard with groups; ngroups == 0 is exactly that
 *                                   call.  Beside its errors, ACM_ERR_ARG: ngroups < 0, a null pointer, a width
 *                                   below 2, count < 1, a flag that is not 0 or 1, a group that leaves [0, n),
 *                                   overlaps the one in front or is not ascending, a covered position whose
 *                                   set is not full; ACM_ERR_LIMIT: more groups, a larger width or more
 *                                   distinct strings than the maxima.  Equal strings of a group are kept once
 *                                   (the first of them).  On an error nothing is applied.
 *   acm_automaton_pattern_groups    the number of groups of pattern `index` (negative: a bad index)
 *   acm_automaton_pattern_group     group j of pattern `index`: at, width, the count of distinct strings, negated
 *                                   and a borrowed pointer to count * width bytes (any pointer may be NULL)
 *   acm_automaton_groups            1 if some pattern has a group
 * ACM_SIG_GROUPS is a second syntax bit, legal only together with ACM_SIG_EXTENDED (alone: ACM_ERR_ARG);
 * ACM_SIG_EXTENDED alone is exactly what it was.  With both, inside (..) and !(..) every alternative is one
 * or more hex byte pairs:
 *   (HHHH|HHHH|...)   one of the listed strings               !(HHHH|...)   none of them
 * All alternatives of one group have the width of the first: another width is ACM_ERR_PARSE at the column
 * where that alternative begins.  A width above ACM_GROUP_MAX_WIDTH, more than ACM_GROUP_MAX_ALTERNATIVES
 * distinct alternatives, or a group beyond ACM_PATTERN_MAX_GROUPS in one part is ACM_ERR_PARSE naming the
 * column of the ( or !.  Alternatives of one byte are a set position as without the bit; a group that is not
 * negated and lists one distinct string is that many exact positions (and may be the anchor); nothing is
 * factored out of the alternatives.  A group may begin or end a body (its positions are not the ?? that
 * may not), and "every part needs an exact byte" stands.  The parts are added with
 * acm_automaton_add_wildcard_groups; a refused body, line or file applies nothing.
 * Not provided: alternatives of unequal length ((aa|bbcc)): the span of a pattern has one length, which is
 * what lets the position and sequence rules fold it into their tables. */
#define ACM_WILDCARD_MAX_POSITIONS 4096
#define ACM_GROUP_MAX_WIDTH 32
#define ACM_GROUP_MAX_ALTERNATIVES 256
#define ACM_PATTERN_MAX_GROUPS 16
enum { ACM_SIG_EXTENDED = 1, ACM_SIG_GROUPS = 2 };
typedef struct acm_wild_group {
	int32_t at, width, count, negated;
	const uint8_t *bytes;   /* count * width bytes */
} acm_wild_group;
int acm_automaton_add_wildcard(acm_automaton *, const uint8_t *sets, int n, int iid, unsigned flags);
int acm_automaton_pattern_wildcard(const acm_automaton *, int index, int *pre, int *post,
    const uint8_t **pre_sets, const uint8_t **post_sets);
int acm_automaton_wildcards(const acm_automaton *);
int acm_automaton_wildcard_reach(const acm_automaton *, int *back, int *ahead);
int acm_automaton_add_wildcard_groups(acm_automaton *, const uint8_t *sets, int n, const acm_wild_group *groups,
    int ngroups, int iid, unsigned flags);
int acm_automaton_pattern_groups(const acm_automaton *, int index);
int acm_automaton_pattern_group(const acm_automaton *, int index, int j, int *at, int *width, int *count,
    int *negated, const uint8_t **bytes);
int acm_automaton_groups(const acm_automaton *);
int acm_automaton_add_signature_ex(acm_automaton *, const char *body, int iid, unsigned flags,
    unsigned syntax);
int acm_automaton_load_signature_file_ex(acm_automaton *, const char *path, unsigned flags,
    unsigned syntax);

/* Approximate patterns: up to k substituted bytes (Hamming distance).  An APPROXIMATE PATTERN is n bytes and a
 * budget k, 0 <= k <= ACM_APPROX_MAX_K and k + 1 <= n <= ACM_APPROX_MAX_LEN.  It matches a span of n text bytes
 * that differs from it in at most k positions.  It is cut into k + 1 PIECES that tile it: with q = n / (k + 1)
 * and r = n % (k + 1), piece i (0 <= i <= k) covers the pattern bytes [b_i, e_i), b_i = i * q + min(i, r) and
 * e_i = b_{i + 1}: the first r pieces are one byte longer.  A span within the budget holds at least one piece
 * exactly, so only the pieces enter the automaton, as k + 1 consecutive patterns added with
 * acm_automaton_add_ex(..., iid, flags); acm_approx_matches_async counts the mismatches where a piece matched.
 * ACM_PATTERN_NOCASE is the only flag and makes the whole comparison fold ASCII case (a..z only: '@' and '`',
 * '[' and '{' stay different bytes), as does acm_automaton_set_nocase for every pattern.  Approximate
 * patterns do not enter acm_automaton_compile; acm_dfa_upload takes a copy.  An automaton without any is bit
 * for bit what it is without this interface: tables, digests, self-tests and acm_dfa_device_bytes.
 *   acm_automaton_add_approx      the index of piece 0 (>= 0), or an error (< 0).  With k == 0 it is exactly
 *                                 acm_automaton_add_ex (any n that call takes; no approximate pattern is
 *                                 recorded) and returns the new pattern's index.  ACM_ERR_ARG: a null pointer,
 *                                 k < 0, n < k + 1, unknown flags, a compiled automaton; ACM_ERR_LIMIT: k or n
 *                                 above the maxima.  On an error nothing is applied.
 *   acm_automaton_num_approx      the number of approximate patterns (k >= 1)
 *   acm_automaton_approx          approximate pattern x: the index of its piece 0, n, k, iid, flags and a borrowed
 *                                 pointer to its n bytes as added (any pointer may be NULL)
 *   acm_automaton_pattern_approx  1 if pattern `index` is a piece, else 0 (negative: a bad index): x, its piece
 *                                 number j, pre = b_j and post = n - e_j (x = -1 and zeros for a plain pattern)
 *   acm_automaton_approx_reach    back = the largest n, ahead = the largest post: what a streaming caller keeps
 *                                 of the text in front, and how far behind a record a match can end.  Both 0
 *                                 without approximate patterns.
 * NOT composed: position windows, sequences, replacements, select and the word pass see a piece as the plain
 * pattern it is (its own bytes, its own span).  Insertions and deletions: see EDIT PATTERNS below
 * (acm_automaton_add_edit, acm_edit_matches_async), where the span's length is an output.
 *
 * EDIT PATTERNS: up to k substituted, inserted or deleted bytes.  An edit pattern is n bytes and a budget k,
 * 1 <= k <= ACM_EDIT_MAX_K and k + 1 <= n <= ACM_APPROX_MAX_LEN.  It is an approximate pattern in every host-side
 * respect: the same pieces [b_i, e_i) as k + 1 consecutive patterns, the same acm_automaton_approx* queries, the
 * same folding.  One thing differs: its distance is the unit-cost edit distance ed (substitution, insertion and
 * deletion cost 1 each), which only acm_edit_matches_async verifies.  The pigeonhole argument holds as it stands:
 * a span within edit distance k holds at least one piece exactly.
 *   acm_automaton_add_edit        as acm_automaton_add_approx: the same return value, the same errors, nothing
 *                                 applied on an error; k above ACM_EDIT_MAX_K is ACM_ERR_LIMIT; with k == 0 it is
 *                                 exactly acm_automaton_add_ex
 *   acm_automaton_approx_mode     0 where approximate pattern x counts substitutions only (add_approx), 1 where
 *                                 it is an edit pattern (negative: a bad index)
 * For an edit pattern acm_automaton_approx_reach takes back = n + 2k and ahead = post + k: its span may begin up
 * to 2k bytes further in front and end up to k bytes further behind than the nominal one.  A set without edit
 * patterns is bit for bit what it is without them: tables, digests, acm_dfa_device_bytes and the reach. */
#define ACM_APPROX_MAX_K 15
#define ACM_APPROX_MAX_LEN 4096
#define ACM_EDIT_MAX_K 4
int acm_automaton_add_approx(acm_automaton *, const unsigned char *bytes, int n, int k, int iid,
    unsigned flags);
int acm_automaton_num_approx(const acm_automaton *);
int acm_automaton_approx(const acm_automaton *, int x, int *first_piece, int *n, int *k, int *iid,
    unsigned *flags, const unsigned char **bytes);
int acm_automaton_pattern_approx(const acm_automaton *, int index, int *x, int *piece, int *pre, int *post);
int acm_automaton_approx_reach(const acm_automaton *, int *back, int *ahead);
int acm_automaton_add_edit(acm_automaton *, const unsigned char *bytes, int n, int k, int iid,
    unsigned flags);
int acm_automaton_approx_mode(const acm_automaton *, int x);

/* Rules: a boolean condition over the signatures that hit ONE text.  A RULE is nops operands, 1 <= nops <=
 * ACM_RULE_MAX_OPERANDS, an expression over them and a user id iid.  Operand j is a SEQUENCE index: the id
 * space in which plain patterns (1-part sequences), multi-part signatures and wildcard signatures meet.  A
 * sequence may be an operand of at most one rule and appear at most once in that rule's operand list; the
 * expression may name an operand any number of times.  To use the same bytes in two rules, add the
 * signature twice.
 * Expressions.  Blanks and tabs between tokens are skipped, nothing else is allowed there:
 *   expr := term ( '&' term )*  |  term ( '|' term )*
 *   term := ( NUMBER | '(' expr ')' ) [ ( '=' | '>' | '<' ) NUMBER ]
 * '&' and '|' at one nesting level without parentheses are ACM_ERR_PARSE: there is no precedence to get
 * wrong.  An operand NUMBER is < nops (else ACM_ERR_PARSE), a comparison NUMBER lies in [0, INT32_MAX].
 * Parentheses nest at most ACM_RULE_MAX_NESTING deep; deeper, or more operands than the maximum, is
 * ACM_ERR_LIMIT.  ClamAV's distinct-count form "=n,m" is ACM_ERR_PARSE: not provided.  Every parse error
 * names the column, counted from 1, in acm_last_error.
 * Values.  Every node has a COUNT (int64) and a TRUTH:
 *   operand      count: the occurrences of its sequence in the text      truth: count > 0
 *   '&'          count: the sum of its children's counts                 truth: all children true
 *   '|'          count: the sum of its children's counts                 truth: any child true
 *   comparison   count: unchanged                                        truth: count = n, count > n, count < n
 * So "A=0" is "A does not occur", and "(0|1)>3" is "more than three hits of the two together" (ClamAV's
 * reading of a block).  A rule whose expression is true with every count 0 ("0=0", "0<5") is refused with
 * ACM_ERR_ARG: no record could trigger it, which is what lets the pass look only at (rule, text) pairs that
 * have a hit.  Negation is legal beside something positive: "0&1=0".
 * Rules do not enter acm_automaton_compile: tables, digests, self-tests, the reference table and
 * acm_dfa_device_bytes of an automaton without rules are what they were.  They may be added before or after
 * compile; acm_dfa_upload takes a copy.  acm_rule_matches_async evaluates them on the device.
 *   acm_automaton_add_rule           returns the rule index.  ACM_ERR_ARG: a bad sequence index, a sequence
 *                                    already an operand (also twice in this call), nops < 1, the empty-text
 *                                    refusal.  On any error nothing is applied.
 *   acm_automaton_rule               rule i: iid, nops, borrowed pointers to the operands and the expression
 *                                    as given (any may be NULL)
 *   acm_automaton_sequence_rule      1 and (rule, operand) if the sequence is an operand, else 0
 *   acm_automaton_add_logical_signature  parses "expr;body0;body1;..." -- a ClamAV .ldb line without its name
 *                                    and target fields -- adds each body with
 *                                    acm_automaton_add_signature_ex(..., iid, flags, syntax) and registers the
 *                                    rule over the sequences that came back; returns the rule index.  The
 *                                    whole line is parsed (the expression, every body, the room for
 *                                    wildcard sets) before anything is added.  Subsignature offsets
 *                                    ("EOF-10:") and "::" modifiers are ACM_ERR_PARSE.  Only before compile.
 *   acm_automaton_load_logical_file  one such line per line, with an optional leading "<decimal iid>:",
 *                                    otherwise the iid is the rule index; '#' lines and blank lines are
 *                                    skipped.  A bad line names its line number and nothing of the file is
 *                                    applied.  Returns the number of rules added.
 * Not provided: counts carried across calls (a text whose records lie in different calls: scan whole
 * texts), the distinct-count form "=n,m", .ldb target blocks and subsignature offsets.  The reference-named
 * layer is unchanged. */
#define ACM_RULE_MAX_OPERANDS 64
#define ACM_RULE_MAX_NESTING 8
int acm_automaton_add_rule(acm_automaton *, const int32_t *sequences, int nops, const char *expr, int iid);
int acm_automaton_num_rules(const acm_automaton *);
int acm_automaton_rule(const acm_automaton *, int index, int *iid, int *nops, const int32_t **sequences,
    const char **expr);
int acm_automaton_sequence_rule(const acm_automaton *, int sequence, int *rule, int *operand);
int acm_automaton_add_logical_signature(acm_automaton *, const char *line, int iid, unsigned flags,
    unsigned syntax);
int acm_automaton_load_logical_file(acm_automaton *, const char *path, unsigned flags, unsigned syntax);

/* ASCII case-insensitive matching for every pattern of the automaton.  With
 * it on, fold(b) = b - 0x20 for 'a' <= b <= 'z' and b otherwise (toupper in
 * the C locale; bytes >= 0x80 are never folded), and a scan of text T gives
 * bit for bit what the automaton of the folded patterns gives on fold(T):
 * same records, planes, states and overflow, pattern indices and iids those
 * of the patterns as added.  acm_automaton_pattern still returns the bytes as
 * added.  Off by default.  Only before acm_automaton_compile: afterwards it
 * fails with ACM_ERR_ARG.  Case sensitivity per pattern: acm_automaton_add_ex
 * above.  Not provided: any folding beyond ASCII letters.  The reference-named
 * layer (acsm_add_pattern's nocase argument) keeps ignoring the flag as the
 * reference does. */
int acm_automaton_set_nocase(acm_automaton *, int enable);
/* 1 if every pattern of the automaton matches case-insensitively, else 0 (a
 * mixed automaton: 0) */
int acm_automaton_nocase(const acm_automaton *);

/* trie -> fail links -> full DFA, reference state numbering preserved
 * (acsmx.c:552-594) and a BFS renumbering derived for the device. */
int acm_automaton_compile(acm_automaton *);

int acm_automaton_num_patterns(const acm_automaton *);
int acm_automaton_max_pattern_len(const acm_automaton *);
/* byte classes of a compiled automaton: bytes that occur in no pattern share
 * one DFA column, every other byte has its own.  256 = every byte its own
 * (no compression).  class_of, if not NULL, gets the 256-entry byte -> class
 * map.  The chain pipeline's planes have one cell per class. */
int acm_automaton_byte_classes(const acm_automaton *, uint8_t *class_of);
/* The LDS-resident form of a small automaton (full rows for the shallow states, a 4-byte record
 * for every other: csrc/compact_tables.h), built on the host and checked transition by transition
 * against the dense DFA -- no device needed.  lds_bytes: what the image may take (0: a CU's 160 KiB
 * less a margin).  Returns 1 if the set qualifies and every (state, byte) transition agrees, 0 if it
 * does not qualify (too many states or byte classes, or the rows that must be full do not fit),
 * negative on error.  stats, if not NULL, gets 9 words: states, classes, rows, side entries, image
 * bytes, rows beyond the mandatory ones, simple records, side entries ending in a row, side entries
 * deferring to the fail state. */
int acm_compact_selftest(const acm_automaton *, uint32_t lds_bytes, uint32_t *stats);
/* The tables of the sparse pipeline (Bloom filter, gram buckets, prefix slots, node records and edges:
 * csrc/sieve_tables.h), built on the host exactly as acm_dfa_upload builds them and looked up again by
 * plain serial code -- no device needed.  Checked: every pattern's 3-gram at every sampled offset is
 * found within the recorded number of buckets with its offset bit set, and no entry has a bit that no
 * pattern justifies; every filter key has its four bits; every depth-D trie node is found under its
 * path bytes within the recorded number of slots, with the automaton's run; the records and the
 * sorted edges reproduce the children of every state; the byte into each state of a unary run is the
 * trie edge's.  Returns 1 if all of that holds, 0 if the set does not qualify for the pipeline (no
 * pattern, one shorter than 3 bytes, 2^24 edges or more), negative on error or when a check fails
 * (acm_last_error names the first failing item).  stats, if not NULL, gets ACM_SIEVE_STATS words:
 *  [0] stride W  [1] prefix length D  [2] filter key bytes LG  [3] log2 of the Bloom filter's words
 *  [4] bits set in the filter  [5] distinct filter keys  [6] distinct 3-grams  [7] log2 of the gram
 *  buckets  [8] full buckets  [9] gram probe bound  [10] log2 of the prefix slots  [11] occupied slots
 *  [12] prefix probe bound  [13] largest number of children of a state of depth >= D  [14] longest
 *  unary run behind such a state  [15] edges  [16..20] FNV-1a (32 bits) of the bytes of the Bloom
 *  words, gram buckets, prefix slots, records and edges as uploaded.  All zero when 0 is returned. */
#define ACM_SIEVE_STATS 21
int acm_sieve_selftest(const acm_automaton *, uint32_t *stats);
/* tuning aid, host only: walks text through the LDS form from the root; counts[5] = steps, steps
 * decided by the record or a row alone, by one side entry, by more than one hop, final states entered.
 * Returns 1, or 0 if the set does not qualify. */
int acm_compact_profile(const acm_automaton *, const unsigned char *text, size_t n, uint64_t *counts);
/* states as acsm_get_states reports them after acsm_gen_state_table */
int acm_automaton_num_states(const acm_automaton *);
/* bytes of the reference's serialised table: states * 2 * 256 * 4 */
size_t acm_automaton_reference_table_bytes(const acm_automaton *);
/* write the reference-format table [states][2][256] int32 (acsmx.c:640-658);
 * cells the reference leaves uninitialised are written as 0 */
int acm_automaton_export_reference_table(const acm_automaton *, int32_t *dst);
/* pattern i: iid, length, bytes (borrowed pointer), index of the next
 * pattern chained to it by acsm_get_patterns_table (acsmx.c:707-721) or -1 */
int acm_automaton_pattern(const acm_automaton *, int index, int *iid, int *n,
    const unsigned char **bytes, int *next_chained);
/* fail link and trie depth of reference state s (depth(root) = 0, depth(fail(s)) < depth(s) for
 * every other state): what the segment pass (acm_segment_matches_async) walks.  ACM_ERR_ARG for an
 * uncompiled automaton or a state out of range.  For host tests and FFI users. */
int acm_automaton_state_fail(const acm_automaton *, int ref_state);
int acm_automaton_state_depth(const acm_automaton *, int ref_state);
/* head-of-match-list pattern index of reference state s, or -1 */
int acm_automaton_state_output(const acm_automaton *, int ref_state);
/* every pattern that ends where the walk enters ref_state, in the order of the
 * state's match list (acsmx.c:299-312, :417-429; the first one is what
 * acm_automaton_state_output returns).  Writes at most cap indices, returns
 * the length of the list (0 for a non-final state, -1 on a bad argument). */
int acm_automaton_state_matches(const acm_automaton *, int ref_state, int32_t *out, int cap);

/* ---------------------------------------------------------------------- */
/* device-resident DFA                                                     */
/* replaces the d_trans upload of acsm_gen_state_table (acsmx.c:618-666)   */
/* ---------------------------------------------------------------------- */
typedef struct acm_dfa acm_dfa;

/* builds the HBM/LDS layout and uploads it to HIP device 'device' */
int acm_dfa_upload(const acm_automaton *, int device, acm_dfa **out);
void acm_dfa_release(acm_dfa *);
size_t acm_dfa_device_bytes(const acm_dfa *);
int acm_dfa_hot_rows(const acm_dfa *);	/* rows staged in LDS by the scan */
int acm_dfa_device(const acm_dfa *);

/* ---------------------------------------------------------------------- */
/* scan pipeline on caller-owned device memory                             */
/* replaces ocl_aho_match + ocl_prefix_sum + ocl_compact_array             */
/* (ocl_aho_match.h:28-29, ocl_prefix_sum.h:21-22, ocl_compact_array.h:21) */
/* ---------------------------------------------------------------------- */

/* bytes of scratch the pipeline needs to scan up to max_text bytes */
size_t acm_scan_workspace_bytes(const acm_dfa *, size_t max_text);

/*
 * Scan d_text[0..n) as one byte stream starting from reference state
 * init_state and produce, in position order, one record per text position
 * whose transition enters a final state:
 *
 *   d_pat_plane[0] = m            d_off_plane[0] = m
 *   d_pat_plane[1..m] = pattern index (head of match list, acsmx.c:650)
 *   d_off_plane[1..m] = offset of the LAST byte of the match
 *   d_*_plane[m+1] = state after the last byte, reference numbering
 *
 * i.e. the compact layout of compactarray.cl:49-55 / databuf.c:656-682.
 * plane_capacity counts int32 cells per plane and must be >= 2; when
 * m + 2 > plane_capacity the first plane_capacity-2 records are stored,
 * cell [0] still holds the full m, the state goes to cell
 * [plane_capacity-1], and ACM_ERR_CAPACITY is reported by acm_scan_finish.
 *
 * d_text must be 16-byte aligned and readable up to n rounded up to 16.
 * Everything is enqueued on 'stream' (a hipStream_t, NULL = default stream);
 * nothing is synchronised.  n <= 2^31 - 17.
 *
 * A mixed automaton (acm_automaton_mixed_case): the records of this and of
 * every other scan entry point are candidates, those of the nocase automaton
 * of the same patterns; acm_case_matches_async keeps the exact ones.
 */
int acm_scan_async(const acm_dfa *, const void *d_text, size_t n,
    long init_state, void *d_workspace, size_t workspace_bytes,
    int32_t *d_pat_plane, int32_t *d_off_plane, size_t plane_capacity,
    void *stream);

/*
 * Shard form of acm_scan_async for texts split across devices (or rounds):
 * the first 'halo' bytes of d_text are context only -- they warm the state
 * up, records ending inside them are dropped -- and every reported offset is
 * shifted by offset_shift (e.g. shard_base - halo, to report offsets in the
 * coordinates of the whole text).  With halo >= max_pattern_len - 1 bytes of
 * real preceding text and init_state 0, the records equal those of the
 * serial scan of the whole text restricted to this shard.
 */
int acm_scan_shard_async(const acm_dfa *, const void *d_text, size_t n,
    size_t halo, long offset_shift, long init_state, void *d_workspace,
    size_t workspace_bytes, int32_t *d_pat_plane, int32_t *d_off_plane,
    size_t plane_capacity, void *stream);

/* tuning knobs for acm_scan_async; 0 = automatic.  chain_bytes: bytes each
 * lane walks per tile (power of two, 16..256).  Returns the value in use. */
int acm_scan_set_chain_bytes(acm_dfa *, int chain_bytes);

/*
 * Everything acm_scan_shard_async takes, plus two optional hipEvent_t for
 * keeping several batches in flight on different streams (what the
 * reference does with its -w workers, one queue each): the first kernel
 * of a pipeline (chain: the walk, sparse: the bulk pass) is the stage that
 * fills the device, so consecutive batches can be chained through it --
 * batch k+1's first kernel waits for wait_before_walk (recorded by batch k
 * as record_after_walk) -- while everything behind it runs concurrently
 * with the next batch's first kernel.  Optional: independent streams alone
 * overlap as well, and that is what bench.py measures.  Every batch that is
 * enqueued records its record_after_walk, an empty text (n == 0: no walk)
 * behind the kernel that writes its header and trailer, so a waiter never
 * sees an older record of the event.
 */
typedef struct acm_scan_batch {
	const void *d_text;
	size_t n;
	size_t halo;
	long offset_shift;
	long init_state;
	void *d_workspace;
	size_t workspace_bytes;
	int32_t *d_pat_plane;
	int32_t *d_off_plane;
	size_t plane_capacity;
	void *stream;
	void *wait_before_walk;		/* hipEvent_t or NULL */
	void *record_after_walk;	/* hipEvent_t or NULL */
	int report;			/* ACM_REPORT_* */
	int profile;			/* non-zero: time this batch's kernels with
					 * events as acm_scan_profile_enable does
					 * for all (acm_scan_profile_read collects) */
	/* The state to start in, handed over on the device: the pattern plane of
	 * the scan this one continues (its trailer cell, found behind its header
	 * cell, holds that scan's final state: databuf.c:622, ahomatch.cl:42-43)
	 * and the capacity that plane was scanned with.  NULL: init_state above.
	 * The scan it names must be in front of this one on the same stream, or
	 * complete.  No host read between consecutive buffers of a worker; such a
	 * batch has its launches to itself (it does not join a launch group). */
	const int32_t *d_init_plane;
	size_t init_plane_capacity;
} acm_scan_batch;

/* What the pattern plane of a scan holds per record.
 *   HEAD   the pattern index the reference reports: the head of the final
 *          state's match list (acsmx.c:650)
 *   STATE  the final state itself (reference numbering), for
 *          acm_expand_matches_async: all-patterns reporting, SURVEY 8(f) row 4 */
enum { ACM_REPORT_HEAD = 0, ACM_REPORT_STATE = 1 };

/* All-patterns reporting.  Input: the planes of a scan enqueued with
 * report = ACM_REPORT_STATE (at most max_records records are looked at).
 * Output, same cell layout ([0] = count, records, trailer = final state): one
 * record per pattern of each final state's match list -- every pattern that
 * ends at that offset, in list order, offsets ascending.  The reference never
 * reports more than the head (ocl_aho_grep.c:276-279 has the table for it,
 * acsmx.c:707-721); off unless asked for.  Stream-ordered, no host sync. */
size_t acm_expand_workspace_bytes(size_t max_records);
int acm_expand_matches_async(const acm_dfa *, const int32_t *d_state_plane,
    const int32_t *d_off_plane, size_t max_records, int32_t *d_pat_out,
    int32_t *d_off_out, size_t out_capacity, void *d_workspace,
    size_t workspace_bytes, void *stream);

/* Segmented scans: many independent texts in one scan, each matched as if scanned alone from the
 * root.  Input: the planes of a scan enqueued with report = ACM_REPORT_STATE (at most max_records
 * records are looked at, as in acm_expand_matches_async), and the start offsets of the texts,
 * d_seg_start[segments]: non-decreasing, in the coordinates of the reported offsets (offset_shift of a
 * shard or halo scan included); empty segments (equal starts) and starts at or beyond text_end are
 * allowed.  A record at offset o belongs to the last segment k with start[k] <= o; its state is
 * clamped to the first state on its fail chain whose depth is <= o - start[k] + 1 (the state a walk
 * restarted at start[k] would be in), and the record is kept iff that state's match list is not empty.
 * A record before start[0] continues a text that began before this scan: it is not clamped and its
 * segment is -1.  segments == 0: nothing is clamped (the output is the input in the report form asked).
 * Output, the scan's cell layout and overflow contract ([0] = full count of kept records, records in
 * position order, trailer at min(count + 1, out_capacity - 1)):
 *   d_pat_out   report = ACM_REPORT_HEAD: the head of the clamped state's match list (what the scan
 *               reports); ACM_REPORT_STATE: the clamped state (for acm_expand_matches_async)
 *   d_off_out   the offset, unchanged
 *   d_seg_out   (NULL: not wanted) the segment k, or -1
 *   trailer     the input trailer clamped with b = text_end - start[k], k the last segment with
 *               start[k] <= text_end (b = 0: the root): the state the next buffer starts in, so the
 *               output planes can be handed to the next scan as acm_scan_batch.d_init_plane with
 *               init_plane_capacity = out_capacity
 *   d_seg_counts (NULL: not wanted) int32[segments], written whole: records kept per segment
 * The output planes must not overlap the input planes.  Stream-ordered, no host sync, no allocation;
 * argument errors return ACM_ERR_ARG before anything is enqueued.  The scan kernels are not involved:
 * it is a pass over the records (cost per record, not per text byte). */
size_t acm_segment_workspace_bytes(size_t max_records);
int acm_segment_matches_async(const acm_dfa *, const int32_t *d_state_plane,
    const int32_t *d_off_plane, size_t max_records, const int32_t *d_seg_start,
    size_t segments, long text_end, int report, int32_t *d_pat_out, int32_t *d_off_out,
    int32_t *d_seg_out, size_t out_capacity, int32_t *d_seg_counts, void *d_workspace,
    size_t workspace_bytes, void *stream);

/* Whole-word matching (grep -w).  A word byte is a byte of the set W: word_set (host, 32 bytes, bit
 * b of byte b / 8 set = byte b is a word byte), or with word_set NULL the default [0-9A-Za-z_] (grep's
 * C locale; bytes >= 0x80 are not word bytes).  Pattern P of length L >= 1 that ends at offset o
 * (starts at a = o - L + 1) is word-bounded when both hold:
 *   the byte at a - 1 is not in W, or a is the start of the text;
 *   the byte at o + 1 is not in W, or o + 1 is the end of the text.
 * Only the bytes outside the match are looked at (grep -w, not a regex \b); patterns of length 0 are
 * never word-bounded.  The test reads raw text bytes: case folding (nocase automata) does not enter.
 * Input: the planes of a scan enqueued with report = ACM_REPORT_STATE, or of the segment pass in STATE
 * form (at most max_records records are looked at, as in acm_expand_matches_async), offsets in the
 * coordinates the scan reported (offset_shift included: a shard or halo scan passes its halo as part
 * of d_text with text_origin = offset_shift).  The text:
 *   d_text      d_text[i] = the byte at offset text_origin + i, for offsets [text_origin, text_end)
 *   d_before    the bytes at [text_origin - before_len, text_origin) (a streaming caller's previous
 *               piece); offsets further back are the text start
 *   next_byte   the byte at text_end, or -1: the text ends there
 *   d_seg_start optional (segments == 0: none), as in acm_segment_matches_async: every start is a text
 *               start and the end of the text in front of it.  Pass the segment pass's output.
 * Output, the scan's cell layout and overflow contract ([0] = full count, records, trailer at
 * min(count + 1, out_capacity - 1)):
 *   all_patterns == 0  one record per offset where some pattern of the record's state is word-bounded:
 *                      the first such pattern in match-list order (acm_automaton_state_matches).  With
 *                      an empty W this is the scan's HEAD records bit for bit.
 *   all_patterns != 0  one record per word-bounded pattern, list order, offsets ascending.  With an
 *                      empty W this is acm_expand_matches_async's output bit for bit.
 *   trailer            the input trailer unchanged: the output can be the next scan's d_init_plane
 *   d_tail_out         (NULL: not wanted) the last min(max_pattern_len, before_len + text_end -
 *                      text_origin) bytes of before ++ text: the next piece's d_before.  It must not
 *                      overlap d_before or d_text.
 * Chained calls over consecutive pieces of a stream (each piece's d_before the previous piece's tail,
 * its next_byte the first byte of the following piece) give exactly the records of one call over the
 * whole stream.  No text read leaves [text_origin, text_end) of d_text or d_before, whatever the
 * records hold.  The output planes must not overlap the input planes.  Stream-ordered, no host sync,
 * no allocation; argument errors return ACM_ERR_ARG before anything is enqueued.  A pass over the
 * records (cost per record, not per text byte); the scan kernels are not involved. */
size_t acm_word_workspace_bytes(size_t max_records);
int acm_word_matches_async(const acm_dfa *, const int32_t *d_state_plane,
    const int32_t *d_off_plane, size_t max_records, const void *d_text, long text_origin,
    long text_end, const void *d_before, size_t before_len, int next_byte,
    const int32_t *d_seg_start, size_t segments, const uint8_t *word_set, int all_patterns,
    int32_t *d_pat_out, int32_t *d_off_out, size_t out_capacity, void *d_tail_out,
    void *d_workspace, size_t workspace_bytes, void *stream);

/* Case sensitivity per pattern: the records of a mixed automaton (acm_automaton_add_ex) made exact.
 * The scan of a mixed automaton has proved fold(text) == fold(pattern) for every entry of a record's
 * match list; this pass keeps pattern p of length L >= 1 in the list of a record's state at offset o
 * iff p ignores case (ACM_PATTERN_NOCASE), or every byte at [o - L + 1, o] equals the pattern's byte
 * as added.  A byte outside the bytes given (in front of text_origin - before_len, or at or behind
 * text_end) equals nothing: an exact pattern that reaches there is dropped.  Patterns of length 0
 * never report; a cell that is no state writes nothing.
 * Input: the planes of a scan enqueued with report = ACM_REPORT_STATE, or of the segment pass in STATE
 * form (at most min([0], max_records) records are looked at), offsets in the coordinates the scan
 * reported.  The text:
 *   d_text      d_text[i] = the byte at offset text_origin + i, for offsets [text_origin, text_end)
 *   d_before    the bytes at [text_origin - before_len, text_origin) (a streaming caller's previous
 *               piece's tail)
 * No next byte is needed: only bytes under a match are read.  No segment argument is needed either:
 * after the segment pass every list entry of a clamped state lies inside its own text.
 * Output, the scan's cell layout and overflow contract ([0] = full count, records, trailer at
 * min(count + 1, out_capacity - 1)):
 *   all_patterns == 0  one record per input record that has a kept entry: the first kept entry in
 *                      match-list order (acm_automaton_state_matches) and the offset, unchanged
 *   all_patterns != 0  one record per kept entry, list order, offsets ascending
 *   trailer            the input trailer unchanged: the output can be the next scan's d_init_plane
 *   d_tail_out         (NULL: not wanted) the last min(max_pattern_len, before_len + text_end -
 *                      text_origin) bytes of before ++ text: the next piece's d_before.  It must not
 *                      overlap d_before or d_text.
 * For an automaton that is not mixed the call is legal and every entry is kept: the all form is
 * acm_expand_matches_async's output and the head form the HEAD scan's records, bit for bit (entries of
 * length 0 aside, which the scan reports and this pass, as the word pass, never does).
 * Chained calls over consecutive pieces of a stream (each piece's d_before the previous piece's tail)
 * give exactly the records of one call over the whole stream.  No read leaves [0, text_end -
 * text_origin) of d_text or [0, before_len) of d_before, whatever the planes hold.  The output planes
 * must not overlap the inputs.  Stream-ordered, no host sync, no allocation; argument errors return
 * ACM_ERR_ARG before anything is enqueued.  A pass over the records (cost per record and per pattern
 * byte under it, never per text byte); the scan kernels are not involved.  The workspace query is
 * monotone and a multiple of 256. */
size_t acm_case_workspace_bytes(size_t max_records);
int acm_case_matches_async(const acm_dfa *, const int32_t *d_state_plane,
    const int32_t *d_off_plane, size_t max_records, const void *d_text, long text_origin,
    long text_end, const void *d_before, size_t before_len, int all_patterns,
    int32_t *d_pat_out, int32_t *d_off_out, size_t out_capacity, void *d_tail_out,
    void *d_workspace, size_t workspace_bytes, void *stream);

/* Position constraints (acm_automaton_set_position) applied to the records of any pass: an entry is
 * kept iff its pattern's window holds in the text the record belongs to.  No text is read: the predicate
 * needs the pattern's length, the record's offset and the bounds of its text.
 * Input: planes in the scan's cell layout; at most min([0], max_records) records are looked at.  report
 * says what the cells of d_pat_plane are:
 *   ACM_REPORT_STATE  final states (a STATE scan, the segment pass in STATE form).  The entries of a
 *                     record are its state's match list (acm_automaton_state_matches).
 *   ACM_REPORT_HEAD   pattern indices (a HEAD scan, or the all-patterns output of the word pass, the
 *                     case pass or acm_expand_matches_async).  Each record is one entry; a maximal run
 *                     of consecutive records with equal offset counts as one offset.  This is how the
 *                     pass composes with the word and case passes, which take states and give patterns.
 * Which text a record belongs to: d_seg_start[segments] as in acm_tally_matches_async (non-decreasing,
 * empty segments and starts at or beyond text_end allowed).  A record at o belongs to the last k with
 * start[k] <= o, and T0 = start[k].  A record in front of start[0], or any record when segments == 0,
 * belongs to the lead text: T0 = lead_begin, which may lie far in front of the piece or be negative (a
 * text that began in an earlier buffer).  Tend is the next start if that start is <= text_end.  Otherwise
 * the text is open and Tend = open_end: the known end (>= text_end, same coordinates; text_end itself
 * when the stream ends there), or -1: unknown.  An ACM_POS_FROM_END entry of an open text whose end is
 * unknown is UNDECIDED: it is dropped and counted.  Nothing is clamped: for per-text matching run the
 * segment pass first.  An unconstrained entry is always kept, whatever its text is.
 * Output, the scan's cell layout and overflow contract ([0] = full count, records, trailer -- the input
 * trailer unchanged -- at min(count + 1, out_capacity - 1)):
 *   all_patterns != 0  one record per kept entry, in list order (STATE input) or input order (HEAD
 *                      input), offsets ascending
 *   all_patterns == 0  the first kept entry per record (STATE input) or per run of equal offsets (HEAD
 *                      input)
 *   d_info             int32[4], required, written whole: [0] undecided entries dropped, [1..3] 0.  In
 *                      the first-entry form only the entries in front of the first kept one of their
 *                      record or run are looked at, and only those are counted.
 * For an automaton that is not positioned the call is legal and every entry is kept: STATE input in the
 * all form is acm_expand_matches_async's output, in the first form the HEAD scan's records, and HEAD
 * input in the all form is the input, all bit for bit (entries of length 0 aside, which the scan reports
 * and this pass, as the word and case passes, never does).  A cell that is neither a state nor a pattern
 * index writes nothing.  No read leaves the input planes, the starts and the library's tables, whatever
 * the planes hold.  The outputs must not overlap the inputs.  Stream-ordered, no host sync, no
 * allocation, no host read of device data; argument errors (a NULL plane, output or d_info, out_capacity
 * < 2, an unknown report, open_end outside {-1} and [text_end, inf), segments without starts, a short
 * workspace) return ACM_ERR_ARG before anything is enqueued.  Two launches over the records
 * (csrc/position.hip); cost per record and per list entry, never per text byte (a first-form run of
 * HEAD input looks back over its own run: bounded by the longest match list for the planes of a pass).
 * The workspace query is monotone and a multiple of 256. */
size_t acm_position_workspace_bytes(size_t max_records);
int acm_position_matches_async(const acm_dfa *, const int32_t *d_pat_plane,
    const int32_t *d_off_plane, size_t max_records, int report, const int32_t *d_seg_start,
    size_t segments, long lead_begin, long text_end, long open_end, int all_patterns,
    int32_t *d_pat_out, int32_t *d_off_out, size_t out_capacity, int32_t *d_info,
    void *d_workspace, size_t workspace_bytes, void *stream);

/* Wildcard patterns (acm_automaton_add_wildcard) confirmed on the device: an entry is kept iff the bytes around
 * its anchor lie in the pattern's context sets.  A pass over the records: cost per record and per context byte,
 * never per text byte; no scan kernel is involved.
 * Input: planes in the scan's cell layout; at most min([0], max_records) records are looked at.  report as in
 * acm_position_matches_async:
 *   ACM_REPORT_STATE  final states; the entries of a record are its state's match list
 *   ACM_REPORT_HEAD   pattern indices, one entry per record (a HEAD scan, or the all-patterns output of the
 *                     expand, case or position pass).  Needs all_patterns != 0, else ACM_ERR_ARG: the first
 *                     form of acm_position_matches_async behind this pass gives the head per offset.
 * The text bytes are given as to acm_case_matches_async (d_text, text_origin, text_end, d_before, before_len).
 * The text [T0, Tend) of a record is found as acm_position_matches_async finds it (d_seg_start, segments,
 * lead_begin; Tend the next start if it is <= text_end, else open_end, or unknown when that is -1: no end
 * is then in the way).
 * The rule for entry (p, o) with L >= 1, a = o - L + 1 and span [a - pre, o + post], int64 arithmetic, in
 * this order:
 *   1. p has no context: kept, whatever its text is
 *   2. the span leaves [T0, Tend): dropped
 *   3. the span leaves the bytes given, [text_origin - before_len, text_end): UNDECIDED -- dropped and
 *      counted, whatever the available bytes hold
 *   4. kept iff every context byte is in its set
 * Output, the scan's cell layout and overflow contract ([0] = full count, records, trailer -- the input
 * trailer unchanged -- at min(count + 1, out_capacity - 1)); offsets are the anchors' ends, unchanged, so the
 * order is the input's (a match ends post bytes behind its offset):
 *   all_patterns != 0  one record per kept entry, in list order (STATE input) or input order (HEAD input)
 *   all_patterns == 0  STATE input only: the first kept entry per record
 *   d_info             int32[4], required, written whole: [0] undecided entries, [1..3] 0.  In the first
 *                      form only the entries in front of a record's first kept one are looked at and counted.
 * For an uploaded set without contexts the call is legal and every entry of length >= 1 is kept: STATE input
 * in the all form is acm_expand_matches_async's output, in the first form the HEAD scan's records, and HEAD
 * input is the input, all bit for bit (entries of length 0 aside).  A cell that is neither a state nor a
 * pattern index writes nothing.  No read leaves the input planes, the starts, [0, text_end - text_origin)
 * of d_text, [0, before_len) of d_before and the library's tables, and no write leaves the outputs and the
 * workspace, whatever the planes hold.  The outputs must not overlap the inputs.  Stream-ordered, no host
 * sync, no allocation, no host read of device data; argument errors (a NULL plane, output or d_info,
 * out_capacity < 2, an unknown report, HEAD input in the first form, a bad text window, open_end outside
 * {-1} and [text_end, inf), segments without starts, a short workspace) return ACM_ERR_ARG before anything
 * is enqueued.  Two launches (csrc/wildcard.hip).  The workspace query is monotone and a multiple of 256. */
size_t acm_wildcard_workspace_bytes(size_t max_records);
int acm_wildcard_matches_async(const acm_dfa *, const int32_t *d_pat_plane,
    const int32_t *d_off_plane, size_t max_records, int report, const void *d_text, long text_origin,
    long text_end, const void *d_before, size_t before_len, const int32_t *d_seg_start,
    size_t segments, long lead_begin, long open_end, int all_patterns, int32_t *d_pat_out,
    int32_t *d_off_out, size_t out_capacity, int32_t *d_info, void *d_workspace,
    size_t workspace_bytes, void *stream);

/* Approximate patterns (acm_automaton_add_approx) confirmed on the device: where a piece matched, the
 * mismatches of the whole pattern are counted.  A pass over the records: cost per record and per compared
 * byte, never per text byte; no scan kernel is involved.
 * Input, text bytes and texts exactly as acm_wildcard_matches_async takes them (report: ACM_REPORT_STATE, or
 * ACM_REPORT_HEAD for pattern cells: a HEAD scan or the all-patterns output of the expand, case or position
 * pass).  The pass always writes one record per kept entry: there is no first-entry form.
 * The rule for entry (p, o) with L >= 1, int64 arithmetic, in this order:
 *   1. p is no piece: kept, distance 0
 *   2. p is piece j of pattern A (n bytes, budget k): a = o - L + 1, s = a - b_j, span [s, s + n).  The span
 *      leaves [T0, Tend): dropped
 *   3. the span leaves the bytes given, [text_origin - before_len, text_end): UNDECIDED -- dropped and counted,
 *      whatever the available bytes hold
 *   4. m_i = the mismatches of piece i against the text under it (raw bytes, or both sides folded if A folds):
 *      kept iff m_j == 0, m_i > 0 for every i < j and the sum of all m_i <= k
 * Rule 4 reports an occurrence within the budget exactly once, by its first exact piece, without a sort.  It
 * stands on the text alone: a mixed automaton needs no case pass in front, and a pattern cell that names a
 * piece where none matched is dropped.
 * Output, the scan's cell layout and overflow contract ([0] = full count, records, trailer -- the input trailer
 * unchanged -- at min(count + 1, out_capacity - 1)), per kept entry in list order (STATE) or input order (HEAD):
 *   d_pat_out    p, the piece (acm_automaton_pattern_approx names its pattern)
 *   d_off_out    o, unchanged: the order is the input's, and the match ends post bytes behind o
 *   d_dist_out   NULL, or a third plane of out_capacity cells: the sum of the m_i in the record's cell; cell 0
 *                and the trailer as in the other planes
 *   d_info       int32[4], required, written whole: [0] undecided entries, [1..3] 0
 * For an uploaded set without approximate patterns the call is legal: STATE input gives
 * acm_expand_matches_async's output and HEAD input the input, bit for bit (entries of length 0 aside), with
 * distances 0.  A cell that is neither a state nor a pattern index writes nothing.  No read leaves the input
 * planes, the starts, [0, text_end - text_origin) of d_text, [0, before_len) of d_before and the library's
 * tables, and no write leaves the outputs and the workspace, whatever the planes hold.  The outputs must not
 * overlap the inputs.  Stream-ordered, no host sync, no allocation, no host read of device data; argument
 * errors (a NULL plane, output or d_info, out_capacity < 2, an unknown report, a bad text window, open_end
 * outside {-1} and [text_end, inf), segments without starts, a short workspace) return ACM_ERR_ARG before
 * anything is enqueued.  Two launches (csrc/approx.hip).  The workspace query is monotone and a multiple of
 * 256. */
size_t acm_approx_workspace_bytes(size_t max_records);
int acm_approx_matches_async(const acm_dfa *, const int32_t *d_pat_plane,
    const int32_t *d_off_plane, size_t max_records, int report, const void *d_text, long text_origin,
    long text_end, const void *d_before, size_t before_len, const int32_t *d_seg_start,
    size_t segments, long lead_begin, long open_end, int32_t *d_pat_out, int32_t *d_off_out,
    int32_t *d_dist_out, size_t out_capacity, int32_t *d_info, void *d_workspace,
    size_t workspace_bytes, void *stream);

/* Edit patterns (acm_automaton_add_edit) verified on the device: where a piece matched, a banded dynamic
 * program finds the nearest end within edit distance k and the shortest span that has it.  A pass over the
 * records, as acm_approx_matches_async, and the one to call for a set that holds an edit pattern
 * (acm_approx_matches_async refuses such a set with ACM_ERR_ARG).
 * Input, text bytes, texts, cell layout, overflow contract and argument errors: acm_approx_matches_async's.
 * For a text [T0, Tend) and an end e, T0 < e <= Tend, D(e) is the minimum of ed(A, T[s:e]) over T0 <= s <= e
 * (Sellers).  A piece (p, o), p piece j of edit pattern A, lies at [o - L + 1, o + 1); its nominal span begins at
 * s0 = o - L + 1 - b_j and ends at e0 = s0 + n.  If D(e) <= k some piece lies exactly inside an optimal span ending
 * at e, and that piece's e0 is within k of e.
 * The rule for entry (p, o) with L >= 1, int64 arithmetic, in this order:
 *   1. p is no piece: the candidate (p, o, 0, L)
 *   2. p is a piece of a Hamming pattern: rules 2 - 4 of acm_approx_matches_async unchanged; a kept entry gives
 *      (first piece of its pattern, o + post, sum of the m_i, n)
 *   3. p is piece j of edit pattern A with window of ends W = { e : |e - e0| <= k, T0 < e <= Tend }:
 *      - the piece itself leaves [T0, Tend): dropped
 *      - Tend is unknown (open_end == -1) and e0 + k > text_end: UNDECIDED
 *      - the bytes [max(T0, s0 - 2k), min(Tend, e0 + k)) leave the bytes given, [text_origin - before_len,
 *        text_end): UNDECIDED -- dropped and counted, whatever the available bytes hold
 *      otherwise e* is the end in W that minimises (min(D(e), k + 1), |e - e0|, e); W empty or D(e*) > k: dropped;
 *      len* is the smallest l with e* - l >= T0 and ed(A, T[e* - l : e*]) == D(e*); the candidate is
 *      (first piece of A, e* - 1, D(e*), len*)
 *   4. the output is the SET of candidates -- equal candidates collapse; two pieces that choose the same (A, e*)
 *      compute the same distance and length -- ordered by (offset, pattern)
 * A candidate whose offset lies outside the bytes given, [text_origin - before_len, text_end), is no record of this
 * text (a cell may hold anything) and is dropped: the order is keyed inside that range.
 * So every record (x, e - 1, d, l) has d == D(e) <= k and ed(A, T[e - l : e]) == d with no shorter l; no (pattern,
 * offset) appears twice; every e with D(e) == 0 is reported with length n, and for every e with D(e) <= k there is
 * a record of the same pattern at e' with |e' - e| <= 2k and distance <= D(e).  Like Hamming rule 4 this stands
 * on the text alone; with HEAD input completeness holds as far as the cells name the pieces.
 *   d_pat_out    the first piece of the pattern, or the plain pattern
 *   d_off_out    the offset of the match's last byte
 *   d_dist_out   NULL, or the distances      d_len_out   NULL, or the lengths of the spans; cell 0 and the trailer
 *                as in the other planes
 *   d_info       int32[4], required, written whole: [0] undecided entries, [1] candidates before equal ones
 *                collapse, [2..3] 0
 * For a set without edit patterns the call is legal and gives the normalised records of rules 1 - 2.  No read
 * leaves the input planes, the starts, the bytes given and the library's tables, and no write the outputs and the
 * workspace, whatever the planes hold.  Stream-ordered, no host sync, no allocation, no host read of device data.
 * The order is a stable radix sort over max_records * (the longest match list of the set) cells for STATE input and
 * max_records cells for HEAD input: size max_records to the planes.  7 + 3 * (digits of the pattern count + digits
 * of the bytes given) launches (csrc/edit.hip).  The workspace query is monotone and a multiple of 256. */
size_t acm_edit_workspace_bytes(const acm_dfa *, size_t max_records);
int acm_edit_matches_async(const acm_dfa *, const int32_t *d_pat_plane,
    const int32_t *d_off_plane, size_t max_records, int report, const void *d_text, long text_origin,
    long text_end, const void *d_before, size_t before_len, const int32_t *d_seg_start,
    size_t segments, long lead_begin, long open_end, int32_t *d_pat_out, int32_t *d_off_out,
    int32_t *d_dist_out, int32_t *d_len_out, size_t out_capacity, int32_t *d_info, void *d_workspace,
    size_t workspace_bytes, void *stream);

/* Sequences (acm_automaton_add_sequence) joined on the device: the records of the parts in, one record
 * per sequence match out.  No text is read.
 * Input: planes in the scan's cell layout whose cells are pattern indices, one record per occurrence: the
 * all-patterns output of acm_expand_matches_async or of the word, case or position pass (a HEAD scan's
 * planes also work: its one pattern per offset).  Offsets non-decreasing.  At most min([0], max_records)
 * records are looked at.  A cell that is no pattern index, or a pattern that is no part, takes part in
 * nothing.  Texts: d_seg_start[segments], lead_begin and text_end as in acm_position_matches_async.
 * Output, the scan's cell layout and overflow contract ([0] = full count, records, trailer -- the input
 * trailer unchanged -- at min(count + 1, out_capacity - 1)): one record per alive record of a sequence's
 * last part, in input order: d_seq_out the sequence index, d_off_out the offset o the match ends at.
 *   d_info   int32[4], required, written whole: [0] input records that are a part of some sequence, [1]
 *            alive records over all levels, [2..3] 0
 * For an uploaded set without sequences the call is legal and writes count 0.  Results are the same on
 * every run (integers; no order decided by atomics).  No read leaves the inputs, the starts and the
 * library's tables and no write leaves the outputs and the workspace, whatever the planes hold.  The
 * outputs must not overlap the inputs.  Stream-ordered, no host sync, no allocation, no host read of device
 * data; argument errors (a NULL plane, output or d_info, out_capacity < 2, segments without starts, a
 * short workspace) return ACM_ERR_ARG before anything is enqueued.  The records are keyed by part, ordered
 * by a stable radix sort over max_records cells (cost per max_records, not per record: size it to the
 * planes), and the levels are joined one after the other (csrc/sequence.hip): the launch count depends on
 * the uploaded set (its parts and levels) alone, never on the data.  The workspace query is monotone in
 * max_records and a multiple of 256. */
size_t acm_sequence_workspace_bytes(const acm_dfa *, size_t max_records);
int acm_sequence_matches_async(const acm_dfa *, const int32_t *d_pat_plane,
    const int32_t *d_off_plane, size_t max_records, const int32_t *d_seg_start, size_t segments,
    long lead_begin, long text_end, int32_t *d_seq_out, int32_t *d_off_out, size_t out_capacity,
    int32_t *d_info, void *d_workspace, size_t workspace_bytes, void *stream);

/* Rules (acm_automaton_add_rule) evaluated on the device: the records of the sequence pass and the text
 * starts in, one record per (rule, text) whose expression is true out.  No text is read.
 * Input: the output planes of acm_sequence_matches_async: sequence index and end offset, offsets
 * non-decreasing.  At most min([0], max_records) records are looked at.  A cell that is no sequence index,
 * or a sequence that is no operand, takes part in nothing.
 * Texts: d_seg_start[segments] as in acm_tally_matches_async: a record at offset o belongs to the last k
 * with start[k] <= o; a record in front of start[0], and every record when segments == 0, belongs to the
 * lead text, index -1.  Nothing is clamped: for per-text matching the caller runs the segment pass first,
 * as for sequences.  Counts are not carried across calls.
 * Output, three planes in the scan's cell layout and overflow contract ([0] = full count, records, trailer
 * -- the input trailer unchanged -- at min(count + 1, out_capacity - 1)): one record per (rule, text) whose
 * expression is true, at the position of its TRIGGER in input order: the first record in that text of the
 * rule's lowest-numbered operand that occurs there.  So records come text by text, and inside a text by the
 * trigger's offset.  d_rule_out the rule index, d_text_out k (-1: the lead text), d_off_out the trigger's
 * offset.
 *   d_info   int32[4], required, written whole: [0] input records that are an operand, [1] distinct
 *            (operand, text) pairs, [2] (rule, text) pairs evaluated, [3] 0
 * For an uploaded set without rules the call is legal and writes count 0.  Results are the same bytes on
 * every run (integers; no order decided by atomics).  No read leaves the inputs, the starts and the
 * library's tables and no write leaves the outputs and the workspace, whatever the planes hold; offsets out
 * of order give unspecified records, nothing worse.  The outputs must not overlap the inputs.
 * Stream-ordered, no host sync, no allocation, no host read of device data; argument errors (a NULL plane,
 * output or d_info, out_capacity < 2, segments without starts, a short workspace) return ACM_ERR_ARG before
 * anything is enqueued.  The records are keyed by operand and ordered by a stable radix sort over
 * max_records cells (cost per max_records: size it to the planes); the first record of every (operand,
 * text) run that no lower-numbered operand precedes evaluates its rule's postfix program, every count two
 * binary searches (csrc/rule.hip).  The launch count depends on the uploaded set alone.  The workspace query
 * is monotone in max_records and a multiple of 256. */
size_t acm_rule_workspace_bytes(const acm_dfa *, size_t max_records);
int acm_rule_matches_async(const acm_dfa *, const int32_t *d_seq_plane, const int32_t *d_off_plane,
    size_t max_records, const int32_t *d_seg_start, size_t segments, int32_t *d_rule_out,
    int32_t *d_text_out, int32_t *d_off_out, size_t out_capacity, int32_t *d_info, void *d_workspace,
    size_t workspace_bytes, void *stream);

/* Leftmost-longest non-overlapping selection on the device: the records of a pass in, the matches a
 * tokenizer, a redactor, a highlighter or grep -o wants out.  No text is read.
 * Input: planes in the scan's cell layout whose cells are pattern indices, one record per occurrence: the
 * all-patterns output of acm_expand_matches_async or of the word, case, position or wildcard pass (a HEAD
 * scan's planes also work: its one pattern per offset).  Offsets non-decreasing.  At most min([0],
 * max_records) records are looked at.  No segment argument: behind the segment pass no entry crosses a text
 * start, so the selection over the whole call is the selection per text.
 * The span of entry (p, o) with L = len(p) and pre, post its wildcard context (both 0 without one) is
 * [s, e] = [o - L + 1 - pre, o + post], int64 arithmetic: the starts the position and sequence passes use for
 * a wildcard pattern.  An entry is ELIGIBLE iff its cell is a pattern index, L >= 1 and s >= min_start.  A
 * cell that is no pattern index, and a pattern of length 0, take part in nothing; an entry with s < min_start
 * began in front of what the caller has: it is dropped and counted.
 * The rule: cursor c = min_start; among the eligible entries with s >= c take the smallest s, among those the
 * largest e, among those the first in the input; emit it, c = e + 1, repeat until none is left.  That is POSIX
 * leftmost-longest over the pattern set: what grep -o prints for a -F pattern list.
 * Output, the scan's cell layout and overflow contract ([0] = full count, records, trailer -- the input
 * trailer unchanged -- at min(count + 1, out_capacity - 1)), in selection order (ascending s, hence ascending
 * offset):
 *   d_pat_out    the pattern
 *   d_off_out    o, unchanged: as everywhere the end of the anchor (a match ends post bytes behind it)
 *   d_start_out  s; may be NULL (not wanted), else a third plane under the same contract, its trailer cell 0
 *   d_info       int32[4], required, written whole: [0] eligible entries, [1] entries dropped for
 *                s < min_start, [2..3] int64 (lo, hi): the cursor behind the last selected entry, min_start
 *                when nothing was selected
 * flags must be 0 (room for a second rule).  min_start lies in [INT32_MIN + 1, INT32_MAX].  Results are the
 * same bytes on every run (integers; no order decided by atomics).  No read leaves the inputs and the
 * library's tables and no write leaves the outputs and the workspace, whatever the planes hold; offsets out
 * of order give unspecified records, nothing worse.  The outputs must not overlap the inputs.  Stream-ordered,
 * no host sync, no allocation, no host read of device data; argument errors (a NULL plane, output or d_info,
 * out_capacity < 2, flags != 0, min_start out of range, a short workspace) return ACM_ERR_ARG before anything
 * is enqueued.  The entries are ordered by s with a stable radix sort over max_records cells (cost per
 * max_records, not per record: size it to the planes), the first entry of every run of equal s walks its run
 * for the largest e (bounded by the entries that begin at one byte: patterns that are prefixes of one
 * another, duplicates, contexts), and pointer doubling marks the chosen path (csrc/select.hip):
 * 16 + ceil(log2(max_records + 1)) launches, whatever the planes hold.  It adds no upload table.  The
 * workspace query is monotone and a multiple of 256.
 * Not provided: a selection that continues across calls (an entry that ends in the next piece can beat one
 * chosen here: select over whole texts; d_info[1] shows the entries lost at the front); leftmost-first
 * (priority) selection; sequence or rule records as input (they carry no start). */
size_t acm_select_workspace_bytes(size_t max_records);
int acm_select_matches_async(const acm_dfa *, const int32_t *d_pat_plane,
    const int32_t *d_off_plane, size_t max_records, long min_start, unsigned flags,
    int32_t *d_pat_out, int32_t *d_off_out, int32_t *d_start_out, size_t out_capacity,
    int32_t *d_info, void *d_workspace, size_t workspace_bytes, void *stream);

/* Match rewriting on the device: the text and the selected matches in, the text with every match replaced
 * (acm_automaton_set_replacement: replaced, masked or deleted) out.  What a redactor or a normaliser wants,
 * without copying records and text back to splice on the host.
 * Text: the scan's contract (16-byte aligned, readable up to n rounded up to 16, n <= 2^31 - 17); d_text[i] is
 * the byte at offset text_origin + i, text_end = text_origin + n, as in acm_line_index_async.  text_origin
 * lies in [INT32_MIN, INT32_MAX].
 * Input records: the pattern and offset planes acm_select_matches_async wrote: spans disjoint and ascending.
 * At most min([0], max_records) records are looked at.  The span [s, e] of a record is the select pass's
 * (int64).  A record is USED iff its cell is a pattern index, L >= 1 and text_origin <= s <= e < text_end;
 * any other record is skipped and counted.  Spans that overlap or descend (planes that did not come from
 * select) give unspecified output bytes, nothing worse.
 * Output: the text with every used span replaced by its pattern's replacement (a pattern without one: the
 * span as it is), m bytes (int64).  d_out receives the first min(m, out_capacity) bytes; no byte of d_out at
 * or behind min(m, out_capacity) is written.  d_out == NULL with out_capacity == 0 is legal: only d_info,
 * d_at_out and d_seg_out are produced.  d_out is 16-byte aligned and overlaps neither the text nor the planes.
 *   d_at_out     may be NULL (not wanted), else the scan's cell layout and overflow contract over at_capacity
 *                cells: [0] the used records, then for each used record, in input order, the output offset
 *                (from 0, saturated to INT32_MAX) at which its replacement begins, then a trailer cell 0
 *   d_seg_out    with d_seg_start, both or neither (segments == 0): int32[segments]; for each start x the output
 *                offset of the first output byte that comes from an offset >= x: clamp(x, text_origin,
 *                text_end) - text_origin + the sum over the used records with s < x of (replacement length -
 *                span length), saturated to int32.  Where each packed text begins after the rewrite.
 *   d_info       int32[8], required, written whole: [0] used records, [1] skipped records, [2..3] m as (lo,
 *                hi), [4..5] the input bytes inside used spans (lo, hi), [6] 1 iff m > out_capacity and d_out
 *                is not NULL (the output was cut: never silently), [7] 0
 * An uploaded set without replacements is legal: the output equals the text.  Results are the same bytes on
 * every run (no order decided by atomics).  Whatever the planes hold, no read leaves the inputs and the
 * library's tables and no write leaves the outputs and the workspace.  Stream-ordered, no host sync, no
 * allocation, no host read of device data; argument errors (a NULL text with n > 0, NULL planes or d_info, a
 * misaligned d_text or d_out, n or out_capacity over 2^31 - 17, d_out == NULL with out_capacity > 0,
 * at_capacity < 2 with d_at_out, segments without both arrays, text_origin out of range, a short workspace)
 * return ACM_ERR_ARG before anything is enqueued.
 * Two launches over max_records cells give every used record its place in the output (64-bit sums), one
 * more the segment offsets, and the copy kernel runs on a grid over out_capacity: a workgroup owns 16 KiB of
 * OUTPUT, finds the records that put a byte into it by a search on the records' output ends, and streams
 * everything between them in 16-byte pieces (csrc/rewrite.hip).  The launch count and the grids depend on
 * max_records, segments and out_capacity only -- m lives on the device -- and tiles behind m leave at once:
 * size out_capacity to what is expected, not to the worst case.  The workspace query is monotone in both
 * arguments and a multiple of 256.
 * Not provided: rewriting in place; a rewrite that continues across calls (rewrite whole texts);
 * replacements that refer to the matched bytes; sequence or rule records as input (they carry no start). */
size_t acm_rewrite_workspace_bytes(size_t max_records, size_t segments);
int acm_rewrite_async(const acm_dfa *, const void *d_text, size_t n, long text_origin,
    const int32_t *d_pat_plane, const int32_t *d_off_plane, size_t max_records, void *d_out,
    size_t out_capacity, int32_t *d_at_out, size_t at_capacity, const int32_t *d_seg_start,
    size_t segments, int32_t *d_seg_out, int32_t *d_info, void *d_workspace, size_t workspace_bytes,
    void *stream);

/* Extraction: ranges of a device text gathered into one packed output -- the matching lines, the lines
 * with their context, the matches themselves (grep -o), snippets for a report -- without copying the text
 * and the planes back to slice on the host.  The complement of acm_rewrite_async, which keeps everything.
 * Text: acm_rewrite_async's contract (16-byte aligned, readable up to n rounded up to 16, n <= 2^31 - 17,
 * d_text[i] the byte at offset text_origin + i, text_end = text_origin + n, text_origin in int32).
 * Ranges: both planes in the scan's cell layout; min(max(begin[0], 0), max_ranges) ranges are looked at.
 * Range i is [b, e) with b = begin[1 + i] and e = end[1 + i], or with ACM_EXTRACT_END_INCLUSIVE
 * e = end[1 + i] + 1: the form of the select pass's (d_start_out, d_off_out) for patterns without a post
 * context (int64).  The planes may be acm_line_context_async's (begin, next), acm_line_select_async's, or
 * the select pass's.  A range is USED iff text_origin <= b < e <= text_end; any other range, garbage
 * cells included, is skipped and counted.  Ranges need not ascend or be disjoint: this is a gather, and
 * the output follows input order.
 * Output, for the used ranges in input order:
 *   glue         in front of every used range except the first and except one whose text id differs from
 *                the previous used range's.  The text id is the number of cells of d_seg_start that are
 *                <= b (0 without segments): glue never joins two texts.  glue is HOST memory of glue_len
 *                bytes, 0..ACM_EXTRACT_MAX_GLUE, passed to the kernels by value (no upload)
 *   the bytes    of the range
 *   terminator   (0..255; -1: none) iff the range's last byte is not that byte: grep supplies a missing
 *                final newline this way
 * m (int64) is the output's length.  d_out receives the first min(m, out_capacity) bytes; no byte at or
 * behind that point is written.  d_out == NULL with out_capacity == 0 is legal: the figures only.  d_out
 * is 16-byte aligned, out_capacity <= 2^31 - 17, and it overlaps neither the text nor the planes.
 *   d_at_out     may be NULL, else the scan's cell layout and overflow contract over at_capacity cells:
 *                [0] the used ranges, then per used range the output offset where its bytes begin (behind
 *                its glue; saturated to INT32_MAX), then a trailer cell 0
 *   d_seg_out    with d_seg_start, both or neither: int32[segments]; cell k = the sum, over the used
 *                ranges with b < start[k], of everything those ranges put into the output (glue, bytes,
 *                terminator), saturated to int32.  For ascending ranges: where text k's part begins
 *   d_info       int32[8], required, written whole: [0] used ranges, [1] skipped ranges, [2..3] m as (lo,
 *                hi), [4..5] the text bytes copied (lo, hi), [6] 1 iff m > out_capacity and d_out is not
 *                NULL (the output was cut: never silently), [7] the terminators appended (saturated)
 * Every run gives the same bytes (no order is decided by atomics).  Whatever the planes hold, no read
 * leaves the inputs and no write leaves the outputs and the workspace.  Stream-ordered, no host sync, no
 * allocation, no host read of device data; argument errors (acm_rewrite_async's list; unknown flag bits,
 * glue_len outside 0..ACM_EXTRACT_MAX_GLUE, a NULL glue with glue_len > 0, a terminator outside -1..255)
 * return ACM_ERR_ARG before anything is enqueued.
 * Two launches over max_ranges cells give every used range its end in the output (64-bit sums; the "used
 * range in front" that decides the glue is a prefix maximum), two more the segment sums, and the copy
 * kernel runs on a grid over out_capacity: a workgroup owns 16 KiB of OUTPUT, finds its ranges by a search
 * on the output ends, stages the tile in LDS -- a 16-byte aligned source piece per lane, shifted in
 * registers to its place -- and streams it out in aligned 16-byte stores; a tile inside one range's
 * bytes is copied straight (csrc/range_pack.h).  The launch count and the grids depend on max_ranges,
 * segments and out_capacity only -- m lives on the device -- and tiles behind min(m, out_capacity) leave
 * at once.  The workspace query is monotone in both arguments and a multiple of 256.
 * Not provided: extraction continued across calls (a range is used whole or not at all: give whole texts);
 * lines cut at a text start that is not a line start; per-line prefixes (file:line:) in the output: that is
 * acm_format_async below; wildcard post contexts in the END_INCLUSIVE (-o) form: such a match ends post bytes behind the offset. */
enum { ACM_EXTRACT_END_INCLUSIVE = 1 };
#define ACM_EXTRACT_MAX_GLUE 16
size_t acm_extract_workspace_bytes(size_t max_ranges, size_t segments);
int acm_extract_async(const void *d_text, size_t n, long text_origin,
    const int32_t *d_begin_plane, const int32_t *d_end_plane, size_t max_ranges, unsigned flags,
    const uint8_t *glue, int glue_len, int terminator,
    void *d_out, size_t out_capacity, int32_t *d_at_out, size_t at_capacity,
    const int32_t *d_seg_start, size_t segments, int32_t *d_seg_out,
    int32_t *d_info, void *d_workspace, size_t workspace_bytes, void *stream);

/* Formatting extract: acm_extract_async with a generated prefix in front of every range's bytes -- grep's
 * `name:12:345:` in front of a selected line and `name-11-330-` in front of a context line (-H -n -b), or in
 * front of every match (-o).  The text, the ranges, USED and skipped, ACM_EXTRACT_END_INCLUSIVE, the
 * terminator, d_out / out_capacity, d_at_out, d_seg_start / d_seg_out, d_info[8], the robustness and the
 * argument errors are acm_extract_async's, word for word; d_at_out still holds where a range's BYTES begin,
 * behind its glue and its prefix, and everything a range puts into the output counts in m and d_seg_out.
 * The text id t of a range is the extract's: the cells of d_seg_start that are <= b, 0..segments.
 * More inputs:
 *   d_kind_plane  int32, the scan's cell layout (cell 1 + i belongs to range i); may be NULL.  Bit 0
 *                 (ACM_LINE_SELECTED) chooses the separator, bit 1 (ACM_LINE_GROUP_HEAD) asks for the glue;
 *                 bits above bit 1 are ignored.  NULL: every range is SELECTED and none is a head.
 *                 acm_line_context_lines_async's d_kind_out is such a plane
 *   d_num_plane   int32, cell layout; required iff ACM_FORMAT_NUMBER: the number of range i before the bases
 *                 (acm_line_context_lines_async's d_rel_out, or acm_line_number_async's output one cell up)
 *   d_seg_num     int32[segments], may be NULL: what is subtracted from the numbers of text t > 0, cell t - 1
 *                 (acm_line_number_async over d_seg_start: the lines in front of each text)
 *   number_base, offset_base   0..10^18 each, else ACM_ERR_ARG (1 and 0 for grep)
 *   sel_sep, ctx_sep   0..255: the byte behind every part of the prefix of a SELECTED / of another range
 *   d_names, d_name_off, names_bytes   the name of text id t is d_names[off[t], off[t + 1]), d_name_off being
 *                 int32[segments + 2].  A name whose two cells descend, leave [0, names_bytes] or lie more
 *                 than ACM_FORMAT_MAX_NAME bytes apart is empty: no read leaves the table, whatever it holds.
 *                 names_bytes <= 2^31 - 1
 *   flags         ACM_EXTRACT_END_INCLUSIVE | ACM_FORMAT_NAME | ACM_FORMAT_NUMBER | ACM_FORMAT_OFFSET; unknown
 *                 bits, ACM_FORMAT_NAME without both name arrays, ACM_FORMAT_NUMBER without d_num_plane and a
 *                 separator outside 0..255 return ACM_ERR_ARG before anything is enqueued
 * Output, for every used range in input order:
 *   glue         iff the range's HEAD bit is set and a used range of the same text id lies in front (the last
 *                used range in front decides; skipped cells in between do not matter)
 *   prefix       with sep = sel_sep if the range is SELECTED, else ctx_sep:
 *                  ACM_FORMAT_NAME    the name of t, then sep
 *                  ACM_FORMAT_NUMBER  number_base + num[i] - (t > 0 && d_seg_num ? d_seg_num[t - 1] : 0), then sep
 *                  ACM_FORMAT_OFFSET  offset_base + b - (t > 0 ? d_seg_start[t - 1] : text_origin), then sep
 *                both values in int64, a negative one prints as 0; decimal, no sign, no padding, at least one digit
 *   the bytes, the terminator   as in the extract
 * With flags == 0 and d_kind_plane == NULL this is acm_extract_async with glue_len == 0, whatever glue is
 * given.  With flags == 0, the planes of acm_line_context_lines_async and a glue, the bytes are those of the
 * extract over acm_line_context_async's groups but for terminators inside a group (none when every line
 * keeps its delimiter).
 * Two launches over max_ranges cells place the parts (64-bit sums; a part's size includes its prefix: the
 * name's length and a digit count against the powers of ten), two more give the segment sums, and the copy
 * kernel runs on a grid over out_capacity: a workgroup owns 16 KiB of OUTPUT, finds its ranges by a search on
 * the output ends and stages the tile in LDS: a thread per range writes glue, prefix and terminator (a name
 * over 32 bytes is copied by the thread's wave), the bytes go as aligned 16-byte source pieces, a piece a
 * lane, and the tile leaves in aligned 16-byte stores (csrc/range_pack.h, csrc/format.hip).  The launch count
 * and the grids depend on max_ranges, segments and out_capacity only.  Every run gives the same bytes.  The workspace
 * query is monotone in both arguments and a multiple of 256.
 * Not provided: prefixes continued across calls (the caller carries the bases); "--" between two texts (glue
 * never joins texts; grep prints one there); padded or aligned numbers (grep -T); lines cut at a text start
 * that is not a line start; wildcard post contexts in the END_INCLUSIVE form. */
enum { ACM_FORMAT_NAME = 2, ACM_FORMAT_NUMBER = 4, ACM_FORMAT_OFFSET = 8 };
#define ACM_FORMAT_MAX_NAME 4096
size_t acm_format_workspace_bytes(size_t max_ranges, size_t segments);
int acm_format_async(const void *d_text, size_t n, long text_origin,
    const int32_t *d_begin_plane, const int32_t *d_end_plane, size_t max_ranges, unsigned flags,
    const int32_t *d_kind_plane, const int32_t *d_num_plane, const int32_t *d_seg_num,
    long number_base, long offset_base, int sel_sep, int ctx_sep,
    const uint8_t *d_names, const int32_t *d_name_off, size_t names_bytes,
    const uint8_t *glue, int glue_len, int terminator,
    void *d_out, size_t out_capacity, int32_t *d_at_out, size_t at_capacity,
    const int32_t *d_seg_start, size_t segments, int32_t *d_seg_out,
    int32_t *d_info, void *d_workspace, size_t workspace_bytes, void *stream);

/* Match tallies: counts of the records of any pass, reduced on the device, so a caller who only counts
 * (a classifier, grep -c, "which signatures hit which file") copies back the counts, not the records.
 * Input: planes in the scan's cell layout; at most min([0], max_records) records are looked at, as in
 * acm_expand_matches_async.  report says what the pattern plane's cells are:
 *   ACM_REPORT_HEAD   pattern indices (a default scan, the segment pass in HEAD form, the word pass,
 *                     acm_expand_matches_async): each record counts once
 *   ACM_REPORT_STATE  final states (a STATE scan, the segment pass in STATE form): each record counts
 *                     once, for the head of the state's match list; with ACM_TALLY_ALL_PATTERNS once for
 *                     every entry of the list (the counts of the expansion, without materialising it).
 *                     ACM_TALLY_ALL_PATTERNS with ACM_REPORT_HEAD is ACM_ERR_ARG.
 * Classes: d_class_of is a device int32[num_patterns], the class of each pattern; NULL is the identity
 * (num_classes must then be the number of patterns).  An entry whose class is negative or >=
 * num_classes is counted nowhere, and so is a cell that is no pattern index or state.  No write leaves
 * the output arrays whatever the planes and the class map hold.
 * Segments (segments == 0: none): d_seg_start as in acm_segment_matches_async.  A record at offset o
 * belongs to the last k with start[k] <= o; one in front of start[0] to no segment (the "lead": it
 * continues a text of an earlier buffer).  The starts are only a grid of attribution: nothing is
 * clamped; for per-text matching run the segment pass first and tally its output.
 * Output:
 *   d_class_total  uint64[num_classes], required: entries per class, the lead included.  Written whole;
 *                  with ACM_TALLY_ACCUMULATE added to what is there (a running total over the buffers
 *                  of a stream, kept on the device)
 *   d_seg_class    (NULL: not wanted; needs segments > 0) int32[segments][num_classes], row-major,
 *                  written whole.  segments * num_classes > 2^31 - 1 is ACM_ERR_LIMIT
 *   d_lead         (NULL: not wanted) int32[num_classes], written whole: the entries of the records in
 *                  front of start[0] (all zero when segments == 0); a streaming caller adds it to the
 *                  last row of its previous buffer
 * Integer sums: exact and the same on every run.  The outputs must not overlap the inputs.  Stream-
 * ordered, no host sync, no allocation, no host read of device data; argument errors return before
 * anything is enqueued.  One launch over the records behind the zero-fills of the outputs (cost per
 * record, not per text byte); the scan kernels are not involved.  The workspace query is monotone in both
 * arguments and a multiple of 256 (the pass keeps no scratch today; the block must still be given). */
enum { ACM_TALLY_ACCUMULATE = 1, ACM_TALLY_ALL_PATTERNS = 2 };
size_t acm_tally_workspace_bytes(size_t max_records, size_t num_classes);
int acm_tally_matches_async(const acm_dfa *, const int32_t *d_pat_plane,
    const int32_t *d_off_plane, size_t max_records, int report, int flags,
    const int32_t *d_class_of, size_t num_classes, const int32_t *d_seg_start, size_t segments,
    uint64_t *d_class_total, int32_t *d_seg_class, int32_t *d_lead, void *d_workspace,
    size_t workspace_bytes, void *stream);

/* Line index: where the lines of a text that is already on the device begin, so that the start array
 * the segment, word and tally passes take (d_seg_start) need not be made on the host.  No acm_dfa is
 * involved.  d_text follows the scan's contract (16-byte aligned, readable up to n rounded up to 16,
 * n <= 2^31 - 17); d_text[i] is the byte at offset text_origin + i, text_end = text_origin + n.
 * delimiter: any byte value 0..255 ('\n' for lines).  The starts, ascending, in the scan's coordinates:
 *   text_origin   if n > 0 and the text begins a line: prev_byte == -1 (start of the stream) or
 *                 prev_byte == delimiter.  With d_prev_info != NULL prev_byte is ignored and the rule
 *                 is taken on the device from the d_info of the index call over the piece in front
 *                 of this one (on the same stream, or complete; as acm_scan_batch.d_init_plane): the
 *                 origin is a start iff that piece's [3] is set.  d_prev_info must not be d_info.
 *   p + 1         for every delimiter at p in [text_origin, text_end) with p + 1 < text_end.  A
 *                 delimiter on the last byte opens the NEXT piece's first line: "a\nb\n" has two lines.
 * Output:
 *   d_line_start  int32[capacity], written whole: the first min(m, capacity) starts, INT32_MAX in
 *                 every cell behind them.  Starts at or beyond text_end are allowed as d_seg_start, so
 *                 the array can be handed on with segments = capacity and nobody reads m on the host.
 *   d_info        int32[8]: [0] m, the full count (m > capacity: overflow, the first capacity starts
 *                 are stored, the scan's contract); [1] delimiters in [text_origin, text_end); [2] 1 if
 *                 the origin is a start; [3] 1 if the next piece's origin is a start (an empty piece
 *                 hands on what it was given); [4..5] uint64 (lo, hi) delimiters of the stream in front
 *                 of text_origin (the previous piece's [4..5] + [1], 0 without d_prev_info); [6..7] 0.
 * n == 0 is legal (m = 0; sentinels and d_info are written).  Bytes in [n, round16(n)) never count.
 * Stream-ordered, no host sync, no allocation, no host read of device data; argument errors (a NULL
 * output, capacity == 0, a misaligned d_text, n over the limit, delimiter outside 0..255, prev_byte
 * outside -1..255, a short workspace) return ACM_ERR_ARG before anything is enqueued.  The workspace
 * query is monotone and a multiple of 256.  Two launches; the text is read once (csrc/lines.hip). */
size_t acm_line_index_workspace_bytes(size_t max_text);
int acm_line_index_async(const void *d_text, size_t n, long text_origin, int delimiter,
    int prev_byte, const int32_t *d_prev_info, int32_t *d_line_start, size_t capacity,
    int32_t *d_info, void *d_workspace, size_t workspace_bytes, void *stream);

/* Delimiters in front of each offset.  For i < min(count, d_count ? max(*d_count, 0) : count):
 * d_line_out[i] = number of delimiters in [text_origin, d_offsets[i]) = k + 1 - info[2], k the index
 * of the last start <= d_offsets[i] (-1: none); cells behind that bound are not written.  The 1-based
 * line number in the stream is 1 + info[4..5] + d_line_out[i]: the caller adds that after the fetch.
 * For a scan's records pass d_offsets = d_off_plane + 1, d_count = d_off_plane, count = max_records;
 * for arbitrary offsets d_count = NULL.  Offsets need not be sorted (a binary search each).  Only
 * offsets in [text_origin, text_end) are guaranteed, and only when info[0] <= capacity. */
int acm_line_number_async(const int32_t *d_line_start, size_t capacity, const int32_t *d_info,
    const int32_t *d_offsets, const int32_t *d_count, size_t count, int32_t *d_line_out,
    void *stream);

/* The lines that hold a record (invert != 0: the lines that hold none).  The lines of the piece: the
 * lead [text_origin, start[0]) if the origin is not a start and the piece is not empty, then
 * [start[k], start[k + 1]) for k < m; the last line ends at text_end.  A line keeps its delimiter.  A
 * record belongs to the line that holds its offset (the tally's rule); only d_off_plane is read (at
 * most min([0], max_records) records), so any pass's planes can be given.  Output, the scan's cell
 * layout and overflow contract in all three planes ([0] = full count, entries ascending, trailer cell
 * at min(count + 1, out_capacity - 1) = 0): per entry d_rel_out = delimiters in front of the line
 * (what acm_line_number_async gives for its first byte), d_begin_out and d_next_out = its first byte
 * and the first byte behind it.  Exact when info[0] <= capacity.  Stream-ordered, no host sync, no
 * allocation; cost per record and per line, never per text byte. */
size_t acm_line_select_workspace_bytes(size_t capacity);
int acm_line_select_async(const int32_t *d_line_start, size_t capacity, const int32_t *d_info,
    long text_origin, long text_end, const int32_t *d_off_plane, size_t max_records, int invert,
    int32_t *d_rel_out, int32_t *d_begin_out, int32_t *d_next_out, size_t out_capacity,
    void *d_workspace, size_t workspace_bytes, void *stream);

/* The selected lines with the lines around them, as groups: grep -A/-B/-C.  The lines of the piece and
 * which of them are SELECTED are exactly acm_line_select_async's: the lead line, the starts, invert, a
 * record belonging to the line that holds its offset.
 * Text id: t(j) of line j is the number of cells of d_seg_start[0, segments) that are <= the line's first
 * byte (0 when segments == 0; d_seg_start non-decreasing, as in the tally pass; starts at or beyond
 * text_end are allowed and count for no line).  A line that has a start in its interior belongs to the
 * text it begins in: that happens when a text does not end in the delimiter.
 * KEPT: line j is kept iff some selected line i has t(i) == t(j) and j - after <= i <= j + before (int64:
 * before or after = INT32_MAX means "to the ends of the text"; negative values are ACM_ERR_ARG).
 * GROUP: a maximal run of consecutive kept lines with equal text id.  This is grep's rule: overlapping or
 * adjacent contexts merge, and context never crosses into another text.
 * Output, the scan's cell layout and overflow contract in every plane ([0] = full count of groups,
 * entries ascending, trailer cell at min(count + 1, out_capacity - 1) = 0), per group:
 *   d_rel_out     delimiters in front of the group's first line
 *   d_begin_out   the group's first byte;  d_next_out: the first byte behind it
 *   d_lines_out   the group's lines; may be NULL (not wanted)
 *   d_ctx_info    int32[4], required, written whole: selected lines, kept lines, groups, 0
 * With before == after == 0 and no segments the groups are the runs of adjacent selected lines: the same
 * bytes as acm_line_select_async's entries, which stay one per line.
 * Stream-ordered, no host sync, no allocation; argument errors (a NULL plane but d_lines_out, a NULL
 * d_ctx_info, capacity == 0, out_capacity < 2, text_end < text_origin, a negative before or after,
 * segments without d_seg_start or the reverse, a short workspace) return ACM_ERR_ARG before anything is
 * enqueued.  Exact when info[0] <= capacity.  Six launches behind the zero-fill of the flags, on grids
 * that depend on capacity and max_records only -- never on before, after or the data: a prefix of the
 * selected bits makes "a selected line within the window" one subtraction, and two searches clamp the
 * window to the line's text (csrc/lines.hip).  Cost per record and per line, never per text byte.  The
 * workspace query is monotone in both arguments and a multiple of 256.
 * Not provided: context continued across calls (a group that would reach into the next piece ends at
 * text_end: give whole texts); lines cut at a text start that is not a line start (see the text id). */
size_t acm_line_context_workspace_bytes(size_t capacity, size_t segments);
int acm_line_context_async(const int32_t *d_line_start, size_t capacity, const int32_t *d_info,
    long text_origin, long text_end, const int32_t *d_off_plane, size_t max_records, int invert,
    int before, int after, const int32_t *d_seg_start, size_t segments,
    int32_t *d_rel_out, int32_t *d_begin_out, int32_t *d_next_out, int32_t *d_lines_out,
    size_t out_capacity, int32_t *d_ctx_info, void *d_workspace, size_t workspace_bytes, void *stream);

/* The per-line form of acm_line_context_async: the same inputs, the same line, SELECTED, text id, KEPT and
 * GROUP rules and the same argument errors (d_kind_out in the place of d_lines_out, and required), but one
 * entry per KEPT line instead of one per group, so that every line can get a prefix of its own
 * (acm_format_async).  Output, the scan's cell layout and overflow contract in every plane ([0] = full
 * count of kept lines, entries ascending, trailer cell at min(count + 1, out_capacity - 1) = 0), per line:
 *   d_rel_out     delimiters in front of the line: acm_line_select_async's value, relative to the piece
 *   d_begin_out   the line's first byte;  d_next_out: the first byte behind it
 *   d_kind_out    bit 0 (ACM_LINE_SELECTED) iff the line is selected, bit 1 (ACM_LINE_GROUP_HEAD) iff it is
 *                 the first line of its group
 *   d_ctx_info    int32[4], required, written whole, as in the group form: selected lines, kept lines,
 *                 groups, 0
 * The entries whose HEAD bit is set begin acm_line_context_async's groups over the same input, and a group
 * ends where the next begins.  Five launches behind the zero-fill of the flags -- the group form's first
 * three, one that leaves the kept and the head bits as planes and one ordered write over the kept bits --
 * on grids that depend on capacity and max_records only, never on before, after or the data
 * (csrc/lines.hip).  Stream-ordered, no host sync, no allocation; exact when info[0] <= capacity.  The
 * workspace query is monotone in both arguments and a multiple of 256.  Not provided: as the group form. */
enum { ACM_LINE_SELECTED = 1, ACM_LINE_GROUP_HEAD = 2 };
size_t acm_line_context_lines_workspace_bytes(size_t capacity, size_t segments);
int acm_line_context_lines_async(const int32_t *d_line_start, size_t capacity, const int32_t *d_info,
    long text_origin, long text_end, const int32_t *d_off_plane, size_t max_records, int invert,
    int before, int after, const int32_t *d_seg_start, size_t segments,
    int32_t *d_rel_out, int32_t *d_begin_out, int32_t *d_next_out, int32_t *d_kind_out,
    size_t out_capacity, int32_t *d_ctx_info, void *d_workspace, size_t workspace_bytes, void *stream);

/* Normalised scanning: a stage in front of the scan that makes the text the signatures were written for --
 * percent triples decoded, blanks squeezed or stripped -- and a pass behind it that brings the records back
 * to the bytes the caller has.  The scan and every pass behind it run unchanged on the normalised text.
 * Text: acm_rewrite_async's contract (16-byte aligned, readable up to n rounded up to 16, n <= 2^31 - 17,
 * d_text[i] the byte at offset text_origin + i, text_origin in int32; bytes behind n never influence
 * anything).  With d_seg_start the n bytes are cut into texts as the segment pass cuts them (every start
 * clamped into the text; the bytes in front of the first start are a text of their own); without it they
 * are one text.
 * flags: ACM_NORM_PERCENT, together with at most one of ACM_NORM_SQUEEZE and ACM_NORM_STRIP; 0 is legal (the
 * output is the text).
 *   Units.   With ACM_NORM_PERCENT offset i is a TRIPLE HEAD iff t[i] == '%', i + 2 lies inside i's own text
 *            and t[i+1], t[i+2] are both in [0-9A-Fa-f].  A head and its two digits are a unit of length 3
 *            whose value is the decoded byte; every byte in no triple is a unit of length 1 whose value is
 *            the byte.  Decoding happens once (%2541 gives %41); a '%' whose digits would lie in the next
 *            text or behind n stays literal.  Without the flag every byte is a unit.
 *   Blanks.  A unit is BLANK iff its value is in the blank set: blank_mask, HOST memory of 32 bytes passed by
 *            value (bit b % 8 of byte b / 8: byte b), NULL for {09, 0a, 0b, 0c, 0d, 20}.  With
 *            ACM_NORM_SQUEEZE a blank unit is emitted as blank_byte (0..255) iff it is the first unit of its
 *            text or the unit in front of it in the same text is not blank, else dropped: a run never
 *            continues across a text start.  With ACM_NORM_STRIP every blank unit is dropped.  With neither
 *            no unit is blank.  Every other unit is emitted with its value.
 *   Output.  The emitted bytes in order, m <= n of them.  For output offset o, first(o) = text_origin + the
 *            offset of the emitting unit's first byte and last(o) = first(o) + the unit's length - 1.  A
 *            squeezed run's emitter is its first unit only.
 *   d_out      receives the first min(m, out_capacity) bytes; no byte at or behind that point is written.
 *              d_out == NULL with out_capacity == 0: the figures only.  16-byte aligned; overlaps neither the
 *              text nor the other outputs
 *   d_keep     uint64[ceil(n / 64)], required: bit i % 64 of word i / 64 is set iff byte i emits (it is the
 *              first byte of a unit that is emitted); bits behind n are 0
 *   d_block    int32[ceil(n / ACM_NORM_BLOCK) + 1], required: cell j = the output bytes emitted by the input
 *              in front of byte j * ACM_NORM_BLOCK; the last cell is m.  With d_keep the whole offset map, in
 *              1/8 + 1/256 of the text
 *   d_seg_out  with d_seg_start, both or neither: int32[segments]; cell k = the output bytes emitted by the
 *              input in front of start k (clamped): where text k begins in the output, ready to be the
 *              segment pass's d_seg_start over the normalised text
 *   d_info     int32[8], required, written whole: [0] m, [1] units dropped, [2] triples (emitted or not),
 *              [3] blank units emitted, [4] 1 iff m > out_capacity and d_out is not NULL (never cut
 *              silently), [5..7] 0
 * Every run gives the same bytes (no order is decided by atomics).  No read leaves the inputs and no write
 * leaves the outputs and the workspace.  Stream-ordered, no host sync, no allocation, no host read of device
 * data; argument errors (acm_rewrite_async's list; unknown flag bits, squeeze with strip, blank_byte outside
 * 0..255 under squeeze, a NULL d_keep or d_block) return ACM_ERR_ARG before anything is enqueued.
 * Three launches on a fixed grid: the keep words and per-block counts from one read of the text, the block
 * sums, and a write kernel that owns 16 KiB of INPUT per tile, ranks the kept bytes, stages them in LDS and
 * streams them out in aligned 16-byte stores (csrc/normalize.hip).  With segments a zero-fill and a launch
 * over the starts go in front (a bit per start) and one launch over the starts behind (d_seg_out).  The
 * workspace query is monotone in both arguments and a multiple of 256.
 *
 * acm_normalize_remap_async: one pass over records in the scan's cell layout (the count read from cell 0 of
 * d_off_plane on the device, clamped to max_records), whose offsets are offsets into the normalised text.
 * The text, n, text_origin, flags, d_keep and d_block are the ones the normalise call got and wrote.
 * d_off_out's record is last(off).  With d_pat_plane (pattern indices) and d_start_out, d_start_out's record
 * is first(s), s where the select pass says the match starts (off - length + 1 for a plain pattern).  An
 * offset or start outside [0, m) and a cell that is no pattern index give the cell -1, and such records are
 * counted; whatever the planes hold, nothing is read or written outside.  Cell 0 of each output is the count.
 * d_off_out may equal d_off_plane (its cell 0 then stays what it is). d_info int32[8]: [0] records looked at, [1] records with an unmapped
 * cell, rest 0.  A triple is told from a '%' in front of two literal digits by the digits' keep bits (the
 * remap is not given the text starts).  One case is therefore not exact: under ACM_NORM_STRIP with a blank set
 * that holds hex digits, a literal '%' whose two digits lie across a text start and are both stripped is taken
 * for a triple, and last(off) is then 2 too large.  With the default set, and with any set without hex digits,
 * the remap is exact.
 * ACM_ERR_ARG: a NULL map, plane, output or d_info, d_start_out without d_pat_plane, d_pat_plane without the
 * automaton, bad flags, max_records over 2^31 - 2.  A zero-fill of d_info and one launch, a thread a record.
 *
 * Not provided: normalisation continued across calls (give whole texts); repeated decoding, '+' as space,
 * %uXXXX, HTML entities; case folding (the automaton's own nocase does that); lines, extraction, rewriting
 * and position windows over a normalised scan; a scan that takes its length from the device (m lives on the
 * device and acm_scan_async's length is a host argument: a caller reads d_info[0] back once in between). */
enum { ACM_NORM_PERCENT = 1, ACM_NORM_SQUEEZE = 2, ACM_NORM_STRIP = 4 };
#define ACM_NORM_BLOCK 1024
size_t acm_normalize_workspace_bytes(size_t max_text, size_t segments);
int acm_normalize_async(const void *d_text, size_t n, long text_origin, unsigned flags,
    const uint8_t *blank_mask, int blank_byte, void *d_out, size_t out_capacity,
    uint64_t *d_keep, int32_t *d_block, const int32_t *d_seg_start, size_t segments, int32_t *d_seg_out,
    int32_t *d_info, void *d_workspace, size_t workspace_bytes, void *stream);
int acm_normalize_remap_async(const acm_dfa *, const void *d_text, size_t n, long text_origin,
    unsigned flags, const uint64_t *d_keep, const int32_t *d_block, const int32_t *d_pat_plane,
    const int32_t *d_off_plane, size_t max_records, int32_t *d_off_out, int32_t *d_start_out,
    int32_t *d_info, void *stream);

int acm_scan_batch_async(const acm_dfa *, const acm_scan_batch *);

/* count batches with one call, enqueued in array order: what a worker pool
 * issues per round, without a trip through the FFI per batch.  Stops at the
 * first batch that fails and returns its status (the batches before it stay
 * enqueued).
 *
 * Grouping: consecutive batches that take the sparse pipeline, have the same
 * stream and size, each its OWN workspace and planes and no events, are
 * enqueued up to acm_scan_set_max_group() at a time as ONE set
 * of three launches -- the kernels' fixed costs (launch, filter fill, the
 * check kernel's chains of dependent loads) are paid per group instead of per
 * batch.  Results are those of enqueueing the batches one by one; they become
 * visible in stream order when the group's last kernel has run.  Batches that
 * share a workspace are never grouped. */
int acm_scan_batches_async(const acm_dfa *, const acm_scan_batch *batches, size_t count);
/* batches per group, 1 (never group) .. 16 (the default).  Returns the value in use;
 * 0 or negative only queries. */
int acm_scan_set_max_group(acm_dfa *, int batches);

/* independent chains each lane interleaves in the walk kernel: 2 or 4.
 * Returns the value in use. */
int acm_scan_set_chains_per_lane(acm_dfa *, int chains);

/* number of kernels the chain pipeline enqueues for a non-empty text of up to
 * 64 MiB (one more above that) */
int acm_scan_kernel_count(void);

/* A scan whose arguments repeat (same text buffer, size, workspace, planes,
 * init_state ... -- a worker cycling through its staging buffers) is captured
 * into a HIP graph the second time it is seen and replayed from then on: one
 * hipGraphLaunch instead of a row of kernel launches.  Off by default (on
 * MI355X / ROCm 7.2 it saves a few microseconds of host time per scan and
 * nothing on the GPU); never used with the NULL stream, profiling or the
 * event fields of acm_scan_batch.  enable = 0 / 1, -1 only queries.  Returns
 * the setting in use. */
int acm_scan_set_graphs(acm_dfa *, int enable);
/* What the graph path has done since acm_dfa_upload: captured = graphs
 * instantiated (one per key seen twice, one more each time an evicted key comes
 * back or two threads capture the same key at once), launched = hipGraphLaunch
 * calls issued.  A key's first enqueue is plain, its second captures and
 * launches, later ones only launch: R enqueues of one key give captured 1,
 * launched R - 1.  Scans the graph path leaves out (NULL stream, profiling,
 * event fields, n == 0, graphs off) move neither.  Either pointer may be NULL.
 * ACM_ERR_ARG for a NULL dfa. */
int acm_scan_graph_stats(const acm_dfa *, uint64_t *captured, uint64_t *launched);

/* Which pipeline acm_scan_*_async runs.  Both produce the same planes.
 *   CHAIN   speculative chains (any pattern set)
 *   SPARSE  strided 3-gram sieve + exact checks + trie-path followers; needs
 *           every pattern to have at least 3 bytes (otherwise CHAIN is used).
 *           Exact on any text, three launches, no fallback; slow on a text
 *           that is dense in matches
 *   AUTO    SPARSE when the pattern set allows it -- adaptively: when half of
 *           the last 16 sparse batches held more than a record per 128 bytes
 *           or more than a flagged sample per 48 (the worst of real binaries) the next 64
 *           go to the chain pipeline; then the sparse one is tried again, 4
 *           batches at a time, and every bad look quadruples the chain
 *           pipeline's share (up to 4096 batches)
 * Returns the mode in use after the call; acm_scan_mode(d, -1) only queries. */
enum { ACM_SCAN_MODE_AUTO = 0, ACM_SCAN_MODE_CHAIN = 1, ACM_SCAN_MODE_SPARSE = 2 };
int acm_scan_set_mode(acm_dfa *, int mode);
/* 1 when the pattern set qualifies for the sparse pipeline */
int acm_scan_sparse_eligible(const acm_dfa *);
/* 1 when the chain pipeline walks this set with the whole automaton in LDS (csrc/lds_walk.hip: small
 * alphabet, at most 16384 states, patterns of at most 33 bytes); 0: hot rows in LDS + cold plane in HBM */
int acm_scan_lds_resident(const acm_dfa *);
/* 1 when consecutive batches of one size handed to acm_scan_batches_async can share their kernel
 * launches in the current mode: the sparse pipeline's batches, and the chain pipeline's when the
 * automaton is LDS-resident */
int acm_scan_group_capable(const acm_dfa *);
/* after a scan of n bytes with this workspace has been enqueued on stream:
 * waits for the stream and says which pipeline produced the planes --
 * ACM_SCAN_MODE_CHAIN or ACM_SCAN_MODE_SPARSE (0xDEAD: the sparse kernels found
 * their own workspace inconsistent and wrote empty planes; cannot happen) */
int acm_scan_path_taken(const acm_dfa *, const void *d_workspace, size_t n, void *stream);

/* in-line timing with HIP events on the launch stream: when enabled, every
 * acm_scan_async records an event before its first kernel, after its first
 * kernel (chain: the walk; sparse: the bulk kernel k_sieve) and after its
 * last.
 * acm_scan_profile_read waits for the recorded events, returns the summed
 * milliseconds of the first kernel, the second, and the whole pipeline over
 * 'launches' calls, and resets the accumulation.  (Sparse pipeline: first =
 * the bulk kernel k_sieve, second = check + emit.)  Safe to use while other
 * threads enqueue scans on other streams. */
int acm_scan_profile_enable(acm_dfa *, int enable);
int acm_scan_profile_read(acm_dfa *, double *first_ms, double *second_ms,
    double *pipeline_ms, int *launches);

/* ---------------------------------------------------------------------- */
/* standalone result post-processing ops (device pointers, async)          */
/* ---------------------------------------------------------------------- */

/* exclusive int32 prefix sum (work-efficient Blelloch up/down sweep in LDS,
 * recursive over block sums).  Replaces ocl_prefix_sum.c:164-221 +
 * scan_kernel.cl.  d_in may equal d_out.  d_total (optional) gets the sum. */
size_t acm_exclusive_scan_workspace_bytes(size_t n);
int acm_exclusive_scan_i32(const int32_t *d_in, int32_t *d_out, size_t n,
    int32_t *d_total, void *d_workspace, size_t workspace_bytes, void *stream);

/* bucket planes -> dense array; compactarray.cl:40-68 cell for cell:
 * dst[0]=total, dst[1..]=cells, dst[total+1]=src[max_results*len] */
int acm_compact_buckets(int32_t *d_dst, const int32_t *d_src,
    const int32_t *d_prefix, int len, int max_results, void *stream);

/* key/value bitonic sort on uint32 keys, same network as BitonicSort.cl
 * (tie order included); len must be a power of two; returns 0, or -1 for an
 * unsupported length like ocl_bitonic_sort.c:154-165.  src may equal dst. */
int acm_bitonic_sort_u32(uint32_t *d_key_dst, uint32_t *d_val_dst,
    const uint32_t *d_key_src, const uint32_t *d_val_src, unsigned batch,
    unsigned len, unsigned dir, void *stream);

/* compact planes (position ordered) -> the reference's bucket planes
 * results/results2 [max_results][chunks] + trailer (ahomatch.cl:63-75,
 * :90-93, :160-162 layout; databuf.c:747-782 reads it).  plane_capacity =
 * cells of the compact planes: a plane whose count exceeds plane_capacity - 2
 * holds the first plane_capacity - 2 records and its trailer in the last cell. */
int acm_bucketize(const int32_t *d_pat_plane, const int32_t *d_off_plane,
    const int32_t *d_indices, const int32_t *d_sizes, int chunks,
    int max_results, int32_t *d_results, int32_t *d_results2,
    size_t plane_capacity, void *stream);

/* chunk list -> contiguous stream and back.  The reference scans chunk by
 * chunk (indices[]/sizes[], databuf.c:326-481) and chunks may be separated by
 * zero padding; acm_pack_chunks copies chunk i to d_dst + d_packed_start[i],
 * acm_remap_offsets rewrites the offsets of a compact plane (scanned over the
 * packed stream) into offsets of the original buffer.  max_records bounds
 * the launch and the records touched (at most plane capacity - 2); the
 * record count is read from d_off_plane[0] on the device. */
int acm_pack_chunks(void *d_dst, const void *d_src, const int32_t *d_indices,
    const int32_t *d_sizes, const int32_t *d_packed_start, int chunks,
    void *stream);
int acm_remap_offsets(int32_t *d_off_plane, size_t max_records,
    const int32_t *d_indices, const int32_t *d_packed_start, int chunks,
    void *stream);

/* ---------------------------------------------------------------------- */
/* multi-GPU: shard plan and the gather of the match planes                */
/* (new functionality: the reference takes one -D, ocl_aho_grep.c:498-502) */
/* ---------------------------------------------------------------------- */

/* One process (or thread) per device.  The text is cut by range: rank g of
 * 'world' owns [begin, end) of the n bytes, loads load_bytes from load_begin
 * on (its range and, in front of it, a halo of max_pattern_len - 1 bytes) and
 * scans them with acm_scan_shard_async(halo, offset_shift): the records it
 * reports are the serial scan's records that end in its range, with offsets
 * in the coordinates of the whole text.  The DFA is replicated; nothing is
 * exchanged during the scan. */
typedef struct acm_shard_plan {
	size_t begin, end;	/* the rank's share of the text              */
	size_t halo;		/* context bytes in front of it               */
	size_t load_begin;	/* first byte the rank reads (begin - halo)   */
	size_t load_bytes;	/* bytes it scans, halo included              */
	long offset_shift;	/* local offset + shift = offset in the text  */
} acm_shard_plan;
int acm_shard_plan_for(size_t n, int world, int rank, int max_pattern_len,
    acm_shard_plan *out);

/* The one exchange: every rank's compact planes (plane_capacity cells each)
 * go to 'root' over RCCL -- nccl_comm is the caller's ncclComm_t; the sends and
 * receives form one group on 'stream', point to point, nothing is
 * synchronised.  On the root d_all_pat / d_all_off receive them rank-major,
 * [world][plane_capacity]; other ranks may pass NULL.  librccl.so is loaded on
 * first use. */
int acm_gather_planes(void *nccl_comm, int rank, int world, int root,
    const int32_t *d_pat_plane, const int32_t *d_off_plane,
    size_t plane_capacity, int32_t *d_all_pat, int32_t *d_all_off,
    void *stream);

/* The same with sized messages: an all-gather of the ranks' record
 * counts (the header cells), then count + 2 cells of each plane per rank instead
 * of plane_capacity -- 7 MB instead of 2 x 8 MB for the sentiment planes.  The
 * counts are on the device: the call waits on 'stream' once, for 4 * world
 * bytes, between the two steps.  d_counts: int32[world] device scratch on every
 * rank; counts_out: host int32[world] or NULL.  A rank whose count exceeds
 * plane_capacity - 2 sends plane_capacity cells; acm_merge_planes then returns
 * ACM_ERR_CAPACITY for it (the single-GPU contract reports such an overflow
 * through the count in the header cell: the merge has no room for the records). */
int acm_gather_planes_sized(void *nccl_comm, int rank, int world, int root,
    const int32_t *d_pat_plane, const int32_t *d_off_plane,
    size_t plane_capacity, int32_t *d_all_pat, int32_t *d_all_off,
    int32_t *d_counts, int32_t *counts_out, void *stream);

/* Host side of the root, after the gather has been copied back: rank order
 * is position order, so the ranks' records back to back are the text's
 * ordered list.  Writes them to pat_out / off_out (either may be NULL to only
 * count), returns how many there are or an error; *last_state = the final
 * state of the last rank's shard = the text's. */
long acm_merge_planes(const int32_t *all_pat, const int32_t *all_off,
    int world, size_t plane_capacity, int32_t *pat_out, int32_t *off_out,
    size_t out_capacity, long *last_state);

/* ---------------------------------------------------------------------- */
/* device-runtime helpers for FFI hosts without a HIP binding              */
/* ---------------------------------------------------------------------- */
int acm_rt_set_device(int device);
int acm_rt_malloc(void **out, size_t bytes);
int acm_rt_free(void *p);
int acm_rt_host_alloc(void **out, size_t bytes);	/* pinned */
int acm_rt_host_free(void *p);
int acm_rt_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
int acm_rt_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);
int acm_rt_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream);
int acm_rt_memset(void *dst, int value, size_t bytes, void *stream);
int acm_rt_stream_create(void **out);
int acm_rt_stream_destroy(void *stream);
int acm_rt_stream_sync(void *stream);
int acm_rt_device_sync(void);
int acm_rt_event_create(void **out);
int acm_rt_event_destroy(void *ev);
int acm_rt_event_record(void *ev, void *stream);
int acm_rt_event_sync(void *ev);
int acm_rt_event_elapsed_ms(void *start, void *stop, float *ms);
int acm_rt_device_info(int device, char *name, int name_cap, int *cus,
    size_t *mem_bytes, int *lds_per_cu);

/* ====================================================================== */
/* (2) the reference's interface                                           */
/* ====================================================================== */

/* OpenCL handle names, declared exactly as <CL/cl.h> does so that a caller
 * that also includes the Khronos headers sees compatible typedefs. */
#ifndef __OPENCL_CL_H
typedef struct _cl_platform_id *cl_platform_id;
typedef struct _cl_device_id *cl_device_id;
typedef struct _cl_context *cl_context;
typedef struct _cl_command_queue *cl_command_queue;
typedef struct _cl_mem *cl_mem;
typedef struct _cl_program *cl_program;
typedef struct _cl_kernel *cl_kernel;
typedef uint64_t cl_device_type;
#endif

/* ---- ocl_context.h:8-38 ------------------------------------------------ */
struct clconf {
	cl_platform_id platform;
	cl_device_id dev;
	cl_context ctx;		/* per-device context of this library      */
	cl_command_queue queue;	/* a hipStream_t                           */

	cl_program program_aho_match;	/* unused: code objects are embedded */
	cl_kernel kernel_aho_match;
	cl_program program_prefixsum;
	cl_kernel kernel_prescan;
	cl_kernel kernel_prescan_store_sum;
	cl_kernel kernel_prescan_store_sum_non_power_of_two;
	cl_kernel kernel_prescan_non_power_of_two;
	cl_kernel kernel_uniform_add;
	cl_program program_compact_array;
	cl_kernel kernel_compact_array;

	cl_device_type type;
};

/* pick the pos-th device, create context + in-order queue
 * (ocl_context.c:18-85; subpos is ignored there too) */
void clinitctx(struct clconf *, int pos, int subpos);

/* ---- acsmx.h:44-196 ---------------------------------------------------- */
#define ALPHABET_SIZE 256
#define ACSM_FAIL_STATE -1

struct _acsm_pattern {
	struct _acsm_pattern *next;
	unsigned char *pattern;
	unsigned char *casepattern;
	int n;
	int nocase;
	int offset;
	int depth;
	void *id;
	int iid;
	unsigned int index;
};
typedef struct _acsm_pattern acsm_pattern_t;

struct _acsm_state_table {	/* kept for source compatibility; unused */
	int next_state[ALPHABET_SIZE];
	int fail_state;
	int num_finals;
	acsm_pattern_t *match_list;
};
typedef struct _acsm_state_table acsm_state_table_t;

struct _acsm {
	int max_states;
	int num_states;
	int max_pattern_len;
	size_t size;
	acsm_pattern_t *patterns;	/* always NULL here: see 'native'   */
	int num_patterns;
	acsm_state_table_t *state_table;	/* always NULL              */
	int *h_trans;			/* NULL: no host copy is kept       */
	cl_mem d_trans;			/* device table (cold plane)        */
	acm_automaton *native;		/* host automaton                   */
	acm_dfa *dfa;			/* device DFA after gen_state_table */
};
typedef struct _acsm acsm_t;

acsm_t *acsm_new(void);						/* acsmx.h:101 */
void acsm_add_pattern(acsm_t *, unsigned char *, int n, int nocase,
    int offset, int depth, void *id, int iid);			/* :118 */
void acsm_compile(acsm_t *);					/* :127 */
void acsm_gen_state_table(acsm_t *, int mapped, cl_context,
    cl_command_queue);						/* :139 */
acsm_pattern_t *acsm_get_patterns_table(acsm_t *);		/* :152 */
int acsm_get_max_pattern_size(acsm_t *);			/* :162 */
int acsm_get_states(acsm_t *);					/* :172 */
size_t acsm_get_size(acsm_t *);					/* :182 */
void acsm_cleanup(acsm_t *);					/* :191 */
void acsm_free(acsm_t *);					/* :200 */

/* ---- databuf.h:9-174 --------------------------------------------------- */
#define MAX_RESULTS 16

struct databuf {
	unsigned char *h_data;
	int *h_indices;
	int *h_sizes;
	int *h_results;
	int *h_results2;
	int *h_prefixsum;
	int *h_results_comp;
	int *h_results2_comp;

	size_t results_comp_size;
	size_t results2_comp_size;

	int *file_ids;
	int mapped;
	int max_results;
	long last_state;
	size_t max_chunks;
	size_t max_chunk_size;
	size_t size;
	size_t chunks;
	size_t bytes;

	cl_mem d_data;
	cl_mem d_indices;
	cl_mem d_sizes;
	cl_mem d_results;
	cl_mem d_results2;
	cl_mem d_prefixsum;
	cl_mem d_results_comp;
	cl_mem d_results2_comp;

	cl_mem p_data;		/* pinned twins: the h_* arrays ARE pinned, */
	cl_mem p_indices;	/* these stay NULL                          */
	cl_mem p_sizes;
	cl_mem p_results;
	cl_mem p_results2;
	cl_mem p_prefixsum;
	cl_mem p_results_comp;
	cl_mem p_results2_comp;

	cl_mem *ScanPartialSums;	/* unused: scan scratch is in 'ws'  */
	unsigned int ScanPartialSums_size;

	struct clconf *cl;

	/* additions of this library */
	void *ws;		/* device scratch of the scan pipeline      */
	size_t ws_bytes;
	int compact;		/* 1: process_results reads the compact
				 * planes (the reference's COMPACT_RESULTS
				 * build, databuf.c:16); 0: bucket planes   */
	int scanned;		/* planes on the device are current         */
	void *pack_text;	/* device copy of a padded chunk list packed */
	size_t pack_text_cap;	/* into one stream (ocl_aho_match), and the  */
	int *pack_starts;	/* packed start of each chunk: device array  */
	int *h_pack_starts;	/* and its pinned host twin                  */
	size_t pack_starts_cap;
};

struct databuf *databuf_new(size_t max_chunks, size_t max_chunk_size,
    int max_results, int mapped, struct clconf *);	/* databuf.h:79 */
int databuf_add_fd(struct databuf *, int fd, int id, size_t *rd_bytes);
int databuf_add_fp(struct databuf *, FILE *, int id, int aligned,
    size_t *rd_bytes, size_t *rd_lines);
int databuf_add_chunk(struct databuf *, char *chunk, size_t len, int id,
    char aligned);					/* databuf.c:487 */
void databuf_reset(struct databuf *);
void databuf_clear(struct databuf *);
void databuf_copy_host_to_device(struct databuf *, cl_command_queue);
void databuf_copy_device_to_host(struct databuf *, cl_command_queue);
int databuf_process_results(struct databuf *,
    int (*cb)(int file_idx, int patrn_idx, int chunk_idx, int offset,
    void *uarg), void *uarg);
void databuf_free(struct databuf *, int mapped, cl_command_queue);

/* ---- ocl_aho_match.h:12-30 --------------------------------------------- */
void ocl_aho_match_init(struct clconf *);
void ocl_aho_match_close(struct clconf *);
/* scans db (device copy) and fills the bucket planes AND the compact
 * planes; blocks until done like the reference's clFinish
 * (ocl_aho_match.c:125-130).  'stream' is accepted and ignored (:83-90). */
void ocl_aho_match(struct clconf *, struct databuf *, acsm_t *,
    size_t local_ws, int stream);

/* ---- ocl_prefix_sum.h:12-22, ocl_compact_array.h:12-22 ----------------- */
void ocl_prefix_sum_init(struct clconf *);
void ocl_prefix_sum_close(struct clconf *);
void ocl_prefix_sum(struct clconf *, struct databuf *, unsigned int n);
void ocl_compact_array_init(struct clconf *);
void ocl_compact_array_close(struct clconf *);
void ocl_compact_array(struct clconf *, struct databuf *, size_t local_ws);

/* ---- ocl_bitonic_sort.h:13-18 ------------------------------------------ */
int ocl_bitonic_sort_init(struct clconf *);
int ocl_bitonic_sort_close(struct clconf *);
int ocl_bitonic_sort(struct clconf *, cl_mem key_dst, cl_mem val_dst,
    cl_mem key_src, cl_mem val_src, unsigned int batch, unsigned int len,
    unsigned int dir);

#ifdef __cplusplus
}
#endif
#endif /* ACMATCH_H_ */
