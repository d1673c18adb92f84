// Host-side Aho-Corasick automaton: pattern list -> trie -> fail links ->
// match lists -> device numbering -> dense DFA rows.
//
// Semantics follow the reference's acsmx.c exactly where they are observable
// (state creation order, match-list order, which pattern a final state
// reports); the data structures do not: the trie is sparse (CSR children +
// hash lookup), fail links are computed on the trie, and dense rows are
// generated once, directly in device numbering.
//
//   acsm_add_pattern   acsmx.c:514-546   -> acm_automaton_add
//   add_pattern_states acsmx.c:318-349   -> insert_patterns()
//   build_NFA          acsmx.c:355-438   -> link_and_collect()
//   convert_NFA_to_DFA acsmx.c:444-486   -> dense_rows()
//   acsm_gen_state_table :640-658        -> acm_automaton_export_reference_table
//   acsm_get_patterns_table :677-735     -> chain_patterns()
//   pattern file parser ocl_worker.c:74-145, utils.c:18-54 -> acm_automaton_load_file
#include <algorithm>
#include <cctype>
#include <cerrno>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <new>
#include <unordered_map>

#include "acm_internal.h"
#include "case_fold.h"

namespace acm {

static thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	g_last_error = buf;
	return code;
}

void clear_error() { g_last_error.clear(); }

}  // namespace acm

extern "C" const char *acm_last_error(void) { return acm::g_last_error.c_str(); }

extern "C" const char *acm_strerror(int code)
{
	switch (code) {
	case ACM_OK: return "ok";
	case ACM_ERR_ARG: return "invalid argument";
	case ACM_ERR_NOMEM: return "out of memory";
	case ACM_ERR_HIP: return "HIP runtime error";
	case ACM_ERR_NODEV: return "no usable device";
	case ACM_ERR_LIMIT: return "design limit exceeded";
	case ACM_ERR_IO: return "cannot open file";
	case ACM_ERR_PARSE: return "malformed pattern";
	case ACM_ERR_CAPACITY: return "result planes too small";
	default: return "unknown error";
	}
}

extern "C" const char *acm_version(void) { return "acmatch 0.1 (gfx950, HIP)"; }

// ---------------------------------------------------------------------------

extern "C" acm_automaton *acm_automaton_new(void)
{
	return new (std::nothrow) acm_automaton();
}

extern "C" void acm_automaton_free(acm_automaton *a) { delete a; }

extern "C" int acm_automaton_add(acm_automaton *a, const unsigned char *bytes, int n, int iid)
{
	return acm_automaton_add_ex(a, bytes, n, iid, 0);
}

extern "C" int acm_automaton_add_ex(acm_automaton *a, const unsigned char *bytes, int n, int iid, unsigned flags)
{
	if (!a || n < 0 || (n > 0 && !bytes))
		return acm::fail(ACM_ERR_ARG, "acm_automaton_add: bad arguments");
	if (flags & ~(unsigned)ACM_PATTERN_NOCASE)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_add_ex: unknown flag bits 0x%x", flags & ~(unsigned)ACM_PATTERN_NOCASE);
	if (a->compiled)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_add: automaton already compiled");
	acm_automaton::Pattern p;
	p.bytes.assign(bytes, bytes + n);
	p.iid = iid;
	p.flags = flags;
	a->patterns.push_back(std::move(p));
	if (n > a->max_pattern_len)
		a->max_pattern_len = n;
	return ACM_OK;
}

extern "C" int acm_automaton_set_nocase(acm_automaton *a, int enable)
{
	if (!a)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_set_nocase: null automaton");
	if (a->compiled)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_set_nocase: automaton already compiled");
	a->nocase = a->want_nocase = enable != 0;
	return ACM_OK;
}

extern "C" int acm_automaton_nocase(const acm_automaton *a) { return (a && a->nocase && !a->mixed) ? 1 : 0; }

extern "C" int acm_automaton_mixed_case(const acm_automaton *a) { return (a && a->compiled && a->mixed) ? 1 : 0; }

extern "C" int acm_automaton_pattern_flags(const acm_automaton *a, int index)
{
	if (!a || index < 0 || index >= (int)a->patterns.size())
		return acm::fail(ACM_ERR_ARG, "acm_automaton_pattern_flags: index out of range");
	return (int)a->patterns[index].flags;
}

// ---- position constraints ----------------------------------------------------

extern "C" int acm_automaton_set_position(acm_automaton *a, int index, int32_t lo, int32_t hi, unsigned flags)
{
	if (!a || index < 0 || index >= (int)a->patterns.size())
		return acm::fail(ACM_ERR_ARG, "acm_automaton_set_position: index out of range");
	if (lo < 0 || hi < 0)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_set_position: negative bound (%d, %d)", lo, hi);
	if (flags & ~(unsigned)ACM_POS_FROM_END)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_set_position: unknown flag bits 0x%x", flags & ~(unsigned)ACM_POS_FROM_END);
	acm_automaton::Pattern &p = a->patterns[index];
	p.pos_lo = lo;
	p.pos_hi = hi;
	p.pos_flags = flags;
	return ACM_OK;
}

extern "C" int acm_automaton_pattern_position(const acm_automaton *a, int index, int32_t *lo, int32_t *hi, unsigned *flags)
{
	if (!a || index < 0 || index >= (int)a->patterns.size())
		return acm::fail(ACM_ERR_ARG, "acm_automaton_pattern_position: index out of range");
	const acm_automaton::Pattern &p = a->patterns[index];
	if (lo) *lo = p.pos_lo;
	if (hi) *hi = p.pos_hi;
	if (flags) *flags = p.pos_flags;
	return ACM_OK;
}

extern "C" int acm_automaton_positioned(const acm_automaton *a)
{
	if (a)
		for (auto &p : a->patterns)
			if (p.positioned())
				return 1;
	return 0;
}

// One unsigned decimal field of a position-file line: digits up to a blank or the end, at most INT32_MAX.
static bool pos_field(const char *&s, int32_t &out)
{
	while (*s == ' ' || *s == '\t')
		s++;
	if (!isdigit((unsigned char)*s))
		return false;
	int64_t v = 0;
	for (; isdigit((unsigned char)*s); s++) {
		v = v * 10 + (*s - '0');
		if (v > INT32_MAX)
			return false;
	}
	if (*s && *s != ' ' && *s != '\t')
		return false;
	out = (int32_t)v;
	return true;
}

extern "C" int acm_automaton_load_position_file(acm_automaton *a, const char *path)
{
	if (!a || !path)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_load_position_file: bad arguments");
	FILE *fp = fopen(path, "r");
	if (!fp)
		return acm::fail(ACM_ERR_IO, "cannot open position file '%s': %s", path, strerror(errno));
	struct Line {
		int32_t index, lo, hi;
		unsigned flags;
	};
	std::vector<Line> lines;   // applied only when the whole file has parsed
	std::vector<char> buf(acm::kMaxPatternLine);
	int line_no = 0, rc = ACM_OK;
	while (rc == ACM_OK && fgets(buf.data(), (int)buf.size(), fp)) {
		line_no++;
		std::string line(buf.data());
		while (!line.empty() && (line.back() == '\n' || line.back() == '\r' || line.back() == ' ' || line.back() == '\t'))
			line.pop_back();
		const char *s = line.c_str();
		while (*s == ' ' || *s == '\t')
			s++;
		if (!*s || *s == '#')
			continue;
		Line l{ 0, 0, INT32_MAX, 0 };
		bool ok = pos_field(s, l.index) && pos_field(s, l.lo);
		if (ok) {
			while (*s == ' ' || *s == '\t')
				s++;
			if (*s == '*' && (!s[1] || s[1] == ' ' || s[1] == '\t'))
				s++;
			else
				ok = pos_field(s, l.hi);
		}
		if (ok) {
			while (*s == ' ' || *s == '\t')
				s++;
			if (!strcmp(s, "end"))
				l.flags = ACM_POS_FROM_END;
			else if (*s)
				ok = false;
		}
		if (!ok)
			rc = acm::fail(ACM_ERR_PARSE, "%s:%d: not '<pattern index> <lo> <hi or *> [end]'", path, line_no);
		else if (l.index >= (int)a->patterns.size())
			rc = acm::fail(ACM_ERR_PARSE, "%s:%d: pattern index %d out of range (%zu patterns)", path, line_no, l.index,
			    a->patterns.size());
		else
			lines.push_back(l);
	}
	fclose(fp);
	if (rc != ACM_OK)
		return rc;
	for (const Line &l : lines)
		if ((rc = acm_automaton_set_position(a, l.index, l.lo, l.hi, l.flags)) != ACM_OK)
			return rc;
	return (int)lines.size();
}

static int hex_nibble(unsigned char c)
{
	if (c >= '0' && c <= '9') return c - '0';
	if (c >= 'a' && c <= 'f') return c - 'a' + 10;
	if (c >= 'A' && c <= 'F') return c - 'A' + 10;
	return -1;
}

// ---- replacements ---------------------------------------------------------------

extern "C" int acm_automaton_set_replacement(acm_automaton *a, int index, const unsigned char *bytes, int n, unsigned flags)
{
	if (!a || index < 0 || index >= (int)a->patterns.size())
		return acm::fail(ACM_ERR_ARG, "acm_automaton_set_replacement: index out of range");
	if (flags & ~(unsigned)ACM_REPL_FILL)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_set_replacement: unknown flag bits 0x%x", flags & ~(unsigned)ACM_REPL_FILL);
	if (n < 0 || (n > 0 && !bytes))
		return acm::fail(ACM_ERR_ARG, "acm_automaton_set_replacement: bad bytes (n = %d)", n);
	if ((flags & ACM_REPL_FILL) && n != 1)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_set_replacement: a fill takes one byte, not %d", n);
	if (n > ACM_REPLACEMENT_MAX_LEN)
		return acm::fail(ACM_ERR_LIMIT, "acm_automaton_set_replacement: %d bytes, at most %d", n, ACM_REPLACEMENT_MAX_LEN);
	acm_automaton::Pattern &p = a->patterns[index];
	p.repl_kind = (flags & ACM_REPL_FILL) ? acm::kReplFill : acm::kReplBytes;
	p.repl.assign(bytes, bytes + n);
	return ACM_OK;
}

extern "C" int acm_automaton_clear_replacement(acm_automaton *a, int index)
{
	if (!a || index < 0 || index >= (int)a->patterns.size())
		return acm::fail(ACM_ERR_ARG, "acm_automaton_clear_replacement: index out of range");
	a->patterns[index].repl_kind = acm::kReplNone;
	a->patterns[index].repl.clear();
	return ACM_OK;
}

extern "C" int acm_automaton_pattern_replacement(const acm_automaton *a, int index, const unsigned char **bytes, int *n,
    unsigned *flags)
{
	if (!a || index < 0 || index >= (int)a->patterns.size())
		return acm::fail(ACM_ERR_ARG, "acm_automaton_pattern_replacement: index out of range");
	const acm_automaton::Pattern &p = a->patterns[index];
	if (bytes) *bytes = p.repl.data();
	if (n) *n = (int)p.repl.size();
	if (flags) *flags = p.repl_kind == acm::kReplFill ? (unsigned)ACM_REPL_FILL : 0u;
	return p.repl_kind != acm::kReplNone ? 1 : 0;
}

extern "C" int acm_automaton_has_replacements(const acm_automaton *a)
{
	if (a)
		for (auto &p : a->patterns)
			if (p.repl_kind != acm::kReplNone)
				return 1;
	return 0;
}

extern "C" int acm_automaton_max_replacement_len(const acm_automaton *a)
{
	int longest = 0;
	if (a)
		for (auto &p : a->patterns)
			if (p.repl_kind == acm::kReplBytes)
				longest = std::max(longest, (int)p.repl.size());
	return longest;
}

extern "C" int acm_automaton_load_replacement_file(acm_automaton *a, const char *path)
{
	if (!a || !path)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_load_replacement_file: bad arguments");
	FILE *fp = fopen(path, "r");
	if (!fp)
		return acm::fail(ACM_ERR_IO, "cannot open replacement file '%s': %s", path, strerror(errno));
	struct Line {
		int32_t index;
		unsigned flags;
		std::vector<unsigned char> bytes;
	};
	std::vector<Line> lines;   // applied only when the whole file has parsed
	std::vector<char> buf(2 * (size_t)ACM_REPLACEMENT_MAX_LEN + 64);   // the longest legal line and its index
	int line_no = 0, rc = ACM_OK;
	while (rc == ACM_OK && fgets(buf.data(), (int)buf.size(), fp)) {
		line_no++;
		std::string line(buf.data());
		const bool whole = !line.empty() && line.back() == '\n';
		while (!line.empty() && (line.back() == '\n' || line.back() == '\r' || line.back() == ' ' || line.back() == '\t'))
			line.pop_back();
		const char *s = line.c_str();
		while (*s == ' ' || *s == '\t')
			s++;
		if (!*s || *s == '#')
			continue;
		Line l{ 0, 0, {} };
		bool ok = (whole || feof(fp)) && pos_field(s, l.index);
		if (ok) {
			while (*s == ' ' || *s == '\t')
				s++;
			if (!strncmp(s, "fill", 4) && (s[4] == ' ' || s[4] == '\t')) {
				s += 4;
				while (*s == ' ' || *s == '\t')
					s++;
				const int hi = hex_nibble((unsigned char)s[0]), lo = hi < 0 ? -1 : hex_nibble((unsigned char)s[1]);
				ok = lo >= 0 && !s[2];
				if (ok) {
					l.flags = ACM_REPL_FILL;
					l.bytes.push_back((unsigned char)(hi << 4 | lo));
				}
			} else {
				for (; ok && *s; s += 2) {
					const int hi = hex_nibble((unsigned char)s[0]), lo = hi < 0 ? -1 : hex_nibble((unsigned char)s[1]);
					ok = lo >= 0;
					if (ok)
						l.bytes.push_back((unsigned char)(hi << 4 | lo));
				}
				ok = ok && l.bytes.size() <= (size_t)ACM_REPLACEMENT_MAX_LEN;
			}
		}
		if (!ok)
			rc = acm::fail(ACM_ERR_PARSE, "%s:%d: not '<pattern index> <hex bytes or empty>' or '<pattern index> fill <hh>'", path,
			    line_no);
		else if (l.index >= (int)a->patterns.size())
			rc = acm::fail(ACM_ERR_PARSE, "%s:%d: pattern index %d out of range (%zu patterns)", path, line_no, l.index,
			    a->patterns.size());
		else
			lines.push_back(std::move(l));
	}
	fclose(fp);
	if (rc != ACM_OK)
		return rc;
	for (const Line &l : lines)
		if ((rc = acm_automaton_set_replacement(a, l.index, l.bytes.data(), (int)l.bytes.size(), l.flags)) != ACM_OK)
			return rc;
	return (int)lines.size();
}

// ---- sequences -----------------------------------------------------------------

extern "C" int acm_automaton_add_sequence(acm_automaton *a, const int32_t *parts, const int32_t *gap_lo, const int32_t *gap_hi,
    int nparts, int iid)
{
	if (!a || !parts || nparts < 1)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_add_sequence: bad arguments");
	if (nparts > ACM_SEQ_MAX_PARTS)
		return acm::fail(ACM_ERR_LIMIT, "acm_automaton_add_sequence: %d parts, at most %d", nparts, ACM_SEQ_MAX_PARTS);
	if (nparts > 1 && (!gap_lo || !gap_hi))
		return acm::fail(ACM_ERR_ARG, "acm_automaton_add_sequence: %d parts without gaps", nparts);
	if (a->sequences.size() >= (size_t)INT32_MAX)
		return acm::fail(ACM_ERR_LIMIT, "acm_automaton_add_sequence: too many sequences");
	for (int j = 0; j < nparts; j++) {
		const int32_t p = parts[j];
		if (p < 0 || p >= (int)a->patterns.size())
			return acm::fail(ACM_ERR_ARG, "acm_automaton_add_sequence: part %d: pattern index %d out of range", j, p);
		if (a->patterns[p].seq >= 0)
			return acm::fail(ACM_ERR_ARG, "acm_automaton_add_sequence: part %d: pattern %d is a part of sequence %d", j, p,
			    a->patterns[p].seq);
		if (a->patterns[p].bytes.empty())
			return acm::fail(ACM_ERR_ARG, "acm_automaton_add_sequence: part %d: pattern %d has length 0", j, p);
		for (int i = 0; i < j; i++)
			if (parts[i] == p)
				return acm::fail(ACM_ERR_ARG, "acm_automaton_add_sequence: pattern %d is part %d and part %d", p, i, j);
		if (j > 0 && (gap_lo[j - 1] < 0 || gap_hi[j - 1] < 0))
			return acm::fail(ACM_ERR_ARG, "acm_automaton_add_sequence: gap %d: negative bound (%d, %d)", j, gap_lo[j - 1],
			    gap_hi[j - 1]);
	}
	acm_automaton::Sequence s;
	s.iid = iid;
	s.parts.assign(parts, parts + nparts);
	if (nparts > 1) {
		s.gap_lo.assign(gap_lo, gap_lo + nparts - 1);
		s.gap_hi.assign(gap_hi, gap_hi + nparts - 1);
	}
	const int index = (int)a->sequences.size();
	a->sequences.push_back(std::move(s));
	for (int j = 0; j < nparts; j++) {
		a->patterns[parts[j]].seq = index;
		a->patterns[parts[j]].seq_level = j;
	}
	return index;
}

extern "C" int acm_automaton_num_sequences(const acm_automaton *a) { return a ? (int)a->sequences.size() : 0; }

extern "C" int acm_automaton_sequence(const acm_automaton *a, int index, int *iid, int *nparts, const int32_t **parts,
    const int32_t **gap_lo, const int32_t **gap_hi)
{
	if (!a || index < 0 || index >= (int)a->sequences.size())
		return acm::fail(ACM_ERR_ARG, "acm_automaton_sequence: index out of range");
	const acm_automaton::Sequence &s = a->sequences[index];
	if (iid) *iid = s.iid;
	if (nparts) *nparts = (int)s.parts.size();
	if (parts) *parts = s.parts.data();
	if (gap_lo) *gap_lo = s.gap_lo.data();
	if (gap_hi) *gap_hi = s.gap_hi.data();
	return ACM_OK;
}

extern "C" int acm_automaton_pattern_sequence(const acm_automaton *a, int pattern, int *sequence, int *level)
{
	if (!a || pattern < 0 || pattern >= (int)a->patterns.size())
		return acm::fail(ACM_ERR_ARG, "acm_automaton_pattern_sequence: index out of range");
	const acm_automaton::Pattern &p = a->patterns[pattern];
	if (p.seq < 0)
		return 0;
	if (sequence) *sequence = p.seq;
	if (level) *level = p.seq_level;
	return 1;
}

namespace {

// a signature body, parsed: the parts and the gap in front of every part but the first.  Syntax 0: a part is
// its bytes.  ACM_SIG_EXTENDED: a part is its positions, 32 bytes of set each (acm_automaton_add_wildcard).
struct SigGroup {
	int32_t at, width, negated;
	std::vector<unsigned char> bytes;   // the distinct strings
};

struct Signature {
	std::vector<std::vector<unsigned char>> parts;
	std::vector<std::vector<SigGroup>> groups;   // ACM_SIG_GROUPS: per part (empty without the bit)
	std::vector<int32_t> gap_lo, gap_hi;
	int iid = 0;
	bool has_iid = false;
	bool extended = false;
};

// digits at s[i]; false where there is none or the value is too large
bool sig_number(const char *s, size_t &i, int64_t &v)
{
	if (!isdigit((unsigned char)s[i]))
		return false;
	for (v = 0; isdigit((unsigned char)s[i]); i++)
		if ((v = v * 10 + (s[i] - '0')) >= INT32_MAX)
			return false;
	return true;
}

// {n}, {n-m}, {-m} or {n-} at s[i] == '{': the gap (l, h), h -1 unbounded; i moves behind it
bool sig_braces(const char *s, size_t &i, int64_t &l, int64_t &h)
{
	i++;
	bool ok;
	if (s[i] == '-') {   // {-m}
		i++;
		ok = sig_number(s, i, h);
	} else {
		ok = sig_number(s, i, l);
		if (ok && s[i] == '-') {   // {n-} or {n-m}
			i++;
			if (s[i] == '}')
				h = -1;
			else
				ok = sig_number(s, i, h);
		} else {
			h = l;   // {n}
		}
	}
	if (!ok || s[i] != '}')
		return false;
	i++;
	return true;
}

// the gap being summed between two parts
struct GapSum {
	int64_t lo = 0, hi = 0;   // hi: -1 unbounded
	bool open = false;
	bool add(int64_t l, int64_t h)
	{
		lo += l;
		hi = (hi < 0 || h < 0) ? -1 : hi + h;
		return lo < INT32_MAX && hi < INT32_MAX;
	}
	void close(Signature &sig)
	{
		sig.gap_lo.push_back((int32_t)lo);
		sig.gap_hi.push_back(hi < 0 ? INT32_MAX : (int32_t)hi);
		open = false;
	}
};

// Parses body (hex byte pairs, ??, *, {n}, {n-m}, {-m}, {n-}).  Returns 0, or the column (from 1) of the
// first byte that is wrong, with why.
int parse_signature(const char *s, Signature &sig, const char *&why)
{
	sig.parts.clear();
	sig.gap_lo.clear();
	sig.gap_hi.clear();
	std::vector<unsigned char> part;
	GapSum gap;
	size_t i = 0;
	while (s[i]) {
		const size_t at = i;
		const unsigned char c = (unsigned char)s[i];
		int64_t l = 0, h = 0;
		if (hex_nibble(c) >= 0) {
			if (hex_nibble((unsigned char)s[i + 1]) < 0) {
				why = s[i + 1] == '?' ? "nibble wildcards are not supported" : "odd hex digit";
				return (int)at + 1;
			}
			if (gap.open)
				gap.close(sig);
			part.push_back((unsigned char)(hex_nibble(c) << 4 | hex_nibble((unsigned char)s[i + 1])));
			i += 2;
			continue;
		}
		if (c == '?') {
			if (s[i + 1] != '?') {
				why = "nibble wildcards are not supported";
				return (int)at + 1;
			}
			l = h = 1;
			i += 2;
		} else if (c == '*') {
			h = -1;
			i++;
		} else if (c == '{') {
			if (!sig_braces(s, i, l, h)) {
				why = "not {n}, {n-m}, {-m} or {n-}";
				return (int)at + 1;
			}
		} else {
			why = (c == '(' || c == '|' || c == ')') ? "alternatives are not supported"
			      : c == '!'                         ? "negation is not supported"
			                                         : "not a hex digit, ??, * or {..}";
			return (int)at + 1;
		}
		if (part.empty() && !gap.open) {
			why = "a gap in front of the first part";
			return (int)at + 1;
		}
		if (!gap.open) {
			sig.parts.push_back(part);
			part.clear();
			gap = GapSum{ 0, 0, true };
		}
		if (!gap.add(l, h)) {
			why = "gap too large";
			return (int)at + 1;
		}
	}
	if (gap.open || part.empty()) {
		why = gap.open ? "a gap behind the last part" : "empty signature";
		return (int)i + 1;
	}
	sig.parts.push_back(part);
	if (sig.parts.size() > (size_t)ACM_SEQ_MAX_PARTS) {
		why = "too many parts";
		return (int)i + 1;
	}
	return 0;
}

inline void set_add(unsigned char *set, unsigned b) { set[b >> 3] |= (unsigned char)(1u << (b & 7)); }

int set_count(const unsigned char *set)
{
	int n = 0;
	for (int k = 0; k < 32; k++)
		n += __builtin_popcount(set[k]);
	return n;
}

// The extended syntax (ACM_SIG_EXTENDED): a position is HH, H?, ?H, ??, (HH|HH|...) or !(HH|...); * and {..}
// separate parts.  A part is its positions' sets.  Returns 0, or the column (from 1) of the first byte that is
// wrong, with why; a part without an exact byte is reported at the column it begins at.  with_groups
// (ACM_SIG_GROUPS): an alternative is one or more byte pairs, and a part has its groups beside its sets.
int parse_signature_ex(const char *s, Signature &sig, const char *&why, bool with_groups = false)
{
	sig.parts.clear();
	sig.groups.clear();
	std::vector<SigGroup> part_groups;
	sig.gap_lo.clear();
	sig.gap_hi.clear();
	sig.extended = true;
	std::vector<unsigned char> part;   // 32 bytes per position
	size_t part_at = 0;                // where the part began
	bool exact = false, last_any = false;
	GapSum gap;
	size_t i = 0;
	auto hex_pair = [&](size_t k) {   // the byte at s[k], s[k + 1], or -1
		const int a = hex_nibble((unsigned char)s[k]);
		const int b = a < 0 ? -1 : hex_nibble((unsigned char)s[k + 1]);
		return b < 0 ? -1 : (a << 4 | b);
	};
	while (s[i]) {
		const size_t at = i;
		const unsigned char c = (unsigned char)s[i];
		unsigned char set[32] = { 0 };
		bool position = true;
		int64_t l = 0, h = 0;
		if (hex_nibble(c) >= 0) {
			const int lo = hex_nibble((unsigned char)s[i + 1]);
			if (lo >= 0) {
				set_add(set, (unsigned)(hex_nibble(c) << 4 | lo));
			} else if (s[i + 1] == '?') {
				for (unsigned x = 0; x < 16; x++)
					set_add(set, (unsigned)hex_nibble(c) << 4 | x);
			} else {
				why = "odd hex digit";
				return (int)at + 1;
			}
			i += 2;
		} else if (c == '?') {
			const int lo = hex_nibble((unsigned char)s[i + 1]);
			if (s[i + 1] == '?') {
				memset(set, 0xFF, 32);
			} else if (lo >= 0) {
				for (unsigned x = 0; x < 16; x++)
					set_add(set, x << 4 | (unsigned)lo);
			} else {
				why = "not ?? or ?H";
				return (int)at + 1;
			}
			i += 2;
		} else if (c == '(' || c == '!') {
			if (c == '!' && s[i + 1] != '(') {
				why = "a ! that no ( follows";
				return (int)at + 1;
			}
			i += c == '!' ? 2 : 1;
			size_t width = 1;
			std::vector<unsigned char> strings;   // with_groups: the distinct alternatives, width bytes each
			while (with_groups) {   // (left by break)
				const size_t alt_at = i;
				std::vector<unsigned char> alt;
				for (int b; (b = hex_pair(i)) >= 0; i += 2)
					alt.push_back((unsigned char)b);
				if (alt.empty() || hex_nibble((unsigned char)s[i]) >= 0) {
					why = alt.empty() ? "not a hex byte in an alternative" : "odd hex digit";
					return (int)i + 1;
				}
				if (alt_at == at + (c == '!' ? 2 : 1))
					width = alt.size();
				if (alt.size() != width) {
					why = "an alternative of another width than the first";
					return (int)alt_at + 1;
				}
				bool seen = false;
				for (size_t k = 0; k < strings.size() && !seen; k += width)
					seen = !memcmp(&strings[k], alt.data(), width);
				if (!seen)
					strings.insert(strings.end(), alt.begin(), alt.end());
				if (s[i] == ')')
					break;
				if (s[i] != '|') {
					why = "not | or ) in an alternative";
					return (int)i + 1;
				}
				i++;
			}
			if (with_groups && width > 1) {
				i++;
				const size_t count = strings.size() / width;
				if (width > (size_t)ACM_GROUP_MAX_WIDTH || count > (size_t)ACM_GROUP_MAX_ALTERNATIVES) {
					why = width > (size_t)ACM_GROUP_MAX_WIDTH ? "alternatives of too many bytes" : "too many alternatives";
					return (int)at + 1;
				}
				const bool exact_run = c != '!' && count == 1;
				if (!exact_run && part_groups.size() >= (size_t)ACM_PATTERN_MAX_GROUPS) {
					why = "too many groups in a part";
					return (int)at + 1;
				}
				if (part.size() / 32 + width > (size_t)ACM_WILDCARD_MAX_POSITIONS) {
					why = "a part of too many positions";
					return (int)at + 1;
				}
				if (gap.open)
					gap.close(sig);
				if (part.empty()) {
					part_at = at;
					exact = false;
				}
				if (!exact_run)
					part_groups.push_back(SigGroup{ (int32_t)(part.size() / 32), (int32_t)width, c == '!', strings });
				for (size_t k = 0; k < width; k++) {
					unsigned char one[32] = { 0 };
					if (exact_run)
						set_add(one, strings[k]);
					else
						memset(one, 0xFF, 32);
					part.insert(part.end(), one, one + 32);
				}
				exact = exact || exact_run;
				last_any = false;
				continue;
			}
			for (size_t k = 0; k < strings.size(); k++)   // (one-byte alternatives: a set position)
				set_add(set, strings[k]);
			while (!with_groups) {
				const int b = hex_pair(i);
				if (b < 0) {
					why = "not a hex byte in an alternative";
					return (int)i + 1;
				}
				set_add(set, (unsigned)b);
				i += 2;
				if (s[i] == ')')
					break;
				if (s[i] != '|') {
					why = hex_nibble((unsigned char)s[i]) >= 0 ? "alternatives of more than one byte are not supported"
					                                           : "not | or ) in an alternative";
					return (int)i + 1;
				}
				i++;
			}
			i++;
			if (c == '!')
				for (int k = 0; k < 32; k++)
					set[k] = (unsigned char)~set[k];
			if (set_count(set) == 0) {
				why = "a position that no byte matches";
				return (int)at + 1;
			}
		} else if (c == '*') {
			position = false;
			h = -1;
			i++;
		} else if (c == '{') {
			position = false;
			if (!sig_braces(s, i, l, h)) {
				why = "not {n}, {n-m}, {-m} or {n-}";
				return (int)at + 1;
			}
		} else {
			why = "not a position, * or {..}";
			return (int)at + 1;
		}
		if (position) {
			const int n = set_count(set);
			if (sig.parts.empty() && part.empty() && n == 256) {
				why = "?? in front of the first position";
				return (int)at + 1;
			}
			if (part.size() / 32 >= (size_t)ACM_WILDCARD_MAX_POSITIONS) {
				why = "a part of too many positions";
				return (int)at + 1;
			}
			if (gap.open)
				gap.close(sig);
			if (part.empty()) {
				part_at = at;
				exact = false;
			}
			part.insert(part.end(), set, set + 32);
			exact = exact || n == 1;
			last_any = n == 256;
			continue;
		}
		if (part.empty() && !gap.open) {
			why = "a gap in front of the first part";
			return (int)at + 1;
		}
		if (!gap.open) {
			if (!exact) {
				why = "a part without an exact byte";
				return (int)part_at + 1;
			}
			sig.parts.push_back(part);
			sig.groups.push_back(part_groups);
			part.clear();
			part_groups.clear();
			gap = GapSum{ 0, 0, true };
		}
		if (!gap.add(l, h)) {
			why = "gap too large";
			return (int)at + 1;
		}
	}
	if (gap.open || part.empty()) {
		why = gap.open ? "a gap behind the last part" : "empty signature";
		return (int)i + 1;
	}
	if (last_any) {
		why = "?? behind the last position";
		return (int)i + 1;
	}
	if (!exact) {
		why = "a part without an exact byte";
		return (int)part_at + 1;
	}
	sig.parts.push_back(part);
	sig.groups.push_back(part_groups);
	if (sig.parts.size() > (size_t)ACM_SEQ_MAX_PARTS) {
		why = "too many parts";
		return (int)i + 1;
	}
	return 0;
}

// a body in the syntax asked for
int parse_body(unsigned syntax, const char *s, Signature &sig, const char *&why)
{
	if (!(syntax & ACM_SIG_EXTENDED))
		return parse_signature(s, sig, why);
	return parse_signature_ex(s, sig, why, (syntax & ACM_SIG_GROUPS) != 0);
}

// the context sets of two or more bytes among the n positions of sets that the automaton has not interned and
// fresh does not hold yet are added to fresh; false when the automaton would then hold more than 256
bool wild_room(const acm_automaton *a, const unsigned char *sets, int n, std::vector<std::array<uint8_t, 32>> &fresh)
{
	for (int i = 0; i < n; i++) {
		if (set_count(sets + 32 * (size_t)i) < 2)
			continue;
		std::array<uint8_t, 32> c;
		memcpy(c.data(), sets + 32 * (size_t)i, 32);
		if (std::find(a->wild_classes.begin(), a->wild_classes.end(), c) == a->wild_classes.end() &&
		    std::find(fresh.begin(), fresh.end(), c) == fresh.end())
			fresh.push_back(c);
	}
	return a->wild_classes.size() + fresh.size() <= 256;
}

// adds the parts and the sequence of a parsed signature: cannot fail but for memory, once signatures_fit
int apply_signature(acm_automaton *a, const Signature &sig, int iid, unsigned flags)
{
	std::vector<int32_t> parts;
	for (size_t k = 0; k < sig.parts.size(); k++) {
		const auto &p = sig.parts[k];
		parts.push_back((int32_t)a->patterns.size());
		std::vector<acm_wild_group> groups;   // (their limits were checked by the parser)
		if (k < sig.groups.size())
			for (const SigGroup &g : sig.groups[k])
				groups.push_back(acm_wild_group{ g.at, g.width, (int32_t)(g.bytes.size() / (size_t)g.width), g.negated, g.bytes.data() });
		const int rc = !sig.extended ? acm_automaton_add_ex(a, p.data(), (int)p.size(), iid, flags)
		               : groups.empty() ? acm_automaton_add_wildcard(a, p.data(), (int)(p.size() / 32), iid, flags)
		                                : acm_automaton_add_wildcard_groups(a, p.data(), (int)(p.size() / 32), groups.data(),
		                                      (int)groups.size(), iid, flags);
		if (rc < 0)
			return rc;
	}
	return acm_automaton_add_sequence(a, parts.data(), sig.gap_lo.data(), sig.gap_hi.data(), (int)parts.size(), iid);
}

// do the context sets of all these signatures fit the automaton's 256?  (Exact: a set of two or more bytes
// never lies in an anchor.)  Asked before anything is added, so that a refused load applies nothing.
bool signatures_fit(const acm_automaton *a, const Signature *sigs, size_t n)
{
	std::vector<std::array<uint8_t, 32>> fresh;
	for (size_t k = 0; k < n; k++)
		if (sigs[k].extended)
			for (const auto &p : sigs[k].parts)
				if (!wild_room(a, p.data(), (int)(p.size() / 32), fresh))
					return false;
	return true;
}

int sig_args(const char *fn, acm_automaton *a, const void *arg, unsigned flags, unsigned syntax)
{
	if (!a || !arg)
		return acm::fail(ACM_ERR_ARG, "%s: bad arguments", fn);
	if (flags & ~(unsigned)ACM_PATTERN_NOCASE)
		return acm::fail(ACM_ERR_ARG, "%s: unknown flag bits 0x%x", fn, flags & ~(unsigned)ACM_PATTERN_NOCASE);
	if (syntax & ~(unsigned)(ACM_SIG_EXTENDED | ACM_SIG_GROUPS))
		return acm::fail(ACM_ERR_ARG, "%s: unknown syntax bits 0x%x", fn, syntax & ~(unsigned)(ACM_SIG_EXTENDED | ACM_SIG_GROUPS));
	if ((syntax & ACM_SIG_GROUPS) && !(syntax & ACM_SIG_EXTENDED))
		return acm::fail(ACM_ERR_ARG, "%s: ACM_SIG_GROUPS needs ACM_SIG_EXTENDED", fn);
	if (a->compiled)
		return acm::fail(ACM_ERR_ARG, "%s: automaton already compiled", fn);
	return ACM_OK;
}

int add_signature(const char *fn, acm_automaton *a, const char *body, int iid, unsigned flags, unsigned syntax)
{
	if (int rc = sig_args(fn, a, body, flags, syntax))
		return rc;
	Signature sig;
	const char *why = "";
	if (const int col = parse_body(syntax, body, sig, why))
		return acm::fail(ACM_ERR_PARSE, "signature: column %d: %s", col, why);
	if (!signatures_fit(a, &sig, 1))
		return acm::fail(ACM_ERR_LIMIT, "%s: more than 256 distinct context sets", fn);
	return apply_signature(a, sig, iid, flags);
}

int load_signature_file(const char *fn, acm_automaton *a, const char *path, unsigned flags, unsigned syntax)
{
	if (int rc = sig_args(fn, a, path, flags, syntax))
		return rc;
	std::ifstream in(path);
	if (!in)
		return acm::fail(ACM_ERR_IO, "cannot open signature file '%s': %s", path, strerror(errno));
	std::vector<Signature> sigs;   // applied only when the whole file has parsed
	std::string line;
	for (int line_no = 1; std::getline(in, line); line_no++) {
		while (!line.empty() && (line.back() == '\n' || line.back() == '\r' || line.back() == ' ' || line.back() == '\t'))
			line.pop_back();
		size_t b = line.find_first_not_of(" \t");
		if (b == std::string::npos || line[b] == '#')
			continue;
		Signature sig;
		size_t k = b;
		int64_t iid = 0;
		while (k < line.size() && isdigit((unsigned char)line[k]) && iid <= INT32_MAX)
			iid = iid * 10 + (line[k++] - '0');
		if (k > b && k < line.size() && line[k] == ':') {
			if (iid > INT32_MAX)
				return acm::fail(ACM_ERR_PARSE, "%s:%d: iid too large", path, line_no);
			sig.iid = (int)iid;
			sig.has_iid = true;
			b = k + 1;
		}
		const char *why = "";
		const char *body = line.c_str() + b;
		if (const int col = parse_body(syntax, body, sig, why))
			return acm::fail(ACM_ERR_PARSE, "%s:%d: column %d: %s", path, line_no, (int)b + col, why);
		sigs.push_back(std::move(sig));
	}
	if (!signatures_fit(a, sigs.data(), sigs.size()))
		return acm::fail(ACM_ERR_LIMIT, "%s: '%s' needs more than 256 distinct context sets", fn, path);
	for (const Signature &sig : sigs) {
		const int rc = apply_signature(a, sig, sig.has_iid ? sig.iid : (int)a->sequences.size(), flags);
		if (rc < 0)
			return rc;
	}
	return (int)sigs.size();
}

}  // namespace

extern "C" int acm_automaton_add_signature(acm_automaton *a, const char *body, int iid, unsigned flags)
{
	return add_signature("acm_automaton_add_signature", a, body, iid, flags, 0);
}

extern "C" int acm_automaton_add_signature_ex(acm_automaton *a, const char *body, int iid, unsigned flags, unsigned syntax)
{
	return add_signature("acm_automaton_add_signature_ex", a, body, iid, flags, syntax);
}

extern "C" int acm_automaton_load_signature_file(acm_automaton *a, const char *path, unsigned flags)
{
	return load_signature_file("acm_automaton_load_signature_file", a, path, flags, 0);
}

extern "C" int acm_automaton_load_signature_file_ex(acm_automaton *a, const char *path, unsigned flags, unsigned syntax)
{
	return load_signature_file("acm_automaton_load_signature_file_ex", a, path, flags, syntax);
}

// ---- rules -------------------------------------------------------------------------

namespace {

// A rule's expression, compiled to its postfix program (acm::RuleOp).  Recursive descent over
//   expr := term ( '&' term )*  |  term ( '|' term )*
//   term := ( NUMBER | '(' expr ')' ) [ ( '=' | '>' | '<' ) NUMBER ]
// The first error stops it: code (ACM_ERR_PARSE or ACM_ERR_LIMIT), col (from 1) and why.
struct RuleParser {
	const char *s;
	int nops;
	std::vector<int32_t> &code;
	size_t i = 0;
	int err = 0, col = 0;
	const char *why = "";

	bool bad(int code_, size_t at, const char *w)
	{
		err = code_;
		col = (int)at + 1;
		why = w;
		return false;
	}
	void blanks()
	{
		while (s[i] == ' ' || s[i] == '\t')
			i++;
	}
	// digits at s[i], at most INT32_MAX
	bool number(int64_t &v)
	{
		const size_t at = i;
		for (v = 0; isdigit((unsigned char)s[i]); i++)
			if ((v = v * 10 + (s[i] - '0')) > INT32_MAX)
				return bad(ACM_ERR_PARSE, at, "number too large");
		return true;
	}
	bool term(int depth)
	{
		blanks();
		const size_t at = i;
		if (isdigit((unsigned char)s[i])) {
			int64_t op;
			if (!number(op))
				return false;
			if (op >= nops)
				return bad(ACM_ERR_PARSE, at, "operand out of range");
			code.insert(code.end(), { acm::kRulePush, (int32_t)op });
		} else if (s[i] == '(') {
			if (depth + 1 > ACM_RULE_MAX_NESTING)
				return bad(ACM_ERR_LIMIT, at, "parentheses nested too deep");
			i++;
			if (!expr(depth + 1))
				return false;
			blanks();
			if (s[i] != ')')
				return bad(ACM_ERR_PARSE, i, "expected )");
			i++;
		} else {
			return bad(ACM_ERR_PARSE, at, "expected an operand or (");
		}
		blanks();
		if (s[i] == '=' || s[i] == '>' || s[i] == '<') {
			const int32_t op = s[i] == '=' ? acm::kRuleEq : s[i] == '>' ? acm::kRuleGt : acm::kRuleLt;
			i++;
			blanks();
			if (!isdigit((unsigned char)s[i]))
				return bad(ACM_ERR_PARSE, i, "expected a number");
			int64_t n;
			if (!number(n))
				return false;
			if (s[i] == ',')
				return bad(ACM_ERR_PARSE, i, "the distinct-count form =n,m is not provided");
			code.insert(code.end(), { op, (int32_t)n });
		}
		return true;
	}
	bool expr(int depth)
	{
		if (!term(depth))
			return false;
		blanks();
		const char op = s[i];
		if (op != '&' && op != '|')
			return true;
		while (s[i] == op) {
			i++;
			if (!term(depth))
				return false;
			code.insert(code.end(), { op == '&' ? acm::kRuleAnd : acm::kRuleOr, 0 });
			blanks();
		}
		if (s[i] == '&' || s[i] == '|')
			return bad(ACM_ERR_PARSE, i, "& and | at one level without parentheses");
		return true;
	}
	bool all()
	{
		if (!expr(0))
			return false;
		blanks();
		if (s[i])
			return bad(ACM_ERR_PARSE, i, "unexpected character");
		return true;
	}
};

// the program over counts that are all 0: is the expression true for a text without a hit?
bool rule_true_when_empty(const std::vector<int32_t> &code)
{
	std::vector<std::pair<int64_t, bool>> st;
	for (size_t k = 0; k + 1 < code.size(); k += 2) {
		const int32_t op = code[k], arg = code[k + 1];
		if (op == acm::kRulePush) {
			st.push_back({ 0, false });
		} else if (op == acm::kRuleAnd || op == acm::kRuleOr) {
			const auto b = st.back();
			st.pop_back();
			auto &a = st.back();
			a.first += b.first;
			a.second = op == acm::kRuleAnd ? (a.second && b.second) : (a.second || b.second);
		} else {
			auto &a = st.back();
			a.second = op == acm::kRuleEq ? a.first == arg : op == acm::kRuleGt ? a.first > arg : a.first < arg;
		}
	}
	return !st.empty() && st.back().second;
}

// compiles expr over nops operands; on an error sets acm_last_error with the column shifted by col0
int compile_rule(const char *where, const char *expr, int nops, int col0, std::vector<int32_t> &code)
{
	code.clear();
	RuleParser p{ expr, nops, code };
	if (!p.all())
		return acm::fail(p.err, "%s: column %d: %s", where, col0 + p.col, p.why);
	if (rule_true_when_empty(code))
		return acm::fail(ACM_ERR_ARG, "%s: the expression is true for a text without any hit", where);
	return ACM_OK;
}

int rule_operand_count(const char *fn, int nops)
{
	if (nops < 1)
		return acm::fail(ACM_ERR_ARG, "%s: %d operands", fn, nops);
	if (nops > ACM_RULE_MAX_OPERANDS)
		return acm::fail(ACM_ERR_LIMIT, "%s: %d operands, at most %d", fn, nops, ACM_RULE_MAX_OPERANDS);
	return ACM_OK;
}

// registers a compiled rule over sequences that are free: cannot fail but for memory
int apply_rule(acm_automaton *a, const int32_t *sequences, int nops, const char *expr, std::vector<int32_t> code, int iid)
{
	acm_automaton::Rule r;
	r.iid = iid;
	r.sequences.assign(sequences, sequences + nops);
	r.expr = expr;
	r.code = std::move(code);
	const int index = (int)a->rules.size();
	a->rules.push_back(std::move(r));
	for (int j = 0; j < nops; j++) {
		a->sequences[sequences[j]].rule = index;
		a->sequences[sequences[j]].rule_op = j;
	}
	return index;
}

// a logical signature, parsed: "expr;body0;body1;..."
struct Logical {
	std::string expr;
	std::vector<int32_t> code;
	std::vector<Signature> bodies;
	int iid = 0;
	bool has_iid = false;
};

// parses line (its first byte is column col0 + 1 of what the caller shows); where: the prefix of the message
int parse_logical(const char *where, const char *line, int col0, unsigned syntax, Logical &out)
{
	const char *semi = strchr(line, ';');
	if (!semi)
		return acm::fail(ACM_ERR_PARSE, "%s: column %d: no ';' and subsignature behind the expression", where,
		    col0 + (int)strlen(line) + 1);
	out.expr.assign(line, semi);
	out.bodies.clear();
	for (const char *b = semi + 1;;) {
		const char *e = strchr(b, ';');
		const std::string body = e ? std::string(b, e) : std::string(b);
		const int at = col0 + (int)(b - line);
		if (const size_t colon = body.find(':'); colon != std::string::npos)
			return acm::fail(ACM_ERR_PARSE, "%s: column %d: subsignature offsets and modifiers are not supported", where,
			    at + (int)colon + 1);
		Signature sig;
		const char *why = "";
		if (const int col = parse_body(syntax, body.c_str(), sig, why))
			return acm::fail(ACM_ERR_PARSE, "%s: column %d: %s", where, at + col, why);
		out.bodies.push_back(std::move(sig));
		if (!e)
			break;
		b = e + 1;
	}
	if (int rc = rule_operand_count(where, (int)out.bodies.size()))
		return rc;
	return compile_rule(where, out.expr.c_str(), (int)out.bodies.size(), col0, out.code);
}

// adds the bodies and the rule of parsed logical signatures: cannot fail but for memory, once they fit
int apply_logical(acm_automaton *a, const Logical &l, int iid, unsigned flags)
{
	std::vector<int32_t> seqs;
	for (const Signature &sig : l.bodies) {
		const int q = apply_signature(a, sig, iid, flags);
		if (q < 0)
			return q;
		seqs.push_back(q);
	}
	return apply_rule(a, seqs.data(), (int)seqs.size(), l.expr.c_str(), l.code, iid);
}

bool logicals_fit(const acm_automaton *a, const std::vector<Logical> &ls)
{
	std::vector<Signature> all;
	for (const Logical &l : ls)
		all.insert(all.end(), l.bodies.begin(), l.bodies.end());
	return signatures_fit(a, all.data(), all.size());
}

}  // namespace

extern "C" int acm_automaton_add_rule(acm_automaton *a, const int32_t *sequences, int nops, const char *expr, int iid)
{
	const char *fn = "acm_automaton_add_rule";
	if (!a || !sequences || !expr)
		return acm::fail(ACM_ERR_ARG, "%s: bad arguments", fn);
	if (int rc = rule_operand_count(fn, nops))
		return rc;
	if (a->rules.size() >= (size_t)INT32_MAX)
		return acm::fail(ACM_ERR_LIMIT, "%s: too many rules", fn);
	for (int j = 0; j < nops; j++) {
		const int32_t q = sequences[j];
		if (q < 0 || q >= (int)a->sequences.size())
			return acm::fail(ACM_ERR_ARG, "%s: operand %d: sequence index %d out of range", fn, j, q);
		if (a->sequences[q].rule >= 0)
			return acm::fail(ACM_ERR_ARG, "%s: operand %d: sequence %d is an operand of rule %d", fn, j, q, a->sequences[q].rule);
		for (int i = 0; i < j; i++)
			if (sequences[i] == q)
				return acm::fail(ACM_ERR_ARG, "%s: sequence %d is operand %d and operand %d", fn, q, i, j);
	}
	std::vector<int32_t> code;
	if (int rc = compile_rule(fn, expr, nops, 0, code))
		return rc;
	return apply_rule(a, sequences, nops, expr, std::move(code), iid);
}

extern "C" int acm_automaton_num_rules(const acm_automaton *a) { return a ? (int)a->rules.size() : 0; }

extern "C" int acm_automaton_rule(const acm_automaton *a, int index, int *iid, int *nops, const int32_t **sequences,
    const char **expr)
{
	if (!a || index < 0 || index >= (int)a->rules.size())
		return acm::fail(ACM_ERR_ARG, "acm_automaton_rule: index out of range");
	const acm_automaton::Rule &r = a->rules[index];
	if (iid) *iid = r.iid;
	if (nops) *nops = (int)r.sequences.size();
	if (sequences) *sequences = r.sequences.data();
	if (expr) *expr = r.expr.c_str();
	return ACM_OK;
}

extern "C" int acm_automaton_sequence_rule(const acm_automaton *a, int sequence, int *rule, int *operand)
{
	if (!a || sequence < 0 || sequence >= (int)a->sequences.size())
		return acm::fail(ACM_ERR_ARG, "acm_automaton_sequence_rule: index out of range");
	const acm_automaton::Sequence &s = a->sequences[sequence];
	if (s.rule < 0)
		return 0;
	if (rule) *rule = s.rule;
	if (operand) *operand = s.rule_op;
	return 1;
}

extern "C" int acm_automaton_add_logical_signature(acm_automaton *a, const char *line, int iid, unsigned flags, unsigned syntax)
{
	const char *fn = "acm_automaton_add_logical_signature";
	if (int rc = sig_args(fn, a, line, flags, syntax))
		return rc;
	std::vector<Logical> l(1);
	if (int rc = parse_logical("logical signature", line, 0, syntax, l[0]))
		return rc;
	if (!logicals_fit(a, l))
		return acm::fail(ACM_ERR_LIMIT, "%s: more than 256 distinct context sets", fn);
	return apply_logical(a, l[0], iid, flags);
}

extern "C" int acm_automaton_load_logical_file(acm_automaton *a, const char *path, unsigned flags, unsigned syntax)
{
	const char *fn = "acm_automaton_load_logical_file";
	if (int rc = sig_args(fn, a, path, flags, syntax))
		return rc;
	std::ifstream in(path);
	if (!in)
		return acm::fail(ACM_ERR_IO, "cannot open logical signature file '%s': %s", path, strerror(errno));
	std::vector<Logical> ls;   // applied only when the whole file has parsed
	std::string line;
	for (int line_no = 1; std::getline(in, line); line_no++) {
		while (!line.empty() && (line.back() == '\n' || line.back() == '\r' || line.back() == ' ' || line.back() == '\t'))
			line.pop_back();
		size_t b = line.find_first_not_of(" \t");
		if (b == std::string::npos || line[b] == '#')
			continue;
		Logical l;
		size_t k = b;
		int64_t iid = 0;
		while (k < line.size() && isdigit((unsigned char)line[k]) && iid <= INT32_MAX)
			iid = iid * 10 + (line[k++] - '0');
		if (k > b && k < line.size() && line[k] == ':') {
			if (iid > INT32_MAX)
				return acm::fail(ACM_ERR_PARSE, "%s:%d: iid too large", path, line_no);
			l.iid = (int)iid;
			l.has_iid = true;
			b = k + 1;
		}
		char where[320];
		snprintf(where, sizeof(where), "%.280s:%d", path, line_no);
		if (int rc = parse_logical(where, line.c_str() + b, (int)b, syntax, l))
			return rc;
		ls.push_back(std::move(l));
	}
	if (!logicals_fit(a, ls))
		return acm::fail(ACM_ERR_LIMIT, "%s: '%s' needs more than 256 distinct context sets", fn, path);
	for (const Logical &l : ls) {
		const int rc = apply_logical(a, l, l.has_iid ? l.iid : (int)a->rules.size(), flags);
		if (rc < 0)
			return rc;
	}
	return (int)ls.size();
}

// ---- wildcard patterns -----------------------------------------------------------

// the groups of a wildcard pattern of n positions, checked and with equal strings dropped: ACM_OK or the error
static int checked_groups(const char *fn, const uint8_t *sets, int n, const acm_wild_group *groups, int ngroups,
    std::vector<acm_automaton::Pattern::Group> &out)
{
	if (ngroups < 0 || (ngroups > 0 && !groups))
		return acm::fail(ACM_ERR_ARG, "%s: bad arguments", fn);
	if (ngroups > ACM_PATTERN_MAX_GROUPS)
		return acm::fail(ACM_ERR_LIMIT, "%s: %d groups, at most %d", fn, ngroups, ACM_PATTERN_MAX_GROUPS);
	int end = 0;   // behind the group in front
	for (int j = 0; j < ngroups; j++) {
		const acm_wild_group &g = groups[j];
		if (!g.bytes || g.width < 2 || g.count < 1 || (g.negated != 0 && g.negated != 1))
			return acm::fail(ACM_ERR_ARG, "%s: group %d: width %d, count %d, negated %d", fn, j, g.width, g.count, g.negated);
		if (g.width > ACM_GROUP_MAX_WIDTH)
			return acm::fail(ACM_ERR_LIMIT, "%s: group %d: width %d, at most %d", fn, j, g.width, ACM_GROUP_MAX_WIDTH);
		if (g.at < 0 || g.at > n - g.width)
			return acm::fail(ACM_ERR_ARG, "%s: group %d: positions [%d, %ld) leave the pattern's %d", fn, j, g.at,
			    (long)g.at + g.width, n);
		if (g.at < end)
			return acm::fail(ACM_ERR_ARG, "%s: group %d begins at %d, inside or in front of the group before it", fn, j, g.at);
		end = g.at + g.width;
		for (int i = g.at; i < end; i++)
			for (int k = 0; k < 32; k++)
				if (sets[32 * (size_t)i + k] != 0xFF)
					return acm::fail(ACM_ERR_ARG, "%s: group %d: position %d does not carry the full set", fn, j, i);
		acm_automaton::Pattern::Group o{ g.at, g.width, g.negated, {} };
		for (int c = 0; c < g.count; c++) {
			const uint8_t *str = g.bytes + (size_t)c * g.width;
			bool seen = false;
			for (size_t k = 0; k < o.bytes.size() && !seen; k += g.width)
				seen = !memcmp(&o.bytes[k], str, g.width);
			if (seen)
				continue;
			if (o.bytes.size() / g.width >= (size_t)ACM_GROUP_MAX_ALTERNATIVES)
				return acm::fail(ACM_ERR_LIMIT, "%s: group %d: more than %d distinct strings", fn, j, ACM_GROUP_MAX_ALTERNATIVES);
			o.bytes.insert(o.bytes.end(), str, str + g.width);
		}
		out.push_back(std::move(o));
	}
	return ACM_OK;
}

static int add_wildcard(const char *fn, acm_automaton *a, const uint8_t *sets, int n, const acm_wild_group *groups, int ngroups,
    int iid, unsigned flags)
{
	if (!a || !sets || n < 1)
		return acm::fail(ACM_ERR_ARG, "%s: bad arguments", fn);
	if (flags & ~(unsigned)ACM_PATTERN_NOCASE)
		return acm::fail(ACM_ERR_ARG, "%s: unknown flag bits 0x%x", fn, flags & ~(unsigned)ACM_PATTERN_NOCASE);
	if (a->compiled)
		return acm::fail(ACM_ERR_ARG, "%s: automaton already compiled", fn);
	if (n > ACM_WILDCARD_MAX_POSITIONS)
		return acm::fail(ACM_ERR_LIMIT, "%s: %d positions, at most %d", fn, n, ACM_WILDCARD_MAX_POSITIONS);
	std::vector<acm_automaton::Pattern::Group> checked;
	if (int rc = checked_groups(fn, sets, n, groups, ngroups, checked))
		return rc;
	// the anchor: the longest run of one-byte sets, the leftmost among equal runs
	int at = 0, len = 0, run = 0;
	for (int i = 0; i < n; i++) {
		const int c = set_count(sets + 32 * (size_t)i);
		if (c == 0)
			return acm::fail(ACM_ERR_ARG, "%s: position %d: empty set", fn, i);
		run = c == 1 ? run + 1 : 0;
		if (run > len) {
			len = run;
			at = i + 1 - run;
		}
	}
	if (len == 0)
		return acm::fail(ACM_ERR_ARG, "%s: no position with a one-byte set", fn);
	const int pre = at, post = n - at - len;
	std::vector<std::array<uint8_t, 32>> fresh;
	if (!wild_room(a, sets, pre, fresh) || !wild_room(a, sets + 32 * (size_t)(at + len), post, fresh))
		return acm::fail(ACM_ERR_LIMIT, "%s: more than 256 distinct context sets", fn);
	auto only_byte = [&](int i) {
		const uint8_t *s = sets + 32 * (size_t)i;
		for (int b = 0; b < 256; b++)
			if (s[b >> 3] >> (b & 7) & 1)
				return b;
		return 0;
	};
	std::vector<unsigned char> anchor(len);
	for (int i = 0; i < len; i++)
		anchor[i] = (unsigned char)only_byte(at + i);
	const int index = (int)a->patterns.size();
	if (int rc = acm_automaton_add_ex(a, anchor.data(), len, iid, flags))
		return rc;
	a->wild_classes.insert(a->wild_classes.end(), fresh.begin(), fresh.end());
	acm_automaton::Pattern &p = a->patterns[index];
	p.wild_pre = pre;
	p.wild_post = post;
	p.wild_groups = std::move(checked);
	for (int i = 0; i < n; i++) {
		if (i >= at && i < at + len)
			continue;
		const uint8_t *s = sets + 32 * (size_t)i;
		p.wild_sets.insert(p.wild_sets.end(), s, s + 32);
		if (set_count(s) == 1) {
			p.wild_cells.push_back((uint16_t)only_byte(i));
		} else {
			std::array<uint8_t, 32> c;
			memcpy(c.data(), s, 32);
			const size_t k = std::find(a->wild_classes.begin(), a->wild_classes.end(), c) - a->wild_classes.begin();
			p.wild_cells.push_back((uint16_t)(0x100 | k));
		}
	}
	return index;
}

extern "C" int acm_automaton_add_wildcard(acm_automaton *a, const uint8_t *sets, int n, int iid, unsigned flags)
{
	return add_wildcard("acm_automaton_add_wildcard", a, sets, n, nullptr, 0, iid, flags);
}

extern "C" int acm_automaton_add_wildcard_groups(acm_automaton *a, const uint8_t *sets, int n, const acm_wild_group *groups,
    int ngroups, int iid, unsigned flags)
{
	return add_wildcard("acm_automaton_add_wildcard_groups", a, sets, n, groups, ngroups, iid, flags);
}

extern "C" int acm_automaton_pattern_groups(const acm_automaton *a, int index)
{
	if (!a || index < 0 || index >= (int)a->patterns.size())
		return acm::fail(ACM_ERR_ARG, "acm_automaton_pattern_groups: index out of range");
	return (int)a->patterns[index].wild_groups.size();
}

extern "C" int acm_automaton_pattern_group(const acm_automaton *a, int index, int j, int *at, int *width, int *count,
    int *negated, const uint8_t **bytes)
{
	if (!a || index < 0 || index >= (int)a->patterns.size() || j < 0 || j >= (int)a->patterns[index].wild_groups.size())
		return acm::fail(ACM_ERR_ARG, "acm_automaton_pattern_group: index out of range");
	const acm_automaton::Pattern::Group &g = a->patterns[index].wild_groups[j];
	if (at) *at = g.at;
	if (width) *width = g.width;
	if (count) *count = (int)(g.bytes.size() / (size_t)g.width);
	if (negated) *negated = g.negated;
	if (bytes) *bytes = g.bytes.data();
	return ACM_OK;
}

extern "C" int acm_automaton_groups(const acm_automaton *a)
{
	if (a)
		for (auto &p : a->patterns)
			if (!p.wild_groups.empty())
				return 1;
	return 0;
}

extern "C" int acm_automaton_pattern_wildcard(const acm_automaton *a, int index, int *pre, int *post, const uint8_t **pre_sets,
    const uint8_t **post_sets)
{
	if (!a || index < 0 || index >= (int)a->patterns.size())
		return acm::fail(ACM_ERR_ARG, "acm_automaton_pattern_wildcard: index out of range");
	const acm_automaton::Pattern &p = a->patterns[index];
	if (pre) *pre = p.wild_pre;
	if (post) *post = p.wild_post;
	if (pre_sets) *pre_sets = p.wild_sets.data();
	if (post_sets) *post_sets = p.wild_sets.data() + 32 * (size_t)p.wild_pre;
	return (p.wild_pre || p.wild_post) ? 1 : 0;
}

extern "C" int acm_automaton_wildcards(const acm_automaton *a)
{
	if (a)
		for (auto &p : a->patterns)
			if (p.wild_pre || p.wild_post)
				return 1;
	return 0;
}

extern "C" int acm_automaton_wildcard_reach(const acm_automaton *a, int *back, int *ahead)
{
	if (!a)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_wildcard_reach: null automaton");
	int b = 0, f = 0;
	for (auto &p : a->patterns)
		if (p.wild_pre || p.wild_post) {
			b = std::max(b, p.wild_pre + (int)p.bytes.size());
			f = std::max(f, p.wild_post);
		}
	if (back) *back = b;
	if (ahead) *ahead = f;
	return ACM_OK;
}

// ---- approximate patterns ------------------------------------------------------

// where piece i of an approximate pattern of n bytes and budget k begins (i == k + 1: n)
static int approx_piece_begin(int n, int k, int i)
{
	const int q = n / (k + 1), r = n % (k + 1);
	return i * q + std::min(i, r);
}

// acm_automaton_add_approx and acm_automaton_add_edit: the same pieces, checks and errors; fn names the caller,
// max_k is its largest budget and mode what the pattern's distance is (acm_automaton_approx_mode)
static int add_pieces(acm_automaton *a, const char *fn, const unsigned char *bytes, int n, int k, int iid, unsigned flags, int max_k,
    int mode)
{
	if (!a || n < 0 || (n > 0 && !bytes) || k < 0)
		return acm::fail(ACM_ERR_ARG, "%s: bad arguments", fn);
	if (flags & ~(unsigned)ACM_PATTERN_NOCASE)
		return acm::fail(ACM_ERR_ARG, "%s: unknown flag bits 0x%x", fn, flags & ~(unsigned)ACM_PATTERN_NOCASE);
	if (a->compiled)
		return acm::fail(ACM_ERR_ARG, "%s: automaton already compiled", fn);
	if (k > max_k)
		return acm::fail(ACM_ERR_LIMIT, "%s: budget %d, at most %d", fn, k, max_k);
	const int index = (int)a->patterns.size();
	if (k == 0) {
		const int rc = acm_automaton_add_ex(a, bytes, n, iid, flags);
		return rc != ACM_OK ? rc : index;
	}
	if (n < k + 1)
		return acm::fail(ACM_ERR_ARG, "%s: %d bytes cannot be cut into %d pieces", fn, n, k + 1);
	if (n > ACM_APPROX_MAX_LEN)
		return acm::fail(ACM_ERR_LIMIT, "%s: %d bytes, at most %d", fn, n, ACM_APPROX_MAX_LEN);
	acm_automaton::Approx x;
	x.first_piece = index;
	x.n = n;
	x.k = k;
	x.iid = iid;
	x.flags = flags;
	x.mode = mode;
	x.bytes.assign(bytes, bytes + n);
	a->patterns.reserve(a->patterns.size() + (size_t)k + 1);   // (nothing is applied when memory runs out half way)
	a->approx.reserve(a->approx.size() + 1);
	for (int i = 0; i <= k; i++) {
		const int b = approx_piece_begin(n, k, i), e = approx_piece_begin(n, k, i + 1);
		if (int rc = acm_automaton_add_ex(a, bytes + b, e - b, iid, flags)) {   // (every check it makes was made above)
			a->patterns.resize((size_t)index);
			return rc;
		}
		a->patterns.back().approx = (int32_t)a->approx.size();
		a->patterns.back().approx_piece = i;
	}
	a->approx.push_back(std::move(x));
	return index;
}

extern "C" int acm_automaton_add_approx(acm_automaton *a, const unsigned char *bytes, int n, int k, int iid, unsigned flags)
{
	return add_pieces(a, "acm_automaton_add_approx", bytes, n, k, iid, flags, ACM_APPROX_MAX_K, 0);
}

extern "C" int acm_automaton_add_edit(acm_automaton *a, const unsigned char *bytes, int n, int k, int iid, unsigned flags)
{
	return add_pieces(a, "acm_automaton_add_edit", bytes, n, k, iid, flags, ACM_EDIT_MAX_K, 1);
}

extern "C" int acm_automaton_approx_mode(const acm_automaton *a, int x)
{
	if (!a || x < 0 || x >= (int)a->approx.size())
		return acm::fail(ACM_ERR_ARG, "acm_automaton_approx_mode: index out of range");
	return a->approx[x].mode;
}

extern "C" int acm_automaton_num_approx(const acm_automaton *a) { return a ? (int)a->approx.size() : 0; }

extern "C" int acm_automaton_approx(const acm_automaton *a, int x, int *first_piece, int *n, int *k, int *iid, unsigned *flags,
    const unsigned char **bytes)
{
	if (!a || x < 0 || x >= (int)a->approx.size())
		return acm::fail(ACM_ERR_ARG, "acm_automaton_approx: index out of range");
	const acm_automaton::Approx &p = a->approx[x];
	if (first_piece) *first_piece = p.first_piece;
	if (n) *n = p.n;
	if (k) *k = p.k;
	if (iid) *iid = p.iid;
	if (flags) *flags = p.flags;
	if (bytes) *bytes = p.bytes.data();
	return ACM_OK;
}

extern "C" int acm_automaton_pattern_approx(const acm_automaton *a, int index, int *x, int *piece, int *pre, int *post)
{
	if (!a || index < 0 || index >= (int)a->patterns.size())
		return acm::fail(ACM_ERR_ARG, "acm_automaton_pattern_approx: index out of range");
	const acm_automaton::Pattern &p = a->patterns[index];
	const bool is = p.approx >= 0;
	const acm_automaton::Approx *q = is ? &a->approx[p.approx] : nullptr;
	if (x) *x = p.approx;
	if (piece) *piece = is ? p.approx_piece : 0;
	if (pre) *pre = is ? approx_piece_begin(q->n, q->k, p.approx_piece) : 0;
	if (post) *post = is ? q->n - approx_piece_begin(q->n, q->k, p.approx_piece + 1) : 0;
	return is ? 1 : 0;
}

extern "C" int acm_automaton_approx_reach(const acm_automaton *a, int *back, int *ahead)
{
	if (!a)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_approx_reach: null automaton");
	int b = 0, f = 0;
	for (auto &p : a->approx) {
		const int slack = p.mode ? p.k : 0;   // an edit pattern's span begins up to 2k in front and ends up to k behind
		b = std::max(b, p.n + 2 * slack);
		f = std::max(f, p.n - approx_piece_begin(p.n, p.k, 1) + slack);   // (piece 0 has the most behind it)
	}
	if (back) *back = b;
	if (ahead) *ahead = f;
	return ACM_OK;
}

// ---- pattern file ------------------------------------------------------------

// "[+-]?digits" followed by a blank => the file is "ID pattern" per line.
// The reference decides this on line 0 only (ocl_worker.c:79-102); its scan
// loop is broken (tests i instead of j), we implement what it means to do.
static bool looks_categorical(const std::string &line)
{
	size_t sp = line.find_first_of(" \t");
	if (sp == std::string::npos || sp == 0)
		return false;
	size_t k = (line[0] == '+' || line[0] == '-') ? 1 : 0;
	if (k >= sp)
		return false;
	for (; k < sp; k++)
		if (!isdigit((unsigned char)line[k]))
			return false;
	return true;
}

extern "C" int acm_automaton_load_file(acm_automaton *a, const char *path, int hex, int max_len)
{
	return acm_automaton_load_file_ex(a, path, hex, max_len, 0);
}

extern "C" int acm_automaton_load_file_ex(acm_automaton *a, const char *path, int hex, int max_len, unsigned flags)
{
	if (!a || !path)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_load_file: bad arguments");
	if (flags & ~(unsigned)ACM_PATTERN_NOCASE)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_load_file_ex: unknown flag bits 0x%x", flags & ~(unsigned)ACM_PATTERN_NOCASE);
	FILE *fp = fopen(path, "r");
	if (!fp)
		return acm::fail(ACM_ERR_IO, "cannot open pattern file '%s': %s", path, strerror(errno));

	// The reference reads with fgets into a 4096-byte buffer, so a longer
	// line arrives in pieces, each piece a pattern of its own (Q18).  Keep
	// that: it is observable through pattern indices.
	std::vector<char> buf(acm::kMaxPatternLine);
	bool categorical = false;
	int line_no = 0, rc = ACM_OK;
	while (fgets(buf.data(), (int)buf.size(), fp)) {
		std::string line(buf.data());
		if (!line.empty() && line.back() == '\n')
			line.pop_back();
		if (line_no == 0)
			categorical = looks_categorical(line);

		long iid = line_no;
		std::string pat = line;
		if (categorical) {
			char *end = nullptr;
			errno = 0;
			iid = strtol(line.c_str(), &end, 10);
			if (errno != 0) {
				rc = acm::fail(ACM_ERR_PARSE, "%s:%d: bad pattern id", path, line_no + 1);
				break;
			}
			while (*end && isspace((unsigned char)*end))
				end++;
			pat.assign(end);
		}
		if (pat.size() >= 2 && pat.front() == '"' && pat.back() == '"')
			pat = pat.substr(1, pat.size() - 2);
		else if (pat.size() == 1 && pat[0] == '"')
			pat.clear();

		if (hex) {
			if (max_len != -1 && pat.size() > (size_t)max_len * 2)
				pat.resize((size_t)max_len * 2);
			if (pat.size() % 2) {  // utils.c:39-42 prints and exits
				rc = acm::fail(ACM_ERR_PARSE, "%s:%d: odd number of hex digits", path,
				    line_no + 1);
				break;
			}
			std::vector<unsigned char> bytes(pat.size() / 2);
			bool ok = true;
			for (size_t k = 0; k < bytes.size(); k++) {
				int hi = hex_nibble((unsigned char)pat[2 * k]);
				int lo = hex_nibble((unsigned char)pat[2 * k + 1]);
				if (hi < 0 || lo < 0) {
					ok = false;
					break;
				}
				bytes[k] = (unsigned char)(hi * 16 + lo);
			}
			if (!ok) {
				rc = acm::fail(ACM_ERR_PARSE, "%s:%d: not a hex digit", path, line_no + 1);
				break;
			}
			rc = acm_automaton_add_ex(a, bytes.data(), (int)bytes.size(), (int)iid, flags);
		} else {
			if (max_len != -1 && pat.size() > (size_t)max_len)
				pat.resize((size_t)max_len);
			rc = acm_automaton_add_ex(a, (const unsigned char *)pat.data(), (int)pat.size(), (int)iid, flags);
		}
		if (rc != ACM_OK)
			break;
		line_no++;
	}
	fclose(fp);
	return rc == ACM_OK ? line_no : rc;
}

// ---- compile -------------------------------------------------------------------

namespace {

struct Builder {
	acm_automaton &a;
	std::unordered_map<uint64_t, uint32_t> edge;  // (state << 8 | byte) -> child
	std::vector<std::vector<int32_t>> own;        // per state, patterns in the order they were attached

	explicit Builder(acm_automaton &aut) : a(aut) {}

	uint32_t child(uint32_t s, uint8_t c) const
	{
		auto it = edge.find(((uint64_t)s << 8) | c);
		return it == edge.end() ? UINT32_MAX : it->second;
	}

	// Newest pattern first: acsm_add_pattern prepends (acsmx.c:536-538) and
	// acsm_compile walks from the head (:579-580), so the last line of the
	// pattern file creates states 1..n.
	void insert_patterns()
	{
		size_t total = 1;
		for (auto &p : a.patterns)
			total += p.bytes.size();
		edge.reserve(total * 2);
		a.parent.assign(1, 0);
		a.in_byte.assign(1, 0);
		a.depth.assign(1, 0);
		own.assign(1, {});
		for (int i = (int)a.patterns.size() - 1; i >= 0; i--) {
			const auto &bytes = a.patterns[i].bytes;
			uint32_t s = 0;
			size_t k = 0;
			for (; k < bytes.size(); k++) {
				uint32_t t = child(s, bytes[k]);
				if (t == UINT32_MAX)
					break;
				s = t;
			}
			for (; k < bytes.size(); k++) {
				uint32_t t = (uint32_t)a.parent.size();
				edge.emplace(((uint64_t)s << 8) | bytes[k], t);
				a.parent.push_back(s);
				a.in_byte.push_back(bytes[k]);
				a.depth.push_back((uint16_t)(a.depth[s] + 1));
				own.emplace_back();
				s = t;
			}
			own[s].push_back(i);
		}
		a.num_states = (uint32_t)a.parent.size();
	}

	void index_children()
	{
		uint32_t n = a.num_states;
		a.child_begin.assign(n + 1, 0);
		for (uint32_t s = 1; s < n; s++)
			a.child_begin[a.parent[s] + 1]++;
		for (uint32_t s = 0; s < n; s++)
			a.child_begin[s + 1] += a.child_begin[s];
		a.child_list.resize(n ? n - 1 : 0);
		std::vector<uint32_t> cursor(a.child_begin.begin(), a.child_begin.end() - 1);
		for (uint32_t s = 1; s < n; s++)
			a.child_list[cursor[a.parent[s]]++] = { a.in_byte[s], s };
		for (uint32_t s = 0; s < n; s++)
			std::sort(a.child_list.begin() + a.child_begin[s],
			    a.child_list.begin() + a.child_begin[s + 1],
			    [](const acm_automaton::Edge &x, const acm_automaton::Edge &y) {
				    return x.byte < y.byte;
			    });
	}

	// BFS: fail links on the trie, and the match list of every state:
	//   list(s) = reverse(list(fail(s))) ++ own(s), own(s) newest first.
	// That is what build_NFA's "copy every node of the fail state's list,
	// each pushed at the front" produces (acsmx.c:417-429) on top of the
	// push-front of add_match_list_entry (:304-309).
	void link_and_collect()
	{
		uint32_t n = a.num_states;
		a.fail.assign(n, 0);
		a.list_begin.assign(n, -1);
		a.list_len.assign(n, 0);
		a.list_pool.clear();
		a.bfs_order.clear();
		a.bfs_order.reserve(n);
		a.bfs_order.push_back(0);
		set_list(0, 0, false);
		for (size_t qh = 0; qh < a.bfs_order.size(); qh++) {
			uint32_t s = a.bfs_order[qh];
			for (uint32_t e = a.child_begin[s]; e < a.child_begin[s + 1]; e++) {
				uint32_t t = a.child_list[e].to;
				uint8_t c = a.child_list[e].byte;
				uint32_t f = 0;
				if (s != 0) {
					uint32_t g = a.fail[s];
					for (;;) {
						uint32_t u = child(g, c);
						if (u != UINT32_MAX) {
							f = u;
							break;
						}
						if (g == 0)
							break;
						g = a.fail[g];
					}
				}
				a.fail[t] = f;
				// depth-1 states get fail = root WITHOUT inheriting the
				// root's list (acsmx.c:376-382 vs :417-429); it only
				// matters when an empty pattern made the root "final"
				set_list(t, f, /*inherit=*/s != 0);
				a.bfs_order.push_back(t);
			}
		}
	}

	void set_list(uint32_t s, uint32_t f, bool inherit)
	{
		int inherited = inherit ? a.list_len[f] : 0;
		int total = inherited + (int)own[s].size();
		if (total == 0)
			return;
		a.list_begin[s] = (int32_t)a.list_pool.size();
		a.list_len[s] = total;
		for (int k = inherited - 1; k >= 0; k--) {
			int32_t v = a.list_pool[a.list_begin[f] + k];
			a.list_pool.push_back(v);
		}
		for (int k = (int)own[s].size() - 1; k >= 0; k--)
			a.list_pool.push_back(own[s][k]);
	}

	// dev ids: hot rows first (the first non-final states in BFS order), then
	// the other non-final states and the final states, both in ref order.
	// The root is never final: a transition into state 0 cannot be flagged
	// because the reference stores finals as -state (acsmx.c:645).
	void byte_classes()
	{
		bool used[256] = { false };
		for (const auto &p : a.patterns)
			for (uint8_t b : p.bytes)
				used[b] = true;
		uint32_t nused = 0;
		for (int b = 0; b < 256; b++)
			nused += used[b] ? 1 : 0;
		const uint32_t classes = nused + (nused < 256 ? 1 : 0);
		if (classes > 128) {   // nothing to gain: the identity
			for (int b = 0; b < 256; b++)
				a.byte_class[b] = a.class_byte[b] = (uint8_t)b;
			a.num_classes = 256;
			a.log_stride = 8;
			return;
		}
		uint32_t next = 1, spare = 0;
		for (int b = 0; b < 256; b++)
			if (!used[b])
				spare = (uint32_t)b;   // (one exists: fewer than 256 bytes are used)
		memset(a.class_byte, (int)spare, sizeof(a.class_byte));
		for (int b = 0; b < 256; b++) {
			a.byte_class[b] = used[b] ? (uint8_t)next : 0;
			if (used[b])
				a.class_byte[next++] = (uint8_t)b;
		}
		if (a.nocase)   // (no lowercase letter is used: each gets its uppercase letter's class)
			for (uint32_t b = 'a'; b <= 'z'; b++)
				a.byte_class[b] = a.byte_class[acm::fold_byte(b)];
		a.num_classes = classes;
		a.log_stride = 1;
		while ((1u << a.log_stride) < classes)
			a.log_stride++;
	}

	void number_for_device()
	{
		const uint32_t n = a.num_states;
		// rows the LDS budget of the walk kernel holds (a hot cell is 16 bits: ids below the sentinel)
		const uint32_t hot_max = std::min<uint32_t>(acm::kHotBytes / (2u << a.log_stride), 0x8000u);
		a.ref2dev.assign(n, UINT32_MAX);
		a.dev2ref.assign(n, 0);
		uint32_t next = 0;
		a.hot_depth1 = 0;
		for (uint32_t s : a.bfs_order) {
			if (next >= hot_max)
				break;
			if (a.is_final_ref(s))
				continue;
			if (a.depth[s] <= 1)
				a.hot_depth1 = next + 1;
			a.ref2dev[s] = next;
			a.dev2ref[next++] = s;
		}
		a.hot_count = next;
		for (uint32_t s = 0; s < n; s++)
			if (a.ref2dev[s] == UINT32_MAX && !a.is_final_ref(s)) {
				a.ref2dev[s] = next;
				a.dev2ref[next++] = s;
			}
		a.first_final = next;
		for (uint32_t s = 0; s < n; s++)
			if (a.ref2dev[s] == UINT32_MAX) {
				a.ref2dev[s] = next;
				a.dev2ref[next++] = s;
			}
	}

	// dev_run[d]: length of the unary, non-final path d -> d+1 -> d+2 ...
	// Computed right to left over dev ids.
	void unary_runs()
	{
		const uint32_t n = a.num_states;
		a.dev_run.assign(n, 0);
		for (uint32_t d = n; d-- > 0;) {
			if (d + 1 >= a.first_final || d == 0)
				continue;   // the state entered must not be final; the root has no run
			const uint32_t r = a.dev2ref[d], r1 = a.dev2ref[d + 1];
			const bool only_child = a.child_begin[r + 1] - a.child_begin[r] == 1 &&
			    a.child_list[a.child_begin[r]].to == r1;
			if (!only_child)
				continue;
			const uint32_t nx = a.dev_run[d + 1];
			a.dev_run[d] = (uint16_t)(nx >= 65534 ? 65535 : nx + 1);
		}
	}

	// acsm_get_patterns_table's linking pass (acsmx.c:707-721), state ids
	// ascending.  The reference's "walk to the end of q's chain" never ends
	// once two states have linked their patterns into a cycle -- it does so
	// on its own apps/patterns.txt -- so the walk is bounded by the number
	// of patterns and simply stops where it is when it does not terminate.
	void chain_patterns()
	{
		a.next_chained.assign(a.patterns.size(), -1);
		const size_t bound = a.patterns.size();
		for (uint32_t s = 0; s < a.num_states; s++) {
			if (a.list_len[s] < 2)
				continue;
			const int32_t *l = &a.list_pool[a.list_begin[s]];
			int32_t q = l[0];
			for (size_t hops = 0; a.next_chained[q] != -1 && hops < bound; hops++)
				q = a.next_chained[q];
			for (int k = 0; k + 1 < a.list_len[s]; k++) {
				if (l[k + 1] == q)
					break;
				a.next_chained[q] = l[k + 1];
				q = l[k + 1];
			}
		}
	}
};

}  // namespace

extern "C" int acm_automaton_compile(acm_automaton *a)
{
	if (!a)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_compile: null automaton");
	if (a->compiled)
		return ACM_OK;
	if (a->max_pattern_len >= acm::kMaxPatternLine)
		return acm::fail(ACM_ERR_LIMIT, "pattern longer than %d bytes", acm::kMaxPatternLine - 1);
	size_t total = 1;
	for (auto &p : a->patterns)
		total += p.bytes.size();
	if (total > acm::kMaxStates)
		return acm::fail(ACM_ERR_LIMIT, "pattern set may need %zu states (limit %u)", total,
		    acm::kMaxStates);
	try {
		if (!a->want_nocase) {   // per-pattern flags: all flagged is the nocase automaton, some is a mixed one
			size_t flagged = 0, plain = 0;
			for (auto &p : a->patterns)
				if (!p.bytes.empty())
					(p.flags & ACM_PATTERN_NOCASE ? flagged : plain)++;
			a->nocase = flagged > 0;
			a->mixed = flagged > 0 && plain > 0;
		}
		if (a->nocase && a->original.empty()) {   // (not again after a failed compile)
			a->original.resize(a->patterns.size());
			for (size_t i = 0; i < a->patterns.size(); i++) {
				a->original[i] = a->patterns[i].bytes;
				for (unsigned char &c : a->patterns[i].bytes)
					c = (unsigned char)acm::fold_byte(c);
			}
		}
		Builder b(*a);
		b.insert_patterns();
		b.index_children();
		b.link_and_collect();
		b.byte_classes();
		b.number_for_device();
		b.chain_patterns();
		b.unary_runs();
	} catch (const std::bad_alloc &) {
		return acm::fail(ACM_ERR_NOMEM, "out of memory while compiling the automaton");
	}
	a->compiled = true;
	return ACM_OK;
}

// Dense rows in BFS order: row(s) = row(fail(s)) with the trie children of s
// written over it; the root row is all "-> root" plus its children.  fail(s)
// is shallower than s, so its row exists by the time s is reached.  A cell
// carries everything the deep walks need to know about its target.
const std::vector<uint64_t> &acm_automaton::dense_rows() const
{
	if (!dense.empty() || num_states == 0)
		return dense;
	std::vector<uint64_t> cell(num_states);
	for (uint32_t r = 0; r < num_states; r++) {
		const uint32_t d = ref2dev[r];
		cell[r] = (uint64_t)d | ((uint64_t)depth[r] << 32) | ((uint64_t)dev_run[d] << 48);
	}
	dense.assign((size_t)num_states * 256, cell[0]);
	for (uint32_t s : bfs_order) {
		uint64_t *row = &dense[(size_t)ref2dev[s] * 256];
		if (s != 0)
			memcpy(row, &dense[(size_t)ref2dev[fail[s]] * 256], 256 * sizeof(uint64_t));
		for (uint32_t e = child_begin[s]; e < child_begin[s + 1]; e++)
			row[child_list[e].byte] = cell[child_list[e].to];
		if (nocase)   // (the raw-byte planes: a lowercase letter's cell is its uppercase letter's)
			for (uint32_t c = 'a'; c <= 'z'; c++)
				row[c] = row[acm::fold_byte(c)];
	}
	return dense;
}

// ---- accessors -------------------------------------------------------------------

extern "C" int acm_automaton_num_patterns(const acm_automaton *a)
{
	return a ? (int)a->patterns.size() : 0;
}

extern "C" int acm_automaton_max_pattern_len(const acm_automaton *a)
{
	return a ? a->max_pattern_len : 0;
}

extern "C" int acm_automaton_byte_classes(const acm_automaton *a, uint8_t *class_of)
{
	if (!a || !a->compiled)
		return 0;
	if (class_of)
		memcpy(class_of, a->byte_class, 256);
	return (int)a->num_classes;
}

extern "C" int acm_automaton_num_states(const acm_automaton *a)
{
	return (a && a->compiled) ? (int)a->num_states : 0;
}

extern "C" size_t acm_automaton_reference_table_bytes(const acm_automaton *a)
{
	return (a && a->compiled) ? (size_t)a->num_states * 2 * 256 * sizeof(int32_t) : 0;
}

extern "C" int acm_automaton_export_reference_table(const acm_automaton *a, int32_t *dst)
{
	if (!a || !a->compiled || !dst)
		return acm::fail(ACM_ERR_ARG, "export_reference_table: automaton not compiled");
	try {
		const std::vector<uint64_t> &rows = a->dense_rows();
		for (uint32_t s = 0; s < a->num_states; s++) {
			const uint64_t *row = &rows[(size_t)a->ref2dev[s] * 256];
			int32_t *out = dst + (size_t)s * 512;
			for (int c = 0; c < 256; c++) {
				const uint32_t td = (uint32_t)row[c];
				uint32_t t = a->dev2ref[td];
				if (td >= a->first_final) {
					out[c] = -(int32_t)t;
					out[256 + c] = a->head_of(t);
				} else {
					out[c] = (int32_t)t;
					out[256 + c] = 0;
				}
			}
		}
	} catch (const std::bad_alloc &) {
		return acm::fail(ACM_ERR_NOMEM, "out of memory building dense rows");
	}
	return ACM_OK;
}

extern "C" int acm_automaton_pattern(const acm_automaton *a, int index, int *iid, int *n,
    const unsigned char **bytes, int *next_chained)
{
	if (!a || index < 0 || index >= (int)a->patterns.size())
		return acm::fail(ACM_ERR_ARG, "acm_automaton_pattern: index out of range");
	if (iid) *iid = a->patterns[index].iid;
	const std::vector<unsigned char> &src =
	    (size_t)index < a->original.size() ? a->original[index] : a->patterns[index].bytes;
	if (n) *n = (int)src.size();
	if (bytes) *bytes = src.data();
	if (next_chained)
		*next_chained = a->compiled ? a->next_chained[index] : -1;
	return ACM_OK;
}

extern "C" int acm_automaton_state_matches(const acm_automaton *a, int ref_state, int32_t *out, int cap)
{
	if (!a || !a->compiled || ref_state < 0 || (uint32_t)ref_state >= a->num_states || (cap > 0 && !out))
		return -1;
	if (!a->is_final_ref((uint32_t)ref_state))
		return 0;
	const int32_t len = a->list_len[ref_state];
	for (int32_t i = 0; i < len && i < cap; i++)
		out[i] = a->list_pool[(size_t)a->list_begin[ref_state] + i];
	return len;
}

extern "C" int acm_automaton_state_output(const acm_automaton *a, int ref_state)
{
	if (!a || !a->compiled || ref_state < 0 || (uint32_t)ref_state >= a->num_states)
		return -1;
	return a->head_of((uint32_t)ref_state);
}

extern "C" int acm_automaton_state_fail(const acm_automaton *a, int ref_state)
{
	if (!a || !a->compiled || ref_state < 0 || (uint32_t)ref_state >= a->num_states)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_state_fail: automaton not compiled or state out of range");
	return (int)a->fail[ref_state];
}

extern "C" int acm_automaton_state_depth(const acm_automaton *a, int ref_state)
{
	if (!a || !a->compiled || ref_state < 0 || (uint32_t)ref_state >= a->num_states)
		return acm::fail(ACM_ERR_ARG, "acm_automaton_state_depth: automaton not compiled or state out of range");
	return (int)a->depth[ref_state];
}
