// acm_grep -- MI355X-native counterpart of the reference's ocl_aho_grep
// (streaming feeder, CLI + stdout contract,
// directory traversal / multi-file packing).
//
// Same flags, same -v line and STATS block as ocl_aho_grep.c:151-204,
// :272-308, :615-631, so apps/sentiment_analysis.py-style consumers keep
// working.  What is different underneath:
//
//   * each worker (-w) owns one HIP stream and TWO staging buffers: while the
//     GPU copies in and scans buffer A (hipMemcpyAsync from pinned memory ->
//     acm_scan_async -> bucket planes -> async copy back), the worker thread
//     is already read(2)-ing the next bytes into buffer B.  The reference
//     reads, copies and scans strictly one after the other
//     (ocl_aho_grep.c:68-139, blocking CL_TRUE copies + clFinish);
//   * one DFA per device, shared by all workers (the reference uploads a
//     private copy per worker, ocl_worker.c:66,149-153 -- quirk Q12);
//   * matches are those of a serial scan, the state is
//     carried from buffer to buffer of a worker like db->last_state.
//
// Files are dealt to workers as in the reference: worker i takes files
// i, i + w, i + 2w, ... (ocl_aho_grep.c:47,87).
#include <dirent.h>
#include <fcntl.h>
#include <pthread.h>
#include <signal.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "acmatch.h"

namespace {

volatile sig_atomic_t g_terminate = 0;
void on_sigint(int) { g_terminate = 1; }

double now_us()
{
	struct timespec tp;
	clock_gettime(CLOCK_MONOTONIC, &tp);  // utils.c:60-68
	return tp.tv_sec * 1e6 + tp.tv_nsec / 1e3;
}

[[noreturn]] void usage()
{
	printf("\nUsage:\n"
	       "    acm_grep -f file -p file -B chunk_size -D devpos\n"
	       "             -G global_ws -L local_ws [-m max]\n"
	       "             [-w cpu_threads] [-R max] [-I file] [-P file] [-tvxFMAiSWcno]\n"
	       "             [-r file -O dir] [-C N[,M] -T dir [-V]] [-k N] [-z SPEC]\n"
	       "    acm_grep -h\n\n"
	       "Options (those of ocl_aho_grep):\n"
	       "  -f file        input: a file, a directory, or comma-separated files\n"
	       "  -p file        patterns, one per line (plain, \"quoted\", or 'ID pattern')\n"
	       "  -F             keep processing data appended to the inputs (e.g. a FIFO)\n"
	       "  -B chunk_size  chunk size in bytes (result buckets are per chunk)\n"
	       "  -D devpos      HIP device ordinal, or a list (0,1,2,...): worker i runs on entry i mod\n"
	       "                 the list length, each device holds its own copy of the automaton\n"
	       "  -G global_ws   chunks per buffer: buffer = global_ws * chunk_size bytes\n"
	       "  -L local_ws    accepted for compatibility; the launch shape is the library's\n"
	       "  -m max         use at most max bytes of every pattern\n"
	       "  -w threads     feeder threads (default 2)\n"
	       "  -R max         result cells per chunk incl. the counter cell (default 16)\n"
	       "  -v             print every match\n"
	       "  -t             text mode: one chunk per line\n"
	       "  -x             patterns are printable hex\n"
	       "  -M             accepted for compatibility (mapped buffers)\n"
	       "  -A             report every pattern that ends at an offset, not only the one the\n"
	       "                 reference reports (extension; off by default)\n"
	       "  -i             ignore ASCII case in patterns and input (extension; the patterns\n"
	       "                 are folded after -x decoding and the -m cut, -v prints them as written)\n"
	       "  -I file        a second pattern file whose patterns ignore ASCII case, appended after those of -p\n"
	       "                 (pattern indices continue; -x and -m apply to it as to -p).  The patterns of -p stay\n"
	       "                 exact: every buffer's records go through the case pass on the device before they\n"
	       "                 are bucketed, printed, counted (-c) or numbered (-n).  With -i it is a second -p\n"
	       "                 (extension; not with -W or -F)\n"
	       "  -P file        position constraints, one per line: '<pattern index> <lo> <hi or *> [end]' -- the pattern\n"
	       "                 may start lo..hi bytes into its text, with 'end' lo..hi bytes in front of its end\n"
	       "                 ('^': 0 0; '$' for a pattern of L bytes: L L end).  Indices count the patterns of -p, then\n"
	       "                 those of -I.  Needs -S: the texts are the files (with -t: the lines).  Composes with -A,\n"
	       "                 -i, -c, -n and with -W or -I.  An end-anchored candidate in a file that goes on in the\n"
	       "                 next buffer cannot be decided: it is counted and reported as an error at exit\n"
	       "                 (extension; not with -F)\n"
	       "  -Q file        multi-part signatures, one per line: a ClamAV-style hex body (hex byte pairs, ??, *, {n},\n"
	       "                 {n-m}, {-m}, {n-}) with an optional leading '<decimal id>:'.  Instead of -p or beside it (the\n"
	       "                 patterns of -p and -I come first).  The matches printed and counted are then those of the\n"
	       "                 signatures, joined on the device: the -v line names the signature's id and the offset its\n"
	       "                 last part ends at.  A signature lies in one buffer and, with -S, in one file.  The pass\n"
	       "                 orders one cell per byte of a buffer, at most 4 Mi (36 bytes of device memory each, per\n"
	       "                 buffer): a buffer with more pattern records than that is an error.  Composes with\n"
	       "                 -i, -I, -S and -P (the indices of the parts follow those of -p and -I)\n"
	       "                 (extension; not with -c, -n, -W or -A)\n"
	       "  -E             the signatures of -Q in the extended syntax: beside hex byte pairs a position may be a\n"
	       "                 nibble wildcard (a?, ?a), any byte (??, a position here, not a gap of one), one of some bytes\n"
	       "                 ((aa|bb|cc)) or none of them (!(aa|bb)); only * and {..} separate parts, and every part\n"
	       "                 needs an exact byte.  The longest run of exact bytes of a part is matched by the automaton,\n"
	       "                 the positions around it are checked on the device where it matched.  A candidate whose\n"
	       "                 positions reach over a buffer border is not decided: such candidates are counted and\n"
	       "                 reported on stderr at exit.  Composes with -i, -I, -S and -P (a window counts from a part's\n"
	       "                 first position) (extension; needs -Q or -K, not with -W)\n"
	       "  -X             with -E: alternatives may be of more than one byte, (aabb|ccdd) and !(aabb|ccdd), all\n"
	       "                 alternatives of one group of one width (at most 32 bytes, 256 alternatives, 16 groups a part).\n"
	       "                 The group is checked on the device where the part's exact run and its other positions\n"
	       "                 held.  For the files of -Q and -K; composes and refuses as -E does (extension; needs -E)\n"
	       "  -K file        rules, one logical signature per line: 'expr;body0;body1;...' with an optional leading\n"
	       "                 '<decimal id>:' -- a ClamAV .ldb line without its name and target fields.  A body is a\n"
	       "                 signature as -Q takes it (with -E: in the extended syntax); expr is a condition over the\n"
	       "                 bodies' hits in ONE text, operand j being body j: '&' and '|' (never mixed at one level\n"
	       "                 without parentheses), '(..)' and '=n', '>n', '<n' behind an operand or a group, whose count\n"
	       "                 is the sum of its operands' hits: '(0&1)|2>3', '0&1=0'.  Needs -S: the texts are the files\n"
	       "                 (with -t: the lines).  Beside or instead of -p / -Q.  The conditions are evaluated on the\n"
	       "                 device; what is printed and counted are the rules that hold: the -v line is \"Rule <id>\n"
	       "                 matched in file '<path>' [text at offset <t>]\", t the text's start in its file.  A text\n"
	       "                 cut by a buffer is NOT evaluated -- the text a buffer begins in the middle of, and a\n"
	       "                 buffer's last text when its file goes on: the number of such texts is printed on stderr\n"
	       "                 at exit; use a larger -G/-B.  The pass orders the same cells as -Q.  Composes with -i, -I,\n"
	       "                 -P, -E and -t (extension; not with -c, -n, -W, -A or -F)\n"
	       "  -S             every input unit is its own text: a file, or with -t a line; no match\n"
	       "                 spans two of them (extension; data appended under -F continues its file\n"
	       "                 when the worker's previous chunk came from the same file)\n"
	       "  -W             whole words only (grep -w): a pattern counts where the bytes around it\n"
	       "                 are not in [0-9A-Za-z_] or are a text start or end; with -A every such\n"
	       "                 pattern, else the first of the match list (extension; not with -F)\n"
	       "  -c             exact counts of the records the run reports, tallied on the device and not\n"
	       "                 limited by -R (extension): after the workers have finished, one line\n"
	       "                 \"Count file '<path>': <n>\" per input file and one line\n"
	       "                 \"Count pattern <id> ('<bytes>'): <n>\" per pattern with n > 0; a record\n"
	       "                 belongs to the file that holds its last byte\n"
	       "  -n             line numbers (grep -n, extension; binary mode only): the lines of every buffer are\n"
	       "                 found on the device, the -v line becomes \"... found in file '<path>' at line <l>\n"
	       "                 offset <o> [relative: <r>]\" with the 1-based line number of the match's last byte\n"
	       "                 in its file, and STATS gains \"Processed lines\", the newlines counted on the device\n"
	       "  -o             only the leftmost-longest non-overlapping matches (grep -o over the pattern list): of\n"
	       "                 every pattern that ends somewhere -- the records -A would print -- the one that starts\n"
	       "                 first, the longest of those, the first added of equals, then the next behind its end;\n"
	       "                 selected on the device, one -v line per selected match, and the matches counted are the\n"
	       "                 selected ones.  A match that began in the buffer in front is no candidate: such entries\n"
	       "                 are counted and reported on stderr at exit; use a larger -G/-B.  Composes with -i, -S,\n"
	       "                 -W, -I and -P (extension; not with -A, -c, -n, -Q, -K, -E or -F)\n"
	       "  -r file        rewrite: replacements, one per line: '<pattern index> <hex bytes or empty>' -- a match of the\n"
	       "                 pattern becomes those bytes (none: it is deleted) -- or '<pattern index> fill <hh>' -- every\n"
	       "                 byte of the match becomes hh (a mask).  Indices count the patterns of -p, then those of -I; a\n"
	       "                 pattern without a line is matched and left as it is.  Runs what -o runs (-o is implied: the\n"
	       "                 same matches, lines and counts), then splices every buffer on the device and writes each\n"
	       "                 input file, rewritten, under the directory of -O.  A file cut by -G is rewritten piece by\n"
	       "                 piece: a match across the cut is not rewritten (the NOTE of -o counts those).  A buffer whose\n"
	       "                 output outgrows twice its input is an error.  Composes as -o does (extension; needs -O; not\n"
	       "                 with -t, -A, -c, -n, -Q, -K, -E or -F)\n"
	       "  -O dir         with -r: where the rewritten files go: dir/<name> for every file of a directory or list\n"
	       "                 given with -f; directories are made as needed.  Two inputs of one name, and an output that\n"
	       "                 is one of the inputs, are refused\n"
	       "  -C N[,M]       extract lines (grep -C, extension; binary mode only): every line that holds a record the run\n"
	       "                 reports, with N lines of context in front of it and M behind it (-C N: N on both sides;\n"
	       "                 -C 0: the matching lines only).  Overlapping and adjacent contexts merge into one group, the\n"
	       "                 groups of a file are separated by a line \"--\" when N + M > 0, and context never crosses into\n"
	       "                 another file.  The lines of every buffer are found, selected and packed on the device; each\n"
	       "                 input file's lines go to a file under the directory of -T (a file without a selected line\n"
	       "                 gets an empty one), a last line without a newline gets one.  stdout is what the run without\n"
	       "                 -C prints.  Context is not continued across buffers: a file that -G cuts is an error that\n"
	       "                 names it; use a larger -G/-B.  Composes with -A, -i, -S, -W, -I, -P, -o, -c and -n\n"
	       "                 (extension; needs -T; not with -t, -F, -r, -O, -Q or -K)\n"
	       "  -V             with -C: the lines that hold NO record are the selected ones (grep -v)\n"
	       "  -T dir         with -C: where the extracted lines go: dir/<name> for every file of a directory or list given\n"
	       "                 with -f, named and refused as -O names and refuses them\n"
	       "  -H             with -C and -T: the file's name and ':' in front of every selected line, the name and '-' in front\n"
	       "                 of every context line (grep -H).  The name is the path of the input file as -f resolved it\n"
	       "  -N             with -C and -T: the line's number in its file, from 1, and the same separator (grep -n; -n keeps\n"
	       "                 its meaning here: the line of every record on stdout)\n"
	       "  -b             with -C and -T: the offset of the line's first byte in its file and the same separator (grep -b).\n"
	       "                 With any of the three the per-line context pass and the format pass run in the place of the\n"
	       "                 group pass and the extract, all on the device; -H -N -b together print name:line:offset:.  The\n"
	       "                 output buffer is sized for lines of four bytes or more on average; a buffer whose output does\n"
	       "                 not fit is an error that says so (extensions; they work with -V; each needs -C and -T)\n"
	       "  -k N           approximate matching, 1 <= N <= 15: every pattern of -p and -I that has at least 3 * (N + 1) bytes\n"
	       "                 after -x and -m also matches where up to N of its bytes are other bytes (substitutions only: the\n"
	       "                 match has the pattern's length).  Such a pattern is cut into N + 1 pieces of 3 bytes or more; the\n"
	       "                 pieces are matched by the automaton and the mismatches counted on the device where a piece\n"
	       "                 matched.  Shorter patterns stay exact; their number is a NOTE on stderr.  Every pattern that ends\n"
	       "                 at an offset is reported, as with -A.  The -v line names the pattern as written and the offset its\n"
	       "                 whole span ends at, the number a run without -k prints for an exact match, and ends in\n"
	       "                 ' mismatches <d>'.  A line is printed where the piece that found the match ends: the lines of one\n"
	       "                 buffer may come out of offset order by up to the length of the longest pattern.  The pass is\n"
	       "                 given the tail of the buffer in front; a candidate whose span reaches behind the buffer's end is\n"
	       "                 not decided: such candidates are counted and reported on stderr at exit.  Composes with -i, -I,\n"
	       "                 -S and -t (extension; not with -W, -P, -Q, -K, -E, -o, -r, -c, -n, -C or -F)\n"
	       "  -e             with -k N, N <= 4: edit distance, agrep's -k.  The N errors may be inserted and deleted bytes as well\n"
	       "                 as substituted ones, so a match may be up to N bytes shorter or longer than its pattern.  The same\n"
	       "                 patterns are cut into the same pieces; where a piece matched, a banded dynamic program on the\n"
	       "                 device finds the nearest end within N errors and the shortest span that has that distance.  A\n"
	       "                 match is reported once per (pattern, end), in offset order, and its neighbouring ends within\n"
	       "                 the budget are reported only where another piece chose them.  The -v line ends in\n"
	       "                 ' edits <d> length <l>'.  Composes with and refuses what -k does, and with -c, which counts the\n"
	       "                 unique records (extension)\n"
	       "  -z SPEC        match against a normalised view of the input: SPEC is a comma list of 'url' (a %%XX triple counts as\n"
	       "                 the byte it encodes, decoded once) and at most one of 'ws' (a run of tab, LF, VT, FF, CR and space\n"
	       "                 counts as one space), 'strip' (those bytes do not count at all) and 'nul' (NUL bytes do not count:\n"
	       "                 UTF-16LE text of ASCII reads as ASCII).  Every buffer is normalised on the device, each text alone;\n"
	       "                 the scan and the passes of -W, -I and -A run on the normalised bytes, and every record is mapped\n"
	       "                 back: offsets and counts are those of the file as it is, a match that ends in a triple ends on the\n"
	       "                 triple's last digit, one that ends in a squeezed run on the run's first byte.  Needs -S: the\n"
	       "                 texts are the files (with -t: the lines); a file that a buffer cuts is normalised piece by piece,\n"
	       "                 and with -W the word test at such a cut sees the next piece's first byte as it is in the file,\n"
	       "                 not as it would be normalised: use a -G/-B that holds every file whole.\n"
	       "                 Composes with -x, -i, -I, -A, -W, -c, -v, -w, -D and -R (extension; not with -n, -C, -T, -o, -r,\n"
	       "                 -O, -H, -N, -b, -k, -e, -P, -Q, -K, -E, -X, -V or -F)\n"
	       "  -h             this help\n");
	exit(EXIT_FAILURE);
}

bool is_dir(const std::string &p)
{
	struct stat st;
	return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}

bool is_readable_input(const std::string &p)
{
	struct stat st;
	return stat(p.c_str(), &st) == 0 && (S_ISREG(st.st_mode) || S_ISFIFO(st.st_mode));
}

// file_traverse.c:107-166: regular files directly under dir (not recursive)
std::vector<std::string> regular_files_in(std::string dir)
{
	std::vector<std::string> out;
	if (!dir.empty() && dir.back() == '/')
		dir.pop_back();
	DIR *d = opendir(dir.c_str());
	if (!d)
		return out;
	while (struct dirent *e = readdir(d)) {
		if (e->d_type == DT_DIR)
			continue;
		std::string f = dir + "/" + e->d_name;
		struct stat st;
		if (stat(f.c_str(), &st) == 0 && S_ISREG(st.st_mode))
			out.push_back(f);
	}
	closedir(d);
	return out;
}

struct Config {
	std::string pat_path, data_path, loose_path, pos_path, seq_path, rule_path;   // loose_path: -I, pos_path: -P, seq_path: -Q, rule_path: -K
	std::string repl_path, out_dir;   // -r, -O
	std::string ext_dir;     // -T
	int ctx = 0, ctx_before = 0, ctx_after = 0, invert = 0;   // -C N[,M], -V
	int fmt_name = 0, fmt_num = 0, fmt_off = 0;   // -H, -N, -b
	int fmt = 0;             // any of them: the per-line context pass and the format pass take the place of the group pass and the extract
	size_t fmt_width = 0;    // the longest prefix a line can get: the longest input path, the digits and the separators
	int extract = 0;         // -C and -T: the selected lines and their context are packed on the device and the files written
	int rewrite = 0;         // -r: the selected matches are replaced on the device and the rewritten files written (only is set too)
	int dev = -1, hex = 0, verbose = 0, text_mode = 0, follow = 0, threads = 2, all_patterns = 0, nocase = 0, segmented = 0,
	    words = 0, count = 0, lineno = 0;
	int cased = 0;           // -I without -i: the records go through the case pass
	int pos = 0;             // -P: the records go through the position pass
	int seq = 0;             // -Q: every pattern of the records goes through the sequence pass; its records are reported
	int grp = 0;             // -X: with -E, alternatives of more than one byte
	int ext = 0;             // -E: the signatures of -Q and the bodies of -K are read in the extended syntax
	int rules = 0;           // -K: the sequence pass's records go through the rule pass; its records are reported (seq is set too)
	int wild = 0;            // -E and some part has a context: the parts' records go through the wildcard pass
	int edit = 0;            // -e: the patterns of -k are edit patterns, verified by the edit pass in the approx pass's place
	int approx = 0;          // -k N: the budget; every pattern's records go through the approx pass (all_patterns is set too)
	int only = 0;            // -o: every pattern of the records goes through the select pass (all_patterns is set too)
	std::string norm_spec;   // -z
	int norm = 0;            // -z: every buffer is normalised on the device, scanned normalised, its records mapped back
	unsigned norm_flags = 0; // ACM_NORM_*
	int norm_nul = 0;        // -z nul: the blank set is {00}
	std::vector<int> devs;   // -D 0,1,...: worker i runs on devs[i % devs.size()] (the reference has one -D)
	int max_results = MAX_RESULTS, pat_limit = -1;
	long global_ws = -1, local_ws = -1, chunk = -1;
};

struct Shared {
	Config cfg;
	std::vector<acm_dfa *> dfas;   // one per entry of cfg.devs
	std::vector<std::string> files;
	std::vector<int> fds;
	std::vector<std::string> pat_bytes;   // for the -v line
	std::vector<int> pat_iid;
	std::vector<int> seq_iid;             // -Q: the id of every sequence, for the -v line
	std::vector<int> seq_post;            // -E: the post context of every sequence's last part: a match ends that far behind its record
	std::vector<int> rule_iid;            // -K: the id of every rule, for the -v line
	std::vector<int> apx_post;            // -k: per pattern, how far behind a piece's end its whole pattern ends (a plain pattern: 0)
	int apx_back = 0;                     // -k: the longest approximate pattern: the tail of its stream a worker keeps
	std::vector<std::string> out_paths;   // -r: where every input file's rewrite goes
	std::vector<char> out_begun;          // -r: the file has been created in this run (a file belongs to one worker)
	int max_pattern_len = 0;
	pthread_mutex_t print_lock = PTHREAD_MUTEX_INITIALIZER;
	pthread_barrier_t ready;   // workers have their buffers; the clock starts (the reference
	                           // also allocates in ocl_worker_ctx_init, before start_time)
};

// -Q: the pattern records of one buffer the sequence pass takes.  The pass keys and orders that many cells for
// every buffer, however few records it holds, in 36 bytes of workspace each: a buffer with more is an error
constexpr size_t kSeqMaxRecords = (size_t)4 << 20;
constexpr size_t kAllFactor = 4;   // -A: records the expanded planes hold per text byte

struct Buffer {   // one of the two staging buffers of a worker
	unsigned char *h_data = nullptr;
	int32_t *h_indices = nullptr, *h_sizes = nullptr, *file_ids = nullptr;
	int32_t *h_results = nullptr, *h_results2 = nullptr;
	void *d_data = nullptr, *d_indices = nullptr, *d_sizes = nullptr, *d_starts = nullptr;
	void *d_results = nullptr, *d_results2 = nullptr, *d_pat = nullptr, *d_off = nullptr;
	void *d_pat_all = nullptr, *d_off_all = nullptr, *d_expand_ws = nullptr;   // -A only
	size_t all_cap = 0;          // cells of the -A planes
	int32_t *h_all_count = nullptr;   // pinned: records the expansion produced
	size_t expand_ws_bytes = 0;
	void *d_seg_pat = nullptr, *d_seg_off = nullptr, *d_seg_start = nullptr, *d_seg_ws = nullptr;   // -S only
	size_t seg_ws_bytes = 0;
	std::vector<int32_t> seg_starts;   // -S: stream offsets where a file (-t: a line) begins
	const int32_t *end_plane = nullptr;   // plane whose trailer holds the state the next buffer starts in
	void *d_word_pat = nullptr, *d_word_off = nullptr, *d_word_ws = nullptr;   // -W only
	size_t word_ws_bytes = 0;
	void *d_case_pat = nullptr, *d_case_off = nullptr, *d_case_ws = nullptr;   // -I only
	size_t case_ws_bytes = 0;
	// -P only: the position pass's planes, workspace and info (pinned twin: [0] = undecided entries dropped)
	void *d_pos_pat = nullptr, *d_pos_off = nullptr, *d_pos_ws = nullptr, *d_pos_info = nullptr;
	int32_t *h_pos_info = nullptr;
	size_t pos_ws_bytes = 0, pos_cap = 0;
	// -Q only: the sequence pass's planes, workspace and info; seq_max: the pattern-form records it takes
	void *d_seq_pat = nullptr, *d_seq_off = nullptr, *d_seq_ws = nullptr, *d_seq_info = nullptr;
	size_t seq_ws_bytes = 0, seq_max = 0;
	// -K only: the rule pass's planes (rule, text, offset: seq_max + 2 cells each), workspace and info; the pinned
	// count, and the records as collect() copies them back
	void *d_rule_out = nullptr, *d_rule_text = nullptr, *d_rule_off = nullptr, *d_rule_ws = nullptr, *d_rule_info = nullptr;
	int32_t *h_rule_count = nullptr;
	std::vector<int32_t> h_rule, h_rule_text;
	size_t rule_ws_bytes = 0;
	std::vector<long> file_off;  // -K: where every chunk begins in its file
	// -E only: the wildcard pass's planes, workspace and info (pinned twin: [0] = undecided entries, [4] = records written)
	void *d_wild_pat = nullptr, *d_wild_off = nullptr, *d_wild_ws = nullptr, *d_wild_info = nullptr;
	int32_t *h_wild_info = nullptr;
	size_t wild_ws_bytes = 0;
	// -k only: the approx pass's planes (patterns, offsets, distances), workspace and info (pinned twin: [0] = undecided
	// entries); the distances go through the buckets into d_results3 as the lines of -n do
	// -e: the edit pass in its place, with a length plane that goes through the buckets into d_results4
	void *d_apx_pat = nullptr, *d_apx_off = nullptr, *d_apx_dist = nullptr, *d_apx_ws = nullptr, *d_apx_info = nullptr;
	void *d_apx_len = nullptr, *d_results4 = nullptr;
	int32_t *h_results4 = nullptr;
	int32_t *h_apx_info = nullptr;
	size_t apx_ws_bytes = 0;
	// -o only: the select pass's planes, workspace and info (pinned twin: [1] = entries that began in front of the buffer)
	void *d_sel_pat = nullptr, *d_sel_off = nullptr, *d_sel_ws = nullptr, *d_sel_info = nullptr;
	int32_t *h_sel_info = nullptr;
	size_t sel_ws_bytes = 0;
	// -r only: the rewrite pass's output, workspace and info, the stream offsets where another file begins and where
	// those lie in the output; pinned twins.  rw_cap: the bytes the output may have
	void *d_rw_out = nullptr, *d_rw_ws = nullptr, *d_rw_info = nullptr, *d_rw_start = nullptr, *d_rw_seg = nullptr;
	int32_t *h_rw_info = nullptr, *h_rw_seg = nullptr;
	unsigned char *h_rw_out = nullptr;
	size_t rw_ws_bytes = 0, rw_cap = 0, rw_max = 0;
	std::vector<int32_t> rw_starts, rw_files;
	// -C only: the line starts of this buffer's stream (indexed over d_ex_text when a file in it does not end in a
	// newline: the stream with one on that file's last byte, so that every file start is a line start), the context
	// pass's planes and figures, the extract's output, figures and the output in front of every file; pinned twins
	void *d_ex_lines = nullptr, *d_ex_line_info = nullptr, *d_ex_ws = nullptr, *d_ex_text = nullptr, *d_ex_rel = nullptr,
	     *d_ex_begin = nullptr, *d_ex_next = nullptr, *d_ex_ctx_info = nullptr, *d_ex_out = nullptr, *d_ex_info = nullptr,
	     *d_ex_seg = nullptr;
	// -H, -N, -b: the kind of every kept line, the names of this buffer's files (text id 0, in front of the first start,
	// has none) and where each lies, the lines in front of every file
	void *d_ex_kind = nullptr, *d_ex_names = nullptr, *d_ex_name_off = nullptr, *d_ex_seg_num = nullptr;
	std::vector<uint8_t> ex_names;
	std::vector<int32_t> ex_name_off;
	int32_t *h_ex_info = nullptr, *h_ex_seg = nullptr;
	unsigned char *h_ex_out = nullptr;
	size_t ex_ws_bytes = 0, ex_cap = 0, ex_lcap = 0;
	long lead_begin = 0;         // -P, -Q: where the text that goes on into this buffer began, in its stream's coordinates (<= 0)
	bool end_known = false;      // -P: the stream's last text ends with the stream (its file, or with -t its line, is finished)
	bool last_of_input = false;  // -P: nothing of the worker's input follows this buffer
	int32_t end_start = 0;       // -P: the start behind the last text when end_known (copied from here)
	// -c only: the grid of file starts of this buffer's stream, the counts per start, of the records in front
	// of the first start (they belong to cnt_prev_file) and of the whole buffer, and their pinned host twins
	void *d_cnt_start = nullptr, *d_cnt_rows = nullptr, *d_cnt_lead = nullptr, *d_cnt_total = nullptr, *d_cnt_ws = nullptr;
	int32_t *h_cnt_rows = nullptr, *h_cnt_lead = nullptr;
	uint64_t *h_cnt_total = nullptr;
	size_t cnt_ws_bytes = 0;
	std::vector<int32_t> cnt_starts, cnt_files;   // stream offset and file of every start
	int cnt_prev_file = -1;      // file of the worker's last chunk in front of this buffer
	// -n only: the line starts of this buffer's stream and their info, the delimiters in front of every record
	// (a plane in the records' layout, bucketed like the patterns) and in front of every file start
	void *d_line_start = nullptr, *d_line_info = nullptr, *d_line_ws = nullptr, *d_line_plane = nullptr, *d_results3 = nullptr,
	     *d_results3_off = nullptr, *d_start_line = nullptr;   // (d_results3_off: the bucket pass's second output, not read)
	int32_t *h_results3 = nullptr, *h_start_line = nullptr, *h_line_info = nullptr;
	size_t line_ws_bytes = 0;
	const void *text = nullptr;  // the buffer's stream on the device (d_data, or d_packed)
	size_t stream_len = 0;
	// -z only: the normalised stream, the map back (keep words, block cells), where every text of seg_starts begins in
	// it, the figures and their pinned twin ([0]: its length); the scan and the word and case passes read scan_text
	void *d_nz_out = nullptr, *d_nz_keep = nullptr, *d_nz_block = nullptr, *d_nz_seg = nullptr, *d_nz_info = nullptr,
	     *d_nz_rinfo = nullptr, *d_nz_ws = nullptr;
	int32_t *h_nz_info = nullptr;
	size_t nz_ws_bytes = 0;
	const void *scan_text = nullptr;      // what is scanned: text, or with -z the normalised stream
	size_t scan_len = 0;
	const int32_t *scan_seg = nullptr;    // the text starts in scan_text: d_seg_start, or with -z d_nz_seg
	bool packed = true;          // the chunks lie back to back in h_data: no offset remapping
	int32_t *rec_pat = nullptr, *rec_off = nullptr;   // the scan's (or segment pass's) planes, for finish()
	void *d_packed = nullptr;
	size_t chunks = 0, bytes = 0;
	std::vector<int32_t> starts;
	void *done = nullptr;        // event behind the buffer's last copy: collect() waits for this buffer, not for the stream
	size_t scan_cap = 0;         // capacity its scan's planes were given (the next buffer reads its final state from them)
};

struct Worker {
	acm_dfa *dfa = nullptr;   // the copy on this worker's device
	int dev = 0;
	Shared *sh = nullptr;
	int id = 0;
	pthread_t thread{};
	void *stream = nullptr, *ws = nullptr;
	size_t ws_bytes = 0;
	Buffer buf[2];
	long last_state = 0;
	int seg_file = -1;        // -S: file of the last chunk submitted
	bool seg_open = false;    // -S -t: that chunk ended inside a line
	size_t text_bytes = 0;    // -P: bytes of the text in progress that the buffers prepared so far hold
	bool file_closed = false; // -P: the file of the last chunk filled has been read to its end
	uint64_t undecided = 0;   // -P: end-anchored entries dropped because their text went on in the next buffer
	uint64_t wild_undecided = 0;   // -E: candidates whose positions reach over a buffer border
	uint64_t apx_undecided = 0;    // -k: candidates whose span reaches behind a buffer's end
	void *d_atail[2] = { nullptr, nullptr };   // -k: the last apx_back bytes of the stream so far, ping-pong
	int atail_cur = 0;
	size_t atail_len = 0;
	uint64_t cut_texts = 0;   // -K: texts that go on in the next buffer: not evaluated
	uint64_t sel_dropped = 0; // -o: entries that began in the buffer in front: no candidates
	long file_pos = 0;        // -K: bytes of the file being read that the buffers filled so far hold
	void *d_tail[2] = { nullptr, nullptr };   // -W, -I: the last max_pattern_len bytes of the stream so far, ping-pong
	int tail_cur = 0;
	size_t tail_len = 0;
	int cnt_file = -1;        // -c, -n: file of the last chunk prepared
	int ex_file = -1;         // -C: file of the last chunk prepared
	const int32_t *line_prev_info = nullptr;   // -n: d_line_info of the buffer indexed last
	uint64_t line_carry = 0;  // -n: newlines of the file the last collected buffer ended in, up to that buffer's end
	void *d_pat_total = nullptr, *d_one_class = nullptr;   // -c: uint64 per pattern, summed over the buffers on the device; a map of every pattern to class 0
	std::vector<uint64_t> pat_total, file_total;            // -c: the worker's counts per pattern (at its end) and per file
	size_t matches = 0, reported = 0, bytes = 0, lines = 0, rounds = 0;
};

void die_acm(const char *what)
{
	fprintf(stderr, "ERROR: %s: %s\n", what, acm_last_error());
	exit(1);
}

#define CK(call) do { if ((call) != ACM_OK) die_acm(#call); } while (0)

void buffer_alloc(Buffer &b, const Config &c, void *stream)
{
	const size_t size = (size_t)c.global_ws * c.chunk, G = (size_t)c.global_ws;
	const size_t plane = ((size_t)c.max_results * G + 1) * 4;
	CK(acm_rt_host_alloc((void **)&b.h_data, size + 32));
	CK(acm_rt_host_alloc((void **)&b.h_indices, (G + 1) * 4));
	CK(acm_rt_host_alloc((void **)&b.h_sizes, (G + 1) * 4));
	CK(acm_rt_host_alloc((void **)&b.h_results, plane));
	CK(acm_rt_host_alloc((void **)&b.h_results2, plane));
	b.file_ids = (int32_t *)calloc(G + 1, 4);
	CK(acm_rt_malloc(&b.d_data, size + 32));
	CK(acm_rt_malloc(&b.d_packed, size + 32));
	CK(acm_rt_malloc(&b.d_indices, (G + 1) * 4));
	CK(acm_rt_malloc(&b.d_sizes, (G + 1) * 4));
	CK(acm_rt_malloc(&b.d_starts, (G + 2) * 4));
	CK(acm_rt_malloc(&b.d_results, plane));
	CK(acm_rt_malloc(&b.d_results2, plane));
	CK(acm_rt_malloc(&b.d_pat, (size + 2) * 4));
	CK(acm_rt_malloc(&b.d_off, (size + 2) * 4));
	if (c.segmented) {
		b.seg_ws_bytes = acm_segment_workspace_bytes(size);
		CK(acm_rt_malloc(&b.d_seg_pat, (size + 2) * 4));
		CK(acm_rt_malloc(&b.d_seg_off, (size + 2) * 4));
		CK(acm_rt_malloc(&b.d_seg_start, (G + 1) * 4));
		CK(acm_rt_malloc(&b.d_seg_ws, b.seg_ws_bytes));
	}
	if (c.norm) {
		b.nz_ws_bytes = acm_normalize_workspace_bytes(size, G + 1);
		CK(acm_rt_malloc(&b.d_nz_out, size + 32));
		CK(acm_rt_malloc(&b.d_nz_keep, (size / 64 + 2) * 8));
		CK(acm_rt_malloc(&b.d_nz_block, (size / ACM_NORM_BLOCK + 3) * 4));
		CK(acm_rt_malloc(&b.d_nz_seg, (G + 1) * 4));
		CK(acm_rt_malloc(&b.d_nz_info, 32));
		CK(acm_rt_malloc(&b.d_nz_rinfo, 32));
		CK(acm_rt_malloc(&b.d_nz_ws, b.nz_ws_bytes));
		CK(acm_rt_host_alloc((void **)&b.h_nz_info, 64));
	}
	if (c.words) {
		b.word_ws_bytes = acm_word_workspace_bytes(size);
		CK(acm_rt_malloc(&b.d_word_pat, (size + 2) * 4));
		CK(acm_rt_malloc(&b.d_word_off, (size + 2) * 4));
		CK(acm_rt_malloc(&b.d_word_ws, b.word_ws_bytes));
	}
	if (c.cased) {
		b.case_ws_bytes = acm_case_workspace_bytes(size);
		CK(acm_rt_malloc(&b.d_case_pat, (size + 2) * 4));
		CK(acm_rt_malloc(&b.d_case_off, (size + 2) * 4));
		CK(acm_rt_malloc(&b.d_case_ws, b.case_ws_bytes));
	}
	if (c.lineno) {
		const size_t cells = c.all_patterns ? size * kAllFactor + 2 : size + 2;
		b.line_ws_bytes = acm_line_index_workspace_bytes(size);
		CK(acm_rt_malloc(&b.d_line_start, (size + 1) * 4));
		CK(acm_rt_malloc(&b.d_line_info, 32));
		CK(acm_rt_malloc(&b.d_line_ws, b.line_ws_bytes));
		CK(acm_rt_malloc(&b.d_line_plane, cells * 4));
		CK(acm_rt_malloc(&b.d_results3, plane));
		CK(acm_rt_malloc(&b.d_results3_off, plane));
		CK(acm_rt_memset(b.d_line_plane, 0, cells * 4, stream));   // cells behind the records, the trailer among them, stay 0
		CK(acm_rt_malloc(&b.d_start_line, (G + 1) * 4));
		CK(acm_rt_host_alloc((void **)&b.h_results3, plane));
		CK(acm_rt_host_alloc((void **)&b.h_start_line, (G + 1) * 4));
		CK(acm_rt_host_alloc((void **)&b.h_line_info, 64));
	}
	if (c.count || c.lineno)
		CK(acm_rt_malloc(&b.d_cnt_start, (G + 1) * 4));
	if (c.count) {
		b.cnt_ws_bytes = acm_tally_workspace_bytes(size * kAllFactor, 1);
		CK(acm_rt_malloc(&b.d_cnt_rows, (G + 1) * 4));
		CK(acm_rt_malloc(&b.d_cnt_lead, 16));
		CK(acm_rt_malloc(&b.d_cnt_total, 16));
		CK(acm_rt_malloc(&b.d_cnt_ws, b.cnt_ws_bytes));
		CK(acm_rt_host_alloc((void **)&b.h_cnt_rows, (G + 1) * 4));
		CK(acm_rt_host_alloc((void **)&b.h_cnt_lead, 64));
		CK(acm_rt_host_alloc((void **)&b.h_cnt_total, 64));
	}
	if (c.pos) {
		b.pos_cap = (c.all_patterns || c.seq) ? size * kAllFactor + 2 : size + 2;
		b.pos_ws_bytes = acm_position_workspace_bytes(size * kAllFactor);
		CK(acm_rt_malloc(&b.d_pos_pat, b.pos_cap * 4));
		CK(acm_rt_malloc(&b.d_pos_off, b.pos_cap * 4));
		CK(acm_rt_malloc(&b.d_pos_ws, b.pos_ws_bytes));
		CK(acm_rt_malloc(&b.d_pos_info, 16));
		CK(acm_rt_host_alloc((void **)&b.h_pos_info, 64));
		b.h_pos_info[0] = 0;
	}
	if (c.all_patterns || c.seq || (c.pos && (c.words || c.cased))) {   // (-P: the word or case pass hands every kept pattern on; -Q takes every pattern)
		b.expand_ws_bytes = acm_expand_workspace_bytes(size);
		// every pattern of every final state's list: more records than text bytes when patterns nest
		// (aaa, aaaa, aaaaa over a run of a's); the planes hold kAllFactor per byte, beyond that the
		// buffer is reported as an error (collect), never overrun
		b.all_cap = size * kAllFactor + 2;
		CK(acm_rt_host_alloc((void **)&b.h_all_count, 64));
		*b.h_all_count = 0;
		CK(acm_rt_malloc(&b.d_pat_all, b.all_cap * 4));
		CK(acm_rt_malloc(&b.d_off_all, b.all_cap * 4));
		CK(acm_rt_malloc(&b.d_expand_ws, b.expand_ws_bytes));
	}
	if (c.approx) {   // (no more kept entries than entries: the planes in front hold all_cap cells)
		CK(acm_rt_malloc(&b.d_apx_pat, b.all_cap * 4));
		CK(acm_rt_malloc(&b.d_apx_off, b.all_cap * 4));
		CK(acm_rt_malloc(&b.d_apx_dist, b.all_cap * 4));
		if (c.edit) {   // (the workspace depends on the uploaded set: worker_main)
			CK(acm_rt_malloc(&b.d_apx_len, b.all_cap * 4));
			CK(acm_rt_malloc(&b.d_results4, plane));
			CK(acm_rt_host_alloc((void **)&b.h_results4, plane));
		} else {
			b.apx_ws_bytes = acm_approx_workspace_bytes(b.all_cap);
			CK(acm_rt_malloc(&b.d_apx_ws, b.apx_ws_bytes));
		}
		CK(acm_rt_malloc(&b.d_apx_info, 16));
		CK(acm_rt_host_alloc((void **)&b.h_apx_info, 64));
		b.h_apx_info[0] = 0;
		CK(acm_rt_malloc(&b.d_results3, plane));
		CK(acm_rt_malloc(&b.d_results3_off, plane));
		CK(acm_rt_host_alloc((void **)&b.h_results3, plane));
	}
	if (c.only) {   // (the planes in front hold all_cap cells, the position pass's as many)
		b.sel_ws_bytes = acm_select_workspace_bytes(b.all_cap - 2);
		CK(acm_rt_malloc(&b.d_sel_pat, b.all_cap * 4));
		CK(acm_rt_malloc(&b.d_sel_off, b.all_cap * 4));
		CK(acm_rt_malloc(&b.d_sel_ws, b.sel_ws_bytes));
		CK(acm_rt_malloc(&b.d_sel_info, 16));
		CK(acm_rt_host_alloc((void **)&b.h_sel_info, 64));
		b.h_sel_info[1] = 0;
	}
	if (c.rewrite) {   // (disjoint matches of a byte or more: no more of them than text bytes)
		b.rw_max = std::min(b.all_cap - 2, size);
		b.rw_cap = std::min(2 * size + 65536 + 16, (size_t)0x7FFFFFE0ul);
		b.rw_ws_bytes = acm_rewrite_workspace_bytes(b.rw_max, G);
		CK(acm_rt_malloc(&b.d_rw_out, b.rw_cap + 16));
		CK(acm_rt_malloc(&b.d_rw_ws, b.rw_ws_bytes));
		CK(acm_rt_malloc(&b.d_rw_info, 32));
		CK(acm_rt_malloc(&b.d_rw_start, (G + 1) * 4));
		CK(acm_rt_malloc(&b.d_rw_seg, (G + 1) * 4));
		CK(acm_rt_host_alloc((void **)&b.h_rw_out, b.rw_cap + 16));
		CK(acm_rt_host_alloc((void **)&b.h_rw_info, 64));
		CK(acm_rt_host_alloc((void **)&b.h_rw_seg, (G + 1) * 4));
	}
	if (c.extract) {   // (a line a byte at most: size + 1 lines; a group costs its bytes, a glue and a terminator at most)
		b.ex_lcap = size + 1;
		b.ex_cap = std::min(size * 5 / 2 + 4 * G + 64, (size_t)0x7FFFFFE0ul);
		b.ex_ws_bytes = std::max(std::max(acm_line_index_workspace_bytes(size), acm_line_context_workspace_bytes(b.ex_lcap, G + 1)),
		    acm_extract_workspace_bytes(b.ex_lcap, G + 1));
		if (c.fmt) {   // (a prefix for every line, were the lines four bytes on average; collect_extract() refuses what does not fit)
			b.ex_cap = std::min(b.ex_cap + (size / 4 + 4096) * c.fmt_width, (size_t)0x7FFFFFE0ul);
			b.ex_ws_bytes = std::max(b.ex_ws_bytes, std::max(acm_line_context_lines_workspace_bytes(b.ex_lcap, G + 1),
			    acm_format_workspace_bytes(b.ex_lcap, G + 1)));
			CK(acm_rt_malloc(&b.d_ex_kind, (b.ex_lcap + 2) * 4));
			CK(acm_rt_malloc(&b.d_ex_names, (G + 1) * (c.fmt_width + 1) + 16));
			CK(acm_rt_malloc(&b.d_ex_name_off, (G + 3) * 4));
			CK(acm_rt_malloc(&b.d_ex_seg_num, (G + 1) * 4));
		}
		CK(acm_rt_malloc(&b.d_ex_lines, b.ex_lcap * 4));
		CK(acm_rt_malloc(&b.d_ex_line_info, 32));
		CK(acm_rt_malloc(&b.d_ex_ws, b.ex_ws_bytes));
		CK(acm_rt_malloc(&b.d_ex_text, size + 32));
		CK(acm_rt_malloc(&b.d_ex_rel, (b.ex_lcap + 2) * 4));
		CK(acm_rt_malloc(&b.d_ex_begin, (b.ex_lcap + 2) * 4));
		CK(acm_rt_malloc(&b.d_ex_next, (b.ex_lcap + 2) * 4));
		CK(acm_rt_malloc(&b.d_ex_ctx_info, 16));
		CK(acm_rt_malloc(&b.d_ex_out, b.ex_cap + 16));
		CK(acm_rt_malloc(&b.d_ex_info, 32));
		CK(acm_rt_malloc(&b.d_rw_start, (G + 1) * 4));
		CK(acm_rt_malloc(&b.d_ex_seg, (G + 1) * 4));
		CK(acm_rt_host_alloc((void **)&b.h_ex_out, b.ex_cap + 16));
		CK(acm_rt_host_alloc((void **)&b.h_ex_info, 64));
		CK(acm_rt_host_alloc((void **)&b.h_ex_seg, (G + 1) * 4));
	}
}

// binary mode: fixed chunks, a short tail chunk per file (databuf.c:326-407)
// returns bytes read (0 = nothing available right now)
size_t fill_binary(Buffer &b, const Config &c, int fd, int file_id, long *file_pos)
{
	const size_t G = (size_t)c.global_ws, B = (size_t)c.chunk;
	if (b.chunks >= G)
		return 0;
	b.file_off.resize(G + 1);
	const ssize_t got = read(fd, b.h_data + b.chunks * B, (G - b.chunks) * B);
	if (got <= 0)
		return 0;
	size_t left = (size_t)got;
	while (left) {
		const size_t take = std::min(left, B);
		b.h_indices[b.chunks] = (int32_t)(b.chunks * B);
		b.h_sizes[b.chunks] = (int32_t)take;
		b.file_ids[b.chunks] = file_id;
		b.file_off[b.chunks] = *file_pos;
		*file_pos += (long)take;
		b.chunks++;
		left -= take;
	}
	b.bytes = b.chunks * B;
	return (size_t)got;
}

// text mode: one chunk per line, 16-byte aligned, gaps zeroed (databuf.c:412-481)
size_t fill_text(Buffer &b, const Config &c, FILE *fp, int file_id, size_t *lines, long *file_pos)
{
	const size_t G = (size_t)c.global_ws, B = (size_t)c.chunk, size = G * B;
	size_t total = 0;
	b.file_off.resize(G + 1);
	while (b.chunks < G && b.bytes < size) {
		const size_t room = std::min(size - b.bytes, B);
		if (room < 2)
			break;
		char *dst = (char *)b.h_data + b.bytes;
		if (!fgets(dst, (int)room, fp))
			break;
		const size_t len = strnlen(dst, room);
		if (len && dst[len - 1] == '\n')
			(*lines)++;
		b.h_indices[b.chunks] = (int32_t)b.bytes;
		b.h_sizes[b.chunks] = (int32_t)len;
		b.file_ids[b.chunks] = file_id;
		b.file_off[b.chunks] = *file_pos;
		*file_pos += (long)len;
		b.chunks++;
		const size_t adv = std::min((len + 15) & ~(size_t)15, size - b.bytes);
		memset(dst + len, 0, adv - len);
		b.bytes += adv;
		total += len;
	}
	return total;
}

// the buffer's chunk list as one stream: chunk starts, its length, and (-S) where its texts begin.  Host
// only; called for every buffer in order, before submit
void prepare(Worker &w, Buffer &b)
{
	const Config &c = w.sh->cfg;
	const int chunks = (int)b.chunks;
	size_t stream_len = 0;
	b.packed = true;
	b.starts.resize((size_t)chunks + 1);
	for (int i = 0; i < chunks; i++) {
		if ((size_t)b.h_indices[i] != stream_len)
			b.packed = false;
		b.starts[i] = (int32_t)stream_len;
		stream_len += (size_t)b.h_sizes[i];
	}
	b.starts[chunks] = (int32_t)stream_len;
	b.stream_len = stream_len;
	if (c.count || c.lineno) {   // a start at every chunk of another file than the chunk before it, across buffers too
		b.cnt_starts.clear();
		b.cnt_files.clear();
		b.cnt_prev_file = w.cnt_file;
		for (int i = 0; i < chunks; i++) {
			if (b.file_ids[i] != w.cnt_file) {
				b.cnt_starts.push_back(b.starts[i]);
				b.cnt_files.push_back(b.file_ids[i]);
			}
			w.cnt_file = b.file_ids[i];
		}
	}
	if (c.extract && chunks > 0) {   // context is not continued across buffers: never silently wrong lines
		if (b.file_ids[0] == w.ex_file) {
			fprintf(stderr, "ERROR: -C: file '%s' is cut across two buffers and context is not continued across them; raise -G/-B\n",
			    w.sh->files[(size_t)w.ex_file].c_str());
			exit(1);
		}
		w.ex_file = b.file_ids[chunks - 1];
	}
	if (c.rewrite || c.extract) {   // the first chunk, and every chunk of another file than the chunk before it
		b.rw_starts.clear();
		b.rw_files.clear();
		for (int i = 0; i < chunks; i++)
			if (i == 0 || b.file_ids[i] != b.file_ids[i - 1]) {
				b.rw_starts.push_back(b.starts[i]);
				b.rw_files.push_back(b.file_ids[i]);
			}
	}
	if (c.segmented) {
		// a text begins at every chunk of another file than the chunk before it (-t: and at every chunk
		// that follows a finished line); a long line split over chunks, or a file over buffers, goes on
		b.seg_starts.clear();
		for (int i = 0; i < chunks; i++) {
			if (b.file_ids[i] != w.seg_file || (c.text_mode && !w.seg_open))
				b.seg_starts.push_back(b.starts[i]);
			w.seg_file = b.file_ids[i];
			w.seg_open = b.h_sizes[i] > 0 && b.h_data[b.h_indices[i] + b.h_sizes[i] - 1] != '\n';
		}
		// -P: how much of the text that goes on into this buffer the earlier buffers held, and whether the
		// last text is known to end here
		b.lead_begin = -(long)w.text_bytes;
		w.text_bytes = b.seg_starts.empty() ? w.text_bytes + stream_len : stream_len - (size_t)b.seg_starts.back();
		b.end_known = w.file_closed || (c.text_mode && chunks > 0 && !w.seg_open);
	}
}

// -W: the byte that follows the stream of the buffer in front of b, the first byte of b's stream; -1
// where b begins a new text (-S) or has no bytes
int first_byte(const Config &c, const Buffer &b)
{
	if (c.segmented && !b.seg_starts.empty() && b.seg_starts[0] == 0)
		return -1;
	for (size_t i = 0; i < b.chunks; i++)
		if (b.h_sizes[i] > 0)
			return b.h_data[b.h_indices[i]];
	return -1;
}

void finish(Worker &w, Buffer &b, int next_byte);

// enqueue copy-in and scan of one buffer (prepared), then, without -W, its bucket planes and copy-back;
// no sync.  prev: the worker's buffer in front of this one if its results have not been collected yet --
// the scan then starts in the state that buffer's scan ended in, read from its planes ON THE DEVICE
// (acm_scan_batch.d_init_plane; the reference carries it through the host, databuf.c:622): the GPU goes on
// with this buffer while the host walks the previous one's results.
void submit(Worker &w, Buffer &b, const Buffer *prev)
{
	const Config &c = w.sh->cfg;
	const int chunks = (int)b.chunks;
	void *s = w.stream;
	CK(acm_rt_memcpy_h2d(b.d_data, b.h_data, (b.bytes + 15) & ~(size_t)15, s));
	CK(acm_rt_memcpy_h2d(b.d_indices, b.h_indices, (size_t)chunks * 4, s));
	CK(acm_rt_memcpy_h2d(b.d_sizes, b.h_sizes, (size_t)chunks * 4, s));
	const size_t cap = (size_t)c.global_ws * c.chunk + 2;
	b.text = b.d_data;
	if (!b.packed) {   // padded chunk list: scan the chunks' bytes back to back
		CK(acm_rt_memcpy_h2d(b.d_starts, b.starts.data(), ((size_t)chunks + 1) * 4, s));
		CK(acm_pack_chunks(b.d_packed, b.d_data, (const int32_t *)b.d_indices, (const int32_t *)b.d_sizes,
		    (const int32_t *)b.d_starts, chunks, s));
		b.text = b.d_packed;
	}
	if (c.segmented && !b.seg_starts.empty())
		CK(acm_rt_memcpy_h2d(b.d_seg_start, b.seg_starts.data(), b.seg_starts.size() * 4, s));
	b.scan_text = b.text;
	b.scan_len = b.stream_len;
	b.scan_seg = (const int32_t *)b.d_seg_start;
	if (c.norm) {
		// the stream normalised, every text (-S: a file, with -t a line) alone; what follows scans and filters the
		// normalised stream, and finish() maps the records back.  The scan's length is a host argument: the host waits
		// here for the figures.  A file that a buffer cuts is normalised piece by piece.
		static const uint8_t nul_set[32] = { 1 };
		const size_t ns = b.seg_starts.size();
		CK(acm_normalize_async(b.text, b.stream_len, 0, c.norm_flags, c.norm_nul ? nul_set : nullptr, ' ', b.d_nz_out,
		    (size_t)c.global_ws * c.chunk + 16, (uint64_t *)b.d_nz_keep, (int32_t *)b.d_nz_block,
		    ns ? (const int32_t *)b.d_seg_start : nullptr, ns, ns ? (int32_t *)b.d_nz_seg : nullptr, (int32_t *)b.d_nz_info,
		    b.d_nz_ws, b.nz_ws_bytes, s));
		CK(acm_rt_memcpy_d2h(b.h_nz_info, b.d_nz_info, 32, s));
		CK(acm_rt_stream_sync(s));
		b.scan_text = b.d_nz_out;
		b.scan_len = (size_t)b.h_nz_info[0];
		b.scan_seg = (const int32_t *)b.d_nz_seg;
	}
	int32_t *pat = (int32_t *)b.d_pat, *off = (int32_t *)b.d_off;
	acm_scan_batch sb;
	memset(&sb, 0, sizeof(sb));
	sb.d_text = b.scan_text;
	sb.n = b.scan_len;
	sb.init_state = w.last_state;
	if (prev) {
		sb.init_state = 0;
		sb.d_init_plane = prev->end_plane;
		sb.init_plane_capacity = prev->scan_cap;
	}
	sb.d_workspace = w.ws;
	sb.workspace_bytes = w.ws_bytes;
	sb.d_pat_plane = pat;
	sb.d_off_plane = off;
	sb.plane_capacity = cap;
	sb.stream = s;
	b.scan_cap = cap;
	b.end_plane = pat;
	// final states instead of head patterns where a pass over the records follows: the segment pass
	// clamps every one to its own text, the word pass keeps whole words, the case pass (-I) the exact
	// patterns where the text has their case, the expansion (-A) lists them
	const bool states = c.segmented || c.words || c.all_patterns || c.cased || c.seq;   // (-P needs -S)
	sb.report = states ? ACM_REPORT_STATE : ACM_REPORT_HEAD;
	if ((c.pos || c.wild || c.approx) && c.segmented && b.end_known) {   // a start at the stream's end, for the position, wildcard and approx passes alone: the last text is closed
		b.end_start = (int32_t)b.stream_len;
		CK(acm_rt_memcpy_h2d((int32_t *)b.d_seg_start + b.seg_starts.size(), &b.end_start, 4, s));
	}
	CK(acm_scan_batch_async(w.dfa, &sb));
	if (c.segmented) {
		CK(acm_segment_matches_async(w.dfa, pat, off, cap - 2, b.scan_seg, b.seg_starts.size(),
		    (long)b.scan_len,(c.all_patterns || c.words || c.cased || c.pos || c.seq) ? ACM_REPORT_STATE : ACM_REPORT_HEAD,
		    (int32_t *)b.d_seg_pat, (int32_t *)b.d_seg_off, nullptr, cap, nullptr, b.d_seg_ws, b.seg_ws_bytes, s));
		pat = (int32_t *)b.d_seg_pat;
		off = (int32_t *)b.d_seg_off;
		b.end_plane = pat;   // its trailer is the clamped state: the next buffer goes on from there
	}
	b.rec_pat = pat;
	b.rec_off = off;
	if (!c.words)
		finish(w, b, -1);
}

// enqueue the passes over b's records, its bucket planes and copy-back.  -W: called once the byte after
// b's stream is known (next_byte: the first byte of the next buffer, or -1 at the end of the stream), on
// the worker's stream in front of the next buffer's copy-in
void finish(Worker &w, Buffer &b, int next_byte)
{
	const Config &c = w.sh->cfg;
	const int chunks = (int)b.chunks;
	void *s = w.stream;
	int32_t *pat = b.rec_pat, *off = b.rec_off;
	size_t cap = b.scan_cap;
	if (c.words) {   // whole words; with -A every word-bounded pattern (the expansion's place)
		const bool every = c.all_patterns || c.pos;   // (-P: the position pass picks the first kept one)
		int32_t *wp = (int32_t *)(every ? b.d_pat_all : b.d_word_pat);
		int32_t *wo = (int32_t *)(every ? b.d_off_all : b.d_word_off);
		const size_t wcap = every ? b.all_cap : b.scan_cap;
		CK(acm_word_matches_async(w.dfa, pat, off, cap - 2, b.scan_text, 0, (long)b.scan_len,
		    w.tail_len ? w.d_tail[w.tail_cur] : nullptr, w.tail_len, next_byte,
		    c.segmented ? b.scan_seg : nullptr, c.segmented ? b.seg_starts.size() : 0, nullptr,
		    every, wp, wo, wcap, w.d_tail[w.tail_cur ^ 1], b.d_word_ws, b.word_ws_bytes, s));
		w.tail_cur ^= 1;
		w.tail_len = std::min((size_t)w.sh->max_pattern_len, w.tail_len + b.scan_len);
		pat = wp;
		off = wo;
		cap = wcap;
		if (every)
			CK(acm_rt_memcpy_d2h(b.h_all_count, pat, 4, s));
	} else if (c.cased) {   // the candidates of a mixed automaton made exact; with -A every kept pattern (the expansion's place)
		const bool every = c.all_patterns || c.pos || c.seq;   // (-P: the position pass picks the first kept one)
		int32_t *cp = (int32_t *)(every ? b.d_pat_all : b.d_case_pat);
		int32_t *co = (int32_t *)(every ? b.d_off_all : b.d_case_off);
		const size_t ccap = every ? b.all_cap : b.scan_cap;
		// the tail of the worker's stream so far is this buffer's before: a pattern that began in the buffer
		// in front is compared whole (-S: the segment pass has left no entry that reaches into another text)
		CK(acm_case_matches_async(w.dfa, pat, off, cap - 2, b.scan_text, 0, (long)b.scan_len,
		    w.tail_len ? w.d_tail[w.tail_cur] : nullptr, w.tail_len, every, cp, co, ccap, w.d_tail[w.tail_cur ^ 1],
		    b.d_case_ws, b.case_ws_bytes, s));
		w.tail_cur ^= 1;
		w.tail_len = std::min((size_t)w.sh->max_pattern_len, w.tail_len + b.scan_len);
		pat = cp;
		off = co;
		cap = ccap;
		if (every)
			CK(acm_rt_memcpy_d2h(b.h_all_count, pat, 4, s));
	} else if ((c.all_patterns || c.seq) && !c.pos) {   // every pattern of each final state's match list
		CK(acm_expand_matches_async(w.dfa, pat, off, cap - 2, (int32_t *)b.d_pat_all, (int32_t *)b.d_off_all,
		    b.all_cap, b.d_expand_ws, b.expand_ws_bytes, s));
		pat = (int32_t *)b.d_pat_all;
		off = (int32_t *)b.d_off_all;
		cap = b.all_cap;
		CK(acm_rt_memcpy_d2h(b.h_all_count, pat, 4, s));
	}
	if (c.norm)   // every pass that reads the normalised stream has run: each record back to the last byte of the unit
		      // that emitted its last byte, in the stream's own coordinates: what is counted, bucketed and printed
		CK(acm_normalize_remap_async(nullptr, b.text, b.stream_len, 0, c.norm_flags, (const uint64_t *)b.d_nz_keep,
		    (const int32_t *)b.d_nz_block, nullptr, off, cap - 2, off, nullptr, (int32_t *)b.d_nz_rinfo, s));
	if (c.approx) {
		// the mismatches of every piece's whole pattern, each in its own text.  The planes hold every pattern (the
		// expansion's, or the case pass's); the tail of the worker's stream so far is this buffer's before: a span
		// that began in the buffer in front is compared whole, one that reaches behind this buffer's end is
		// undecided and counted.
		const size_t nseg = c.segmented ? b.seg_starts.size() + (b.end_known ? 1 : 0) : 0;
		// -e: the edit pass takes the same planes, bytes and texts, and leaves whole matches: unique, in offset order
		if (c.edit)
			CK(acm_edit_matches_async(w.dfa, pat, off, cap - 2, ACM_REPORT_HEAD, b.text, 0, (long)b.stream_len,
			    w.atail_len ? w.d_atail[w.atail_cur] : nullptr, w.atail_len, nseg ? (const int32_t *)b.d_seg_start : nullptr, nseg,
			    c.segmented ? b.lead_begin : -(1L << 40), b.last_of_input ? (long)b.stream_len : -1L, (int32_t *)b.d_apx_pat,
			    (int32_t *)b.d_apx_off, (int32_t *)b.d_apx_dist, (int32_t *)b.d_apx_len, b.all_cap, (int32_t *)b.d_apx_info,
			    b.d_apx_ws, b.apx_ws_bytes, s));
		else
			CK(acm_approx_matches_async(w.dfa, pat, off, cap - 2, ACM_REPORT_HEAD, b.text, 0, (long)b.stream_len,
			    w.atail_len ? w.d_atail[w.atail_cur] : nullptr, w.atail_len, nseg ? (const int32_t *)b.d_seg_start : nullptr, nseg,
			    c.segmented ? b.lead_begin : -(1L << 40), b.last_of_input ? (long)b.stream_len : -1L, (int32_t *)b.d_apx_pat,
			    (int32_t *)b.d_apx_off, (int32_t *)b.d_apx_dist, b.all_cap, (int32_t *)b.d_apx_info, b.d_apx_ws, b.apx_ws_bytes, s));
		// the next buffer's before: the last apx_back bytes of the old tail and this stream
		const size_t keep = std::min((size_t)w.sh->apx_back, w.atail_len + b.stream_len);
		const size_t from_text = std::min(keep, b.stream_len), from_old = keep - from_text;
		char *next_tail = (char *)w.d_atail[w.atail_cur ^ 1];
		if (from_old)
			CK(acm_rt_memcpy_d2d(next_tail, (const char *)w.d_atail[w.atail_cur] + (w.atail_len - from_old), from_old, s));
		if (from_text)
			CK(acm_rt_memcpy_d2d(next_tail + from_old, (const char *)b.text + (b.stream_len - from_text), from_text, s));
		w.atail_cur ^= 1;
		w.atail_len = keep;
		pat = (int32_t *)b.d_apx_pat;
		off = (int32_t *)b.d_apx_off;
		cap = b.all_cap;
		CK(acm_rt_memcpy_d2h(b.h_apx_info, b.d_apx_info, 16, s));
	}
	bool wild_ran = false;
	if (c.wild) {
		// the positions around every anchor, each in its own text (as the position pass below finds it).  Behind
		// the case pass or the expansion the planes hold patterns, else the segment pass's states.  No bytes of
		// the buffer in front are given: a candidate that reaches there is undecided and counted.
		const bool heads = c.cased || !c.pos;
		const size_t nseg = c.segmented ? b.seg_starts.size() + (b.end_known ? 1 : 0) : 0;
		CK(acm_wildcard_matches_async(w.dfa, pat, off, cap - 2, heads ? ACM_REPORT_HEAD : ACM_REPORT_STATE, b.text, 0,
		    (long)b.stream_len, nullptr, 0, nseg ? (const int32_t *)b.d_seg_start : nullptr, nseg,
		    c.segmented ? b.lead_begin : -(1L << 40), b.last_of_input ? (long)b.stream_len : -1L, 1, (int32_t *)b.d_wild_pat,
		    (int32_t *)b.d_wild_off, b.all_cap, (int32_t *)b.d_wild_info, b.d_wild_ws, b.wild_ws_bytes, s));
		pat = (int32_t *)b.d_wild_pat;
		off = (int32_t *)b.d_wild_off;
		cap = b.all_cap;
		CK(acm_rt_memcpy_d2h(b.h_wild_info, b.d_wild_info, 16, s));
		if (!heads)   // (no pass in front has counted every pattern)
			CK(acm_rt_memcpy_d2h(b.h_all_count, pat, 4, s));
		wild_ran = true;
	}
	if (c.pos) {
		// the windows of the patterns, each in its own text: the files' (-t: lines') starts of this stream, the
		// text that goes on from the buffer in front, and the end of the last one where it is known.  Behind
		// the word or case pass the planes hold patterns (every kept one), else the segment pass's states.
		const bool heads = c.words || c.cased || wild_ran;
		CK(acm_position_matches_async(w.dfa, pat, off, cap - 2, heads ? ACM_REPORT_HEAD : ACM_REPORT_STATE,
		    (const int32_t *)b.d_seg_start, b.seg_starts.size() + (b.end_known ? 1 : 0), b.lead_begin, (long)b.stream_len,
		    b.last_of_input ? (long)b.stream_len : -1L, c.all_patterns || c.seq, (int32_t *)b.d_pos_pat, (int32_t *)b.d_pos_off,
		    b.pos_cap, (int32_t *)b.d_pos_info, b.d_pos_ws, b.pos_ws_bytes, s));
		pat = (int32_t *)b.d_pos_pat;
		off = (int32_t *)b.d_pos_off;
		cap = b.pos_cap;
		CK(acm_rt_memcpy_d2h(b.h_pos_info, b.d_pos_info, 16, s));
		if ((c.all_patterns || c.seq) && !heads)
			CK(acm_rt_memcpy_d2h(b.h_all_count, pat, 4, s));
	}
	if (c.seq) {
		// the signatures: the parts' records (every pattern, whatever pass wrote them) joined on the device.
		// Without -S the stream is one text that began long ago: only a chain inside this buffer is found.
		CK(acm_sequence_matches_async(w.dfa, pat, off, b.seq_max, c.segmented ? (const int32_t *)b.d_seg_start : nullptr,
		    c.segmented ? b.seg_starts.size() : 0, c.segmented ? b.lead_begin : -(1L << 40), (long)b.stream_len,
		    (int32_t *)b.d_seq_pat, (int32_t *)b.d_seq_off, b.seq_max + 2, (int32_t *)b.d_seq_info, b.d_seq_ws, b.seq_ws_bytes, s));
		pat = (int32_t *)b.d_seq_pat;
		off = (int32_t *)b.d_seq_off;
		cap = b.seq_max + 2;
	}
	if (c.only) {
		// the leftmost-longest non-overlapping matches of every pattern's records, whatever pass wrote them.  The
		// buffer begins at stream offset 0: an entry that starts in front of it is dropped and counted.
		CK(acm_select_matches_async(w.dfa, pat, off, cap - 2, 0, 0, (int32_t *)b.d_sel_pat, (int32_t *)b.d_sel_off, nullptr,
		    b.all_cap, (int32_t *)b.d_sel_info, b.d_sel_ws, b.sel_ws_bytes, s));
		pat = (int32_t *)b.d_sel_pat;
		off = (int32_t *)b.d_sel_off;
		cap = b.all_cap;
		CK(acm_rt_memcpy_d2h(b.h_sel_info, b.d_sel_info, 16, s));
	}
	if (c.rewrite) {
		// the buffer's stream with every selected match replaced, and where every file's bytes begin in it.  Only the
		// figures come back here; collect() fetches the output once it knows its length.  (In front of the remap below:
		// the offsets are still the stream's.)
		const size_t ns = b.rw_starts.size();
		CK(acm_rt_memcpy_h2d(b.d_rw_start, b.rw_starts.data(), ns * 4, s));
		CK(acm_rewrite_async(w.dfa, b.text, b.stream_len, 0, pat, off, b.rw_max, b.d_rw_out, b.rw_cap, nullptr, 0,
		    (const int32_t *)b.d_rw_start, ns, (int32_t *)b.d_rw_seg, (int32_t *)b.d_rw_info, b.d_rw_ws, b.rw_ws_bytes, s));
		CK(acm_rt_memcpy_d2h(b.h_rw_info, b.d_rw_info, 32, s));
		CK(acm_rt_memcpy_d2h(b.h_rw_seg, b.d_rw_seg, ns * 4, s));
	}
	if (c.extract) {
		// the lines of this buffer's stream, the ones that hold a record as it is reported (or none: -V) with their
		// context, grouped inside every file, and the groups' bytes packed.  Only the figures come back here; collect()
		// fetches the output once it knows its length.  (In front of the remap below: the offsets are still the stream's.)
		const size_t ns = b.rw_starts.size();
		const void *lines_of = b.text;
		bool open_end = false;   // some file in front of another does not end in a newline
		for (size_t k = 1; k < ns && !open_end; k++) {
			const size_t i = (size_t)(std::lower_bound(b.starts.begin(), b.starts.begin() + chunks, b.rw_starts[k]) - b.starts.begin());
			open_end = i > 0 && b.h_sizes[i - 1] > 0 && b.h_data[b.h_indices[i - 1] + b.h_sizes[i - 1] - 1] != '\n';
		}
		if (open_end) {   // the index runs over a copy with a newline on such a file's last byte; the extract reads the text
			CK(acm_rt_memcpy_d2d(b.d_ex_text, b.text, (b.stream_len + 15) & ~(size_t)15, s));
			for (size_t k = 1; k < ns; k++)
				if (b.rw_starts[k] > 0)
					CK(acm_rt_memset((char *)b.d_ex_text + b.rw_starts[k] - 1, '\n', 1, s));
			lines_of = b.d_ex_text;
		}
		CK(acm_rt_memcpy_h2d(b.d_rw_start, b.rw_starts.data(), ns * 4, s));
		CK(acm_line_index_async(lines_of, b.stream_len, 0, '\n', -1, nullptr, (int32_t *)b.d_ex_lines, b.ex_lcap,
		    (int32_t *)b.d_ex_line_info, b.d_ex_ws, b.ex_ws_bytes, s));
		const bool sep = c.ctx_before + c.ctx_after > 0;
		if (c.fmt) {
			// one entry per kept line, and in front of each its file's name, its line and its offset in that file: the
			// lines in front of every file start come from the same index (every file start is a line start there)
			b.ex_names.clear();
			b.ex_name_off.assign(1, 0);
			for (size_t k = 0; k <= ns; k++) {   // text id k: file k - 1 of this buffer
				if (k > 0 && c.fmt_name) {
					const std::string &name = w.sh->files[(size_t)b.rw_files[k - 1]];
					b.ex_names.insert(b.ex_names.end(), name.begin(), name.end());
				}
				b.ex_name_off.push_back((int32_t)b.ex_names.size());
			}
			if (!b.ex_names.empty())
				CK(acm_rt_memcpy_h2d(b.d_ex_names, b.ex_names.data(), b.ex_names.size(), s));
			CK(acm_rt_memcpy_h2d(b.d_ex_name_off, b.ex_name_off.data(), b.ex_name_off.size() * 4, s));
			if (ns > 0)
				CK(acm_line_number_async((const int32_t *)b.d_ex_lines, b.ex_lcap, (const int32_t *)b.d_ex_line_info,
				    (const int32_t *)b.d_rw_start, nullptr, ns, (int32_t *)b.d_ex_seg_num, s));
			CK(acm_line_context_lines_async((const int32_t *)b.d_ex_lines, b.ex_lcap, (const int32_t *)b.d_ex_line_info, 0,
			    (long)b.stream_len, off, cap - 2, c.invert, c.ctx_before, c.ctx_after, (const int32_t *)b.d_rw_start, ns,
			    (int32_t *)b.d_ex_rel, (int32_t *)b.d_ex_begin, (int32_t *)b.d_ex_next, (int32_t *)b.d_ex_kind, b.ex_lcap + 2,
			    (int32_t *)b.d_ex_ctx_info, b.d_ex_ws, b.ex_ws_bytes, s));
			const unsigned flags = (c.fmt_name ? ACM_FORMAT_NAME : 0) | (c.fmt_num ? ACM_FORMAT_NUMBER : 0) | (c.fmt_off ? ACM_FORMAT_OFFSET : 0);
			CK(acm_format_async(b.text, b.stream_len, 0, (const int32_t *)b.d_ex_begin, (const int32_t *)b.d_ex_next, b.ex_lcap, flags,
			    (const int32_t *)b.d_ex_kind, (const int32_t *)b.d_ex_rel, (const int32_t *)b.d_ex_seg_num, 1, 0, ':', '-',
			    (const uint8_t *)b.d_ex_names, (const int32_t *)b.d_ex_name_off, b.ex_names.size(), (const uint8_t *)"--\n", sep ? 3 : 0,
			    '\n', b.d_ex_out, b.ex_cap, nullptr, 0, (const int32_t *)b.d_rw_start, ns, (int32_t *)b.d_ex_seg,
			    (int32_t *)b.d_ex_info, b.d_ex_ws, b.ex_ws_bytes, s));
		} else {
			CK(acm_line_context_async((const int32_t *)b.d_ex_lines, b.ex_lcap, (const int32_t *)b.d_ex_line_info, 0, (long)b.stream_len,
			    off, cap - 2, c.invert, c.ctx_before, c.ctx_after, (const int32_t *)b.d_rw_start, ns, (int32_t *)b.d_ex_rel,
			    (int32_t *)b.d_ex_begin, (int32_t *)b.d_ex_next, nullptr, b.ex_lcap + 2, (int32_t *)b.d_ex_ctx_info, b.d_ex_ws,
			    b.ex_ws_bytes, s));
			CK(acm_extract_async(b.text, b.stream_len, 0, (const int32_t *)b.d_ex_begin, (const int32_t *)b.d_ex_next, b.ex_lcap, 0,
			    (const uint8_t *)"--\n", sep ? 3 : 0, '\n', b.d_ex_out, b.ex_cap, nullptr, 0, (const int32_t *)b.d_rw_start, ns,
			    (int32_t *)b.d_ex_seg, (int32_t *)b.d_ex_info, b.d_ex_ws, b.ex_ws_bytes, s));
		}
		CK(acm_rt_memcpy_d2h(b.h_ex_info, b.d_ex_info, 32, s));
		CK(acm_rt_memcpy_d2h(b.h_ex_seg, b.d_ex_seg, ns * 4, s));
	}
	if (c.rules) {
		// the rules: the signatures' records counted per text and the conditions evaluated on the device.  Only the
		// count comes back here; collect() fetches that many records.  (The bucket planes below keep carrying the
		// signatures' records: the scan state of the next buffer comes from their trailer.)
		CK(acm_rule_matches_async(w.dfa, pat, off, b.seq_max, (const int32_t *)b.d_seg_start, b.seg_starts.size(),
		    (int32_t *)b.d_rule_out, (int32_t *)b.d_rule_text, (int32_t *)b.d_rule_off, b.seq_max + 2, (int32_t *)b.d_rule_info,
		    b.d_rule_ws, b.rule_ws_bytes, s));
		CK(acm_rt_memcpy_d2h(b.h_rule_count, b.d_rule_out, 4, s));
	}
	if (c.lineno) {
		// the lines of this buffer's stream, chained to the buffer in front of it on the device; then the
		// newlines in front of every record and of every file start, in stream coordinates (before the remap)
		const size_t nstart = b.cnt_starts.size(), lcap = (size_t)c.global_ws * c.chunk + 1;
		CK(acm_line_index_async(b.text, b.stream_len, 0, '\n', -1, w.line_prev_info, (int32_t *)b.d_line_start, lcap,
		    (int32_t *)b.d_line_info, b.d_line_ws, b.line_ws_bytes, s));
		w.line_prev_info = (const int32_t *)b.d_line_info;
		CK(acm_rt_memcpy_d2d(b.d_line_plane, off, 4, s));   // the header cell; the trailer cell is not used
		CK(acm_line_number_async((const int32_t *)b.d_line_start, lcap, (const int32_t *)b.d_line_info, off + 1, off, cap - 2,
		    (int32_t *)b.d_line_plane + 1, s));
		if (nstart) {
			CK(acm_rt_memcpy_h2d(b.d_cnt_start, b.cnt_starts.data(), nstart * 4, s));
			CK(acm_line_number_async((const int32_t *)b.d_line_start, lcap, (const int32_t *)b.d_line_info,
			    (const int32_t *)b.d_cnt_start, nullptr, nstart, (int32_t *)b.d_start_line, s));
			CK(acm_rt_memcpy_d2h(b.h_start_line, b.d_start_line, nstart * 4, s));
		}
		CK(acm_rt_memcpy_d2h(b.h_line_info, b.d_line_info, 32, s));
	}
	if (c.count && !w.sh->pat_iid.empty()) {
		// exact counts of the records as they are reported (pattern indices by now, whatever passes ran),
		// in stream coordinates: per pattern into the worker's running totals, per file over the grid of
		// file starts; the records in front of the first start belong to the file the worker was in
		const size_t np = w.sh->pat_iid.size(), nstart = b.cnt_starts.size();
		CK(acm_tally_matches_async(w.dfa, pat, off, cap - 2, ACM_REPORT_HEAD, ACM_TALLY_ACCUMULATE, nullptr, np, nullptr, 0,
		    (uint64_t *)w.d_pat_total, nullptr, nullptr, b.d_cnt_ws, b.cnt_ws_bytes, s));
		if (nstart)
			CK(acm_rt_memcpy_h2d(b.d_cnt_start, b.cnt_starts.data(), nstart * 4, s));
		CK(acm_tally_matches_async(w.dfa, pat, off, cap - 2, ACM_REPORT_HEAD, 0, (const int32_t *)w.d_one_class, 1,
		    (const int32_t *)b.d_cnt_start, nstart, (uint64_t *)b.d_cnt_total, nstart ? (int32_t *)b.d_cnt_rows : nullptr,
		    (int32_t *)b.d_cnt_lead, b.d_cnt_ws, b.cnt_ws_bytes, s));
		if (nstart)
			CK(acm_rt_memcpy_d2h(b.h_cnt_rows, b.d_cnt_rows, nstart * 4, s));
		CK(acm_rt_memcpy_d2h(b.h_cnt_lead, b.d_cnt_lead, 4, s));
		CK(acm_rt_memcpy_d2h(b.h_cnt_total, b.d_cnt_total, 8, s));
	}
	if (!b.packed)
		CK(acm_remap_offsets(off, cap - 2, (const int32_t *)b.d_indices,
		    (const int32_t *)b.d_starts, chunks, s));
	CK(acm_bucketize(pat, off, (const int32_t *)b.d_indices,
	    (const int32_t *)b.d_sizes, chunks, c.max_results, (int32_t *)b.d_results, (int32_t *)b.d_results2, cap, s));
	const size_t cells = (size_t)c.max_results * chunks + 1;
	if (c.lineno) {   // the line plane through the same buckets: cell for cell where the pattern plane's cells went
		CK(acm_bucketize((const int32_t *)b.d_line_plane, off, (const int32_t *)b.d_indices, (const int32_t *)b.d_sizes, chunks,
		    c.max_results, (int32_t *)b.d_results3, (int32_t *)b.d_results3_off, cap, s));
		CK(acm_rt_memcpy_d2h(b.h_results3, b.d_results3, cells * 4, s));
	}
	if (c.approx) {   // the distance plane through the same buckets: cell for cell where the pattern plane's cells went
		CK(acm_bucketize((const int32_t *)b.d_apx_dist, off, (const int32_t *)b.d_indices, (const int32_t *)b.d_sizes, chunks,
		    c.max_results, (int32_t *)b.d_results3, (int32_t *)b.d_results3_off, cap, s));
		CK(acm_rt_memcpy_d2h(b.h_results3, b.d_results3, cells * 4, s));
		if (c.edit) {   // and the length plane
			CK(acm_bucketize((const int32_t *)b.d_apx_len, off, (const int32_t *)b.d_indices, (const int32_t *)b.d_sizes, chunks,
			    c.max_results, (int32_t *)b.d_results4, (int32_t *)b.d_results3_off, cap, s));
			CK(acm_rt_memcpy_d2h(b.h_results4, b.d_results4, cells * 4, s));
		}
	}
	CK(acm_rt_memcpy_d2h(b.h_results, b.d_results, cells * 4, s));
	CK(acm_rt_memcpy_d2h(b.h_results2, b.d_results2, cells * 4, s));
	if (!b.done)
		CK(acm_rt_event_create(&b.done));
	CK(acm_rt_event_record(b.done, s));
}

// -K: the rule pass's planes copied back directly -- the count came with the buffer, the records now -- and the
// records of the texts this buffer holds whole reported.  The text in front of the first start began in an
// earlier buffer, and the last text goes on unless its end is known: their records are dropped.
void collect_rules(Worker &w, Buffer &b)
{
	const Config &c = w.sh->cfg;
	const size_t n = std::min((size_t)std::max(*b.h_rule_count, 0), b.seq_max), S = b.seg_starts.size();
	if (!b.end_known && S > 0)   // (S == 0: the whole buffer lies inside a text that was counted when it was cut first)
		w.cut_texts++;
	if (n == 0)
		return;
	b.h_rule.resize(n);
	b.h_rule_text.resize(n);
	CK(acm_rt_memcpy_d2h(b.h_rule.data(), (const int32_t *)b.d_rule_out + 1, n * 4, w.stream));
	CK(acm_rt_memcpy_d2h(b.h_rule_text.data(), (const int32_t *)b.d_rule_text + 1, n * 4, w.stream));
	CK(acm_rt_stream_sync(w.stream));
	for (size_t j = 0; j < n; j++) {
		const int32_t r = b.h_rule[j], k = b.h_rule_text[j];
		if (k < 0 || (size_t)k >= S || r < 0 || (size_t)r >= w.sh->rule_iid.size())   // the lead text: cut
			continue;
		if ((size_t)k + 1 == S && !b.end_known)   // the last text goes on in the next buffer: cut
			continue;
		w.matches++;
		w.reported++;
		if (!c.verbose)
			continue;
		// a text begins with a chunk: the chunk whose stream offset is the text's start
		const size_t i = (size_t)(std::lower_bound(b.starts.begin(), b.starts.begin() + (long)b.chunks, b.seg_starts[(size_t)k]) -
		                          b.starts.begin());
		if (i >= b.chunks)
			continue;
		pthread_mutex_lock(&w.sh->print_lock);
		printf("Rule %d matched in file '%s' [text at offset %ld]\n", w.sh->rule_iid[(size_t)r], w.sh->files[b.file_ids[i]].c_str(),
		    b.file_off[i]);
		pthread_mutex_unlock(&w.sh->print_lock);
	}
}

// mkdir -p of the directories a path lies in
void make_parents(const std::string &path)
{
	for (size_t at = path.find('/', 1); at != std::string::npos; at = path.find('/', at + 1))
		mkdir(path.substr(0, at).c_str(), 0777);   // (an error shows when the file is opened)
}

// -r: the rewritten stream of the buffer copied back -- its length came with the buffer -- and every file's piece of
// it appended to that file's output
void collect_rewrite(Worker &w, Buffer &b)
{
	Shared &sh = *w.sh;
	const size_t ns = b.rw_starts.size();
	const int64_t m = (int64_t)(((uint64_t)(uint32_t)b.h_rw_info[3] << 32) | (uint32_t)b.h_rw_info[2]);
	if (b.h_rw_info[6] || m < 0 || (size_t)m > b.rw_cap) {
		fprintf(stderr, "ERROR: -r: the rewrite of a buffer of '%s' has %ld bytes, the output buffer holds %zu; use a smaller -G/-B\n",
		    ns ? sh.files[(size_t)b.rw_files[0]].c_str() : "?", (long)m, b.rw_cap);
		exit(1);
	}
	if (m > 0) {
		CK(acm_rt_memcpy_d2h(b.h_rw_out, b.d_rw_out, (size_t)m, w.stream));
		CK(acm_rt_stream_sync(w.stream));
	}
	for (size_t k = 0; k < ns; k++) {
		const size_t f = (size_t)b.rw_files[k];
		const int64_t lo = std::min<int64_t>(std::max(b.h_rw_seg[k], 0), m);
		const int64_t hi = k + 1 < ns ? std::min<int64_t>(std::max<int64_t>(b.h_rw_seg[k + 1], lo), m) : m;
		if (!sh.out_begun[f])
			make_parents(sh.out_paths[f]);
		FILE *fp = fopen(sh.out_paths[f].c_str(), sh.out_begun[f] ? "ab" : "wb");
		if (!fp || fwrite(b.h_rw_out + lo, 1, (size_t)(hi - lo), fp) != (size_t)(hi - lo) || fclose(fp) != 0) {
			fprintf(stderr, "ERROR: -O: cannot write '%s': %s\n", sh.out_paths[f].c_str(), strerror(errno));
			exit(1);
		}
		sh.out_begun[f] = 1;
	}
}

// -C: the packed lines of the buffer copied back -- their length came with the buffer -- and every file's piece of
// them appended to that file's output
void collect_extract(Worker &w, Buffer &b)
{
	Shared &sh = *w.sh;
	const size_t ns = b.rw_starts.size();
	const int64_t m = (int64_t)(((uint64_t)(uint32_t)b.h_ex_info[3] << 32) | (uint32_t)b.h_ex_info[2]);
	if (b.h_ex_info[6] || m < 0 || (size_t)m > b.ex_cap) {
		fprintf(stderr, "ERROR: -C: the lines of a buffer of '%s' have %ld bytes, the output buffer holds %zu; use a smaller -G/-B\n",
		    ns ? sh.files[(size_t)b.rw_files[0]].c_str() : "?", (long)m, b.ex_cap);
		exit(1);
	}
	if (m > 0) {
		CK(acm_rt_memcpy_d2h(b.h_ex_out, b.d_ex_out, (size_t)m, w.stream));
		CK(acm_rt_stream_sync(w.stream));
	}
	for (size_t k = 0; k < ns; k++) {
		const size_t f = (size_t)b.rw_files[k];
		const int64_t lo = std::min<int64_t>(std::max(b.h_ex_seg[k], 0), m);
		const int64_t hi = k + 1 < ns ? std::min<int64_t>(std::max<int64_t>(b.h_ex_seg[k + 1], lo), m) : m;
		if (!sh.out_begun[f])
			make_parents(sh.out_paths[f]);
		FILE *fp = fopen(sh.out_paths[f].c_str(), sh.out_begun[f] ? "ab" : "wb");
		if (!fp || fwrite(b.h_ex_out + lo, 1, (size_t)(hi - lo), fp) != (size_t)(hi - lo) || fclose(fp) != 0) {
			fprintf(stderr, "ERROR: -T: cannot write '%s': %s\n", sh.out_paths[f].c_str(), strerror(errno));
			exit(1);
		}
		sh.out_begun[f] = 1;
	}
}

// wait for the buffer, walk the bucket planes (databuf.c:747-782), print -v lines
void collect(Worker &w, Buffer &b)
{
	const Config &c = w.sh->cfg;
	CK(acm_rt_event_sync(b.done));   // (this buffer's copies; the next buffer's scan may still be running)
	if (b.h_all_count && (size_t)*b.h_all_count > b.all_cap - 2) {
		fprintf(stderr, "ERROR: %s produced %d records for one buffer, the planes hold %zu; use a smaller -G/-B\n",
		    c.seq ? "-Q" : c.only ? "-o" : c.all_patterns ? "-A" : "-P", *b.h_all_count, b.all_cap - 2);
		exit(1);
	}
	if (c.seq && (size_t)*b.h_all_count > b.seq_max) {
		fprintf(stderr, "ERROR: -Q: %d pattern records in one buffer, the sequence pass takes %zu; use a smaller -G/-B\n",
		    *b.h_all_count, b.seq_max);
		exit(1);
	}
	if (c.pos)
		w.undecided += (uint64_t)b.h_pos_info[0];
	if (c.wild)
		w.wild_undecided += (uint64_t)b.h_wild_info[0];
	if (c.approx)
		w.apx_undecided += (uint64_t)b.h_apx_info[0];
	if (c.only)
		w.sel_dropped += (uint64_t)b.h_sel_info[1];
	if (c.rewrite)
		collect_rewrite(w, b);
	if (c.extract)
		collect_extract(w, b);
	if (c.count && !w.sh->pat_iid.empty()) {
		if (b.cnt_starts.empty()) {   // the whole buffer goes on with the file in front of it
			if (b.cnt_prev_file >= 0)
				w.file_total[(size_t)b.cnt_prev_file] += *b.h_cnt_total;
		} else {
			if (b.cnt_prev_file >= 0)
				w.file_total[(size_t)b.cnt_prev_file] += (uint64_t)*b.h_cnt_lead;
			for (size_t k = 0; k < b.cnt_starts.size(); k++)
				w.file_total[(size_t)b.cnt_files[k]] += (uint64_t)b.h_cnt_rows[k];
		}
	}
	const size_t chunks = b.chunks;
	const int R = c.max_results;
	w.last_state = b.h_results[chunks * R];
	if (c.rules) {
		collect_rules(w, b);
		b.chunks = 0;
		b.bytes = 0;
		w.rounds++;
		return;
	}
	long k_start = -1;   // -n: the file start the chunk lies behind (-1: its file began in an earlier buffer)
	if (c.lineno)
		w.lines += (size_t)b.h_line_info[1];
	for (size_t i = 0; i < chunks; i++) {
		while (c.lineno && k_start + 1 < (long)b.cnt_starts.size() && b.cnt_starts[(size_t)k_start + 1] <= b.starts[i])
			k_start++;
		const int n = b.h_results[i];
		w.matches += (size_t)n;
		for (int j = 0; j < n && j < R - 1; j++) {
			const int p_idx = b.h_results[(size_t)(j + 1) * chunks + i];
			int off = b.h_results2[(size_t)(j + 1) * chunks + i] + 1;  // end + 1 (databuf.c:771)
			if (c.wild)   // the record is the end of the last part's anchor: the match ends its post context behind
				off += w.sh->seq_post[p_idx];
			if (c.approx && !c.edit)   // the record is the end of the piece that found the match: the pattern ends its post behind (-e: the record is the match's)
				off += w.sh->apx_post[p_idx];
			w.reported++;
			if (!c.verbose)
				continue;
			pthread_mutex_lock(&w.sh->print_lock);
			if (c.seq) {
				printf("Sequence %d found in file '%s' at offset %d [relative: %d]\n", w.sh->seq_iid[p_idx],
				    w.sh->files[b.file_ids[i]].c_str(), off, off - b.h_indices[i]);
			} else if (c.lineno) {
				// newlines in front of the record less those in front of its file's start; a file that began
				// in an earlier buffer adds what those buffers counted for it
				const uint64_t d_rec = (uint64_t)b.h_results3[(size_t)(j + 1) * chunks + i];
				const uint64_t line = 1 + (k_start >= 0 ? d_rec - (uint64_t)b.h_start_line[k_start] : d_rec + w.line_carry);
				printf("Pattern %d ('%s') found in file '%s' at line %lu offset %d [relative: %d]\n",
				    w.sh->pat_iid[p_idx], w.sh->pat_bytes[p_idx].c_str(),
				    w.sh->files[b.file_ids[i]].c_str(), (unsigned long)line, off, off - b.h_indices[i]);
			} else if (c.edit) {
				printf("Pattern %d ('%s') found in file '%s' at offset %d [relative: %d] edits %d length %d\n",
				    w.sh->pat_iid[p_idx], w.sh->pat_bytes[p_idx].c_str(),
				    w.sh->files[b.file_ids[i]].c_str(), off, off - b.h_indices[i], b.h_results3[(size_t)(j + 1) * chunks + i],
				    b.h_results4[(size_t)(j + 1) * chunks + i]);
			} else if (c.approx) {
				printf("Pattern %d ('%s') found in file '%s' at offset %d [relative: %d] mismatches %d\n",
				    w.sh->pat_iid[p_idx], w.sh->pat_bytes[p_idx].c_str(),
				    w.sh->files[b.file_ids[i]].c_str(), off, off - b.h_indices[i], b.h_results3[(size_t)(j + 1) * chunks + i]);
			} else {
				printf("Pattern %d ('%s') found in file '%s' at offset %d [relative: %d]\n",
				    w.sh->pat_iid[p_idx], w.sh->pat_bytes[p_idx].c_str(),
				    w.sh->files[b.file_ids[i]].c_str(), off, off - b.h_indices[i]);
			}
			if (c.text_mode) {   // the matching line
				fwrite(b.h_data + b.h_indices[i], 1, (size_t)b.h_sizes[i], stdout);
			} else {             // some context around the match, up to a newline
				printf(" ... ");
				const int plen = c.seq ? 0 : (int)w.sh->pat_bytes[p_idx].size();
				const int lo = std::max(0, off - plen - 10);
				for (int k = lo; k < off + 10 && (size_t)k < b.bytes; k++) {
					if (b.h_data[k] == '\n')
						break;
					putchar(b.h_data[k]);
				}
				printf(" ... \n");
			}
			pthread_mutex_unlock(&w.sh->print_lock);
		}
	}
	if (c.lineno) {   // what the file this buffer ends in has counted so far
		const size_t ns = b.cnt_starts.size();
		const uint64_t all = (uint64_t)b.h_line_info[1];
		w.line_carry = ns ? all - (uint64_t)b.h_start_line[ns - 1] : w.line_carry + all;
	}
	b.chunks = 0;
	b.bytes = 0;
	w.rounds++;
}

void *worker_main(void *arg)
{
	Worker &w = *(Worker *)arg;
	Shared &sh = *w.sh;
	const Config &c = sh.cfg;
	CK(acm_rt_set_device(w.dev));
	CK(acm_rt_stream_create(&w.stream));
	w.ws_bytes = acm_scan_workspace_bytes(w.dfa, (size_t)c.global_ws * c.chunk);
	CK(acm_rt_malloc(&w.ws, w.ws_bytes));
	buffer_alloc(w.buf[0], c, w.stream);
	buffer_alloc(w.buf[1], c, w.stream);
	if (c.seq)
		for (Buffer &b : w.buf) {   // (the workspace depends on the uploaded set)
			b.seq_max = std::min((size_t)c.global_ws * c.chunk, kSeqMaxRecords);
			b.seq_ws_bytes = acm_sequence_workspace_bytes(w.dfa, b.seq_max);
			CK(acm_rt_malloc(&b.d_seq_pat, (b.seq_max + 2) * 4));
			CK(acm_rt_malloc(&b.d_seq_off, (b.seq_max + 2) * 4));
			CK(acm_rt_malloc(&b.d_seq_ws, b.seq_ws_bytes));
			CK(acm_rt_malloc(&b.d_seq_info, 16));
			if (c.rules) {
				b.rule_ws_bytes = acm_rule_workspace_bytes(w.dfa, b.seq_max);
				CK(acm_rt_malloc(&b.d_rule_out, (b.seq_max + 2) * 4));
				CK(acm_rt_malloc(&b.d_rule_text, (b.seq_max + 2) * 4));
				CK(acm_rt_malloc(&b.d_rule_off, (b.seq_max + 2) * 4));
				CK(acm_rt_malloc(&b.d_rule_ws, b.rule_ws_bytes));
				CK(acm_rt_malloc(&b.d_rule_info, 16));
				CK(acm_rt_host_alloc((void **)&b.h_rule_count, 64));
				*b.h_rule_count = 0;
			}
			if (c.wild) {
				b.wild_ws_bytes = acm_wildcard_workspace_bytes(b.all_cap);
				CK(acm_rt_malloc(&b.d_wild_pat, b.all_cap * 4));
				CK(acm_rt_malloc(&b.d_wild_off, b.all_cap * 4));
				CK(acm_rt_malloc(&b.d_wild_ws, b.wild_ws_bytes));
				CK(acm_rt_malloc(&b.d_wild_info, 16));
				CK(acm_rt_host_alloc((void **)&b.h_wild_info, 64));
				b.h_wild_info[0] = 0;
			}
		}
	if (c.edit)
		for (Buffer &b : w.buf) {
			b.apx_ws_bytes = acm_edit_workspace_bytes(w.dfa, b.all_cap - 2);
			CK(acm_rt_malloc(&b.d_apx_ws, b.apx_ws_bytes));
		}
	if (c.words || c.cased)
		for (void *&t : w.d_tail)
			CK(acm_rt_malloc(&t, (size_t)sh.max_pattern_len + 16));
	if (c.approx)
		for (void *&t : w.d_atail)
			CK(acm_rt_malloc(&t, (size_t)sh.apx_back + 16));
	const size_t npat = sh.pat_iid.size();
	if (c.count) {
		w.file_total.assign(sh.files.size(), 0);
		w.pat_total.assign(npat, 0);
		if (npat) {
			CK(acm_rt_malloc(&w.d_pat_total, npat * 8));
			CK(acm_rt_malloc(&w.d_one_class, npat * 4));
			CK(acm_rt_memset(w.d_pat_total, 0, npat * 8, w.stream));
			CK(acm_rt_memset(w.d_one_class, 0, npat * 4, w.stream));
		}
	}
	pthread_barrier_wait(&sh.ready);

	const int nfiles = (int)sh.files.size();
	int cur = w.id, filling = 0;
	bool in_flight = false;
	// text mode: one FILE per input, opened once (follow mode comes back to the same inputs
	// every millisecond: a fresh fdopen per visit would leak a stdio buffer each time)
	std::vector<FILE *> fps(c.text_mode ? (size_t)nfiles : 0, nullptr);
	auto stream_of = [&](int f) -> FILE * {
		if (!fps[(size_t)f])
			fps[(size_t)f] = fdopen(sh.fds[f], "r");
		else
			clearerr(fps[(size_t)f]);   // past an EOF seen earlier: data may have been appended
		return fps[(size_t)f];
	};
	FILE *fp = nullptr;
	if (cur < nfiles && c.text_mode)
		fp = stream_of(cur);
	const size_t G = (size_t)c.global_ws, size = G * (size_t)c.chunk;

	while (cur < nfiles) {
		Buffer &b = w.buf[filling];
		size_t got, lines = 0;
		if (c.text_mode)
			got = fill_text(b, c, fp, cur, &lines, &w.file_pos);
		else
			got = fill_binary(b, c, sh.fds[cur], cur, &w.file_pos);
		w.bytes += got;
		w.lines += lines;
		if (got)
			w.file_closed = false;
		const bool full = b.chunks >= G || b.bytes + 2 > size;
		bool file_done = (got == 0) && !full;
		if (file_done) {   // current file exhausted: next one of this worker
			w.file_closed = true;
			w.file_pos = 0;
			if (!c.follow) {
				if (fp) {
					fclose(fp);
					fps[(size_t)cur] = nullptr;
					fp = nullptr;
				} else {
					close(sh.fds[cur]);
				}
			}
			cur += c.threads;
			if (cur >= nfiles && c.follow && !g_terminate) {
				cur = w.id;   // keep polling the inputs (ocl_aho_grep.c:96-99)
				usleep(1000);
			}
			if (cur < nfiles && c.text_mode)
				fp = stream_of(cur);
		}
		const bool last = cur >= nfiles || g_terminate;
		if (b.chunks > 0 && (full || last || (c.follow && file_done))) {
			// the scan starts in the state the previous buffer ended in: taken from that buffer's planes on
			// the device, so this one is enqueued BEFORE the host waits for the previous one and walks its results
			if (c.rules && !w.file_closed && cur < nfiles) {
				// -K: a buffer filled to its end with a file's last bytes: the text is whole, not cut
				if (fp) {
					const int ch = fgetc(fp);
					if (ch == EOF)
						w.file_closed = true;
					else
						ungetc(ch, fp);
				} else {
					struct stat st;
					const off_t at = lseek(sh.fds[cur], 0, SEEK_CUR);
					if (at >= 0 && fstat(sh.fds[cur], &st) == 0 && S_ISREG(st.st_mode) && at >= st.st_size)
						w.file_closed = true;
				}
			}
			prepare(w, b);
			b.last_of_input = last;
			if (in_flight && c.words)   // b's first byte ends the previous buffer's stream
				finish(w, w.buf[filling ^ 1], first_byte(c, b));
			submit(w, b, in_flight ? &w.buf[filling ^ 1] : nullptr);   // GPU works on b while we read into the other buffer
			if (in_flight)
				collect(w, w.buf[filling ^ 1]);
			in_flight = true;
			filling ^= 1;
		}
		if (g_terminate)
			break;
	}
	if (in_flight) {
		if (c.words)   // the end of the worker's stream
			finish(w, w.buf[filling ^ 1], -1);
		collect(w, w.buf[filling ^ 1]);
	}
	if (c.count && npat) {   // the per-pattern totals come back once
		CK(acm_rt_memcpy_d2h(w.pat_total.data(), w.d_pat_total, npat * 8, w.stream));
		CK(acm_rt_stream_sync(w.stream));
	}
	return nullptr;
}

}  // namespace

int main(int argc, char **argv)
{
	// one hardware queue per worker stream (HIP's default is 4 per process; streams that share a
	// queue serialise).  Has to be in the environment before the first HIP call.
	setenv("GPU_MAX_HW_QUEUES", "8", 0);
	Shared sh;
	Config &c = sh.cfg;
	int opt;
	while ((opt = getopt(argc, argv, "f:m:p:tw:vxB:D:FG:L:R:MhAiSWcnI:P:Q:EK:Xor:O:C:VT:HNbk:ez:")) != -1) {   // ocl_aho_grep.c:411 + A, i, S, W, c, n, I, P, Q, E, K, X, o, r, O, C, V, T, H, N, b, k, e, z
		switch (opt) {
		case 'f': c.data_path = optarg; break;
		case 'm': c.pat_limit = atoi(optarg); break;
		case 'p': c.pat_path = optarg; break;
		case 't': c.text_mode = 1; break;
		case 'w': c.threads = atoi(optarg); break;
		case 'v': c.verbose = 1; break;
		case 'x': c.hex = 1; break;
		case 'B': c.chunk = atol(optarg); break;
		case 'D':   // one device, or a comma-separated list: the workers are dealt over it
			c.devs.clear();
			for (const char *q = optarg; *q;) {
				c.devs.push_back(atoi(q));
				while (*q && *q != ',')
					q++;
				if (*q == ',')
					q++;
			}
			c.dev = c.devs.empty() ? -1 : c.devs[0];
			break;
		case 'F': c.follow = 1; break;
		case 'G': c.global_ws = atol(optarg); break;
		case 'L': c.local_ws = atol(optarg); break;
		case 'R': c.max_results = atoi(optarg); break;
		case 'M': break;
		case 'A': c.all_patterns = 1; break;
		case 'i': c.nocase = 1; break;
		case 'S': c.segmented = 1; break;
		case 'W': c.words = 1; break;
		case 'c': c.count = 1; break;
		case 'n': c.lineno = 1; break;
		case 'I': c.loose_path = optarg; break;
		case 'P': c.pos_path = optarg; break;
		case 'Q': c.seq_path = optarg; break;
		case 'E': c.ext = 1; break;
		case 'X': c.grp = 1; break;
		case 'o': c.only = 1; break;
		case 'r': c.repl_path = optarg; break;
		case 'O': c.out_dir = optarg; break;
		case 'K': c.rule_path = optarg; break;
		case 'C': {   // N or N,M: decimal digits only
			const std::string v = optarg;
			const size_t comma = v.find(',');
			const std::string a = v.substr(0, comma), z = comma == std::string::npos ? a : v.substr(comma + 1);
			auto digits = [](const std::string &x) { return !x.empty() && x.size() <= 9 && x.find_first_not_of("0123456789") == std::string::npos; };
			c.ctx = digits(a) && digits(z) ? 1 : -1;
			if (c.ctx == 1) {
				c.ctx_before = atoi(a.c_str());
				c.ctx_after = atoi(z.c_str());
			}
			break;
		}
		case 'V': c.invert = 1; break;
		case 'T': c.ext_dir = optarg; break;
		case 'H': c.fmt_name = 1; break;
		case 'N': c.fmt_num = 1; break;
		case 'b': c.fmt_off = 1; break;
		case 'k': {   // decimal digits only; 0 and junk are refused below
			const std::string v = optarg;
			c.approx = !v.empty() && v.size() <= 2 && v.find_first_not_of("0123456789") == std::string::npos ? atoi(v.c_str()) : -1;
			if (c.approx == 0)
				c.approx = -1;
			break;
		}
		case 'e': c.edit = 1; break;
		case 'z': c.norm_spec = optarg; c.norm = 1; break;
		default: usage();
		}
	}
	int err = 0;   // check_args, ocl_aho_grep.c:210-266
	c.rules = !c.rule_path.empty();
	c.seq = !c.seq_path.empty() || c.rules;   // (-K: the rule pass takes the sequence pass's records)
	if (c.pat_path.empty() && !c.seq) { printf("ERROR: No pattern file\n"); err++; }
	else if (!c.pat_path.empty() && access(c.pat_path.c_str(), R_OK) != 0) {
		printf("ERROR: File '%s' does not exist\n", c.pat_path.c_str()); err++;
	}
	if (c.data_path.empty()) { printf("ERROR: No data file\n"); err++; }
	if (c.dev == -1) { printf("ERROR: No device position\n"); err++; }
	if (c.global_ws == -1) { printf("ERROR: No global work size\n"); err++; }
	if (c.local_ws == -1) { printf("ERROR: No local work size\n"); err++; }
	if (c.chunk == -1) { printf("ERROR: No maximum chunk size\n"); err++; }
	if (c.threads <= 0) { printf("ERROR: The thread number must be greater than 0\n"); err++; }
	if (c.pat_limit != -1 && c.pat_limit <= 0) { printf("ERROR: The pattern size limit should be >= 1\n"); err++; }
	if (c.pat_limit >= 4096) { printf("ERROR: The pattern size limit should be <= 4095\n"); err++; }
	if (c.max_results <= 0) { printf("ERROR: The maximum result cells should be >= 1\n"); err++; }
	if (c.words && c.follow) {   // a buffer's word test needs the byte after it, unknown while the input pauses
		printf("ERROR: -W cannot be combined with -F: the byte after a paused input is not known\n");
		err++;
	}
	if (!c.loose_path.empty() && access(c.loose_path.c_str(), R_OK) != 0) {
		printf("ERROR: File '%s' does not exist\n", c.loose_path.c_str()); err++;
	}
	if (!c.loose_path.empty() && (c.words || c.follow)) {   // the word pass takes states, the case pass gives patterns
		printf("ERROR: -I cannot be combined with -W or -F: the case pass and those are not composed\n");
		err++;
	}
	c.cased = !c.loose_path.empty() && !c.nocase;
	if (!c.pos_path.empty() && access(c.pos_path.c_str(), R_OK) != 0) {
		printf("ERROR: File '%s' does not exist\n", c.pos_path.c_str()); err++;
	}
	if (!c.pos_path.empty() && !c.segmented) {   // a window counts from the bounds of a text: the texts must be told apart
		printf("ERROR: -P needs -S: a position counts from the start or the end of a file (with -t: of a line)\n");
		err++;
	}
	if (!c.pos_path.empty() && c.follow) {
		printf("ERROR: -P cannot be combined with -F: the end of a paused input is not known\n");
		err++;
	}
	c.pos = !c.pos_path.empty();
	if (!c.seq_path.empty() && access(c.seq_path.c_str(), R_OK) != 0) {
		printf("ERROR: File '%s' does not exist\n", c.seq_path.c_str()); err++;
	}
	if (c.rules && access(c.rule_path.c_str(), R_OK) != 0) {
		printf("ERROR: File '%s' does not exist\n", c.rule_path.c_str()); err++;
	}
	if (c.rules && (c.count || c.lineno || c.words || c.all_patterns)) {   // the records are rules that hold, not patterns
		printf("ERROR: -K cannot be combined with -c, -n, -W or -A: the records of -K are rules that hold\n");
		err++;
	} else if (c.seq && (c.count || c.lineno || c.words || c.all_patterns)) {   // the records are sequence matches, not patterns
		printf("ERROR: -Q cannot be combined with -c, -n, -W or -A: the records of -Q are signature matches\n");
		err++;
	}
	if (c.rules && !c.segmented) {   // a condition counts the hits of one text: the texts must be told apart
		printf("ERROR: -K needs -S: a rule is a condition over the hits in one file (with -t: in one line)\n");
		err++;
	}
	if (c.rules && c.follow) {
		printf("ERROR: -K cannot be combined with -F: the end of a paused input is not known\n");
		err++;
	}
	if (c.ext && !c.seq) {
		printf("ERROR: -E needs -Q or -K: it is the syntax of the signature file\n");
		err++;
	}
	if (c.grp && !c.ext) {
		printf("ERROR: -X needs -E\n");
		err++;
	}
	if (c.ext && c.words) {
		printf("ERROR: -E cannot be combined with -W: the word pass looks at the bytes next to a part's exact run\n");
		err++;
	}
	if (c.lineno && c.text_mode) {
		printf("ERROR: -n needs binary mode: -t already makes every line a chunk\n");
		err++;
	}
	if (!c.repl_path.empty() && c.out_dir.empty()) {
		printf("ERROR: -r needs -O: the directory the rewritten files go to\n");
		err++;
	}
	if (c.repl_path.empty() && !c.out_dir.empty()) {
		printf("ERROR: -O needs -r: the replacements\n");
		err++;
	}
	if (!c.repl_path.empty() && access(c.repl_path.c_str(), R_OK) != 0) {
		printf("ERROR: File '%s' does not exist\n", c.repl_path.c_str()); err++;
	}
	c.rewrite = !c.repl_path.empty() && !c.out_dir.empty();
	if ((!c.repl_path.empty() || !c.out_dir.empty()) &&
	    (c.text_mode || c.all_patterns || c.count || c.lineno || c.seq || c.ext || c.follow)) {   // the rewrite is of -o's matches, of whole buffers
		printf("ERROR: -r cannot be combined with -t, -A, -c, -n, -Q, -K, -E or -F: it rewrites the matches -o selects\n");
		err++;
	} else if (c.rewrite) {
		c.only = 1;
	}
	if (c.only && (c.all_patterns || c.count || c.lineno || c.seq || c.ext || c.follow)) {   // the records are a selection of -A's
		printf("ERROR: -o cannot be combined with -A, -c, -n, -Q, -K, -E or -F: the records of -o are the selected matches\n");
		err++;
	}
	if (c.ctx < 0) {
		printf("ERROR: -C takes N or N,M: the lines in front and behind, both >= 0\n");
		err++;
	}
	if (c.ctx && c.ext_dir.empty()) {
		printf("ERROR: -C needs -T: the directory the extracted lines go to\n");
		err++;
	}
	if (c.invert && (!c.ctx || c.ext_dir.empty())) {
		printf("ERROR: -V needs -C and -T: it inverts the selection of the lines that are extracted\n");
		err++;
	}
	c.fmt = c.fmt_name || c.fmt_num || c.fmt_off;
	if (c.fmt && (!c.ctx || c.ext_dir.empty())) {
		printf("ERROR: -H, -N and -b need -C and -T: they put a prefix in front of the lines that are extracted\n");
		err++;
	}
	if (!c.ctx && !c.ext_dir.empty()) {
		printf("ERROR: -T needs -C: the lines of context around a selected line (-C 0: none)\n");
		err++;
	}
	if ((c.ctx || c.invert || !c.ext_dir.empty()) &&
	    (c.text_mode || c.follow || !c.repl_path.empty() || !c.out_dir.empty() || c.seq)) {   // the lines of whole files, around pattern records
		printf("ERROR: -C, -V and -T cannot be combined with -t, -F, -r, -O, -Q or -K: the lines of whole files are extracted, "
		       "around the records of patterns\n");
		err++;
	}
	c.extract = c.ctx == 1 && !c.ext_dir.empty();
	if (c.approx < 0 || c.approx > ACM_APPROX_MAX_K) {
		printf("ERROR: -k takes 1 to %d: the bytes of a pattern that may be other bytes\n", ACM_APPROX_MAX_K);
		err++;
	} else if (c.edit && (c.approx == 0 || c.approx > ACM_EDIT_MAX_K)) {
		printf("ERROR: -e needs -k N with N from 1 to %d: the bytes that may be substituted, inserted or deleted\n", ACM_EDIT_MAX_K);
		err++;
	} else if (c.approx) {
		const struct { bool on; const char *opt, *why; } refused[] = {
			{ c.words != 0, "-W", "the word pass looks at the bytes next to a piece, not next to the match" },
			{ !c.pos_path.empty(), "-P", "a window would count from a piece's start, not from the match's" },
			{ !c.seq_path.empty(), "-Q", "a part of a signature is matched exactly" },
			{ c.rules != 0, "-K", "the bodies of a rule are matched exactly" },
			{ c.ext != 0, "-E", "it is the syntax of the signature file" },
			{ c.only != 0 && c.repl_path.empty() && c.out_dir.empty(), "-o", "the select pass would take a piece for the match" },
			{ !c.repl_path.empty() || !c.out_dir.empty(), "-r", "the rewrite would replace a piece, not the match" },
			{ c.count != 0 && !c.edit, "-c", "the tallies would count pieces" },   // (-e: the records are whole matches, each once)
			{ c.lineno != 0, "-n", "the line would be that of the piece's end, not of the match's" },
			{ c.ctx != 0 || c.invert || !c.ext_dir.empty(), "-C", "the lines would be those of the pieces' ends" },
			{ c.follow != 0, "-F", "the bytes behind a paused input are not known" },
		};
		for (const auto &r : refused)
			if (r.on) {
				printf("ERROR: -k cannot be combined with %s: %s\n", r.opt, r.why);
				err++;
			}
	}
	if (c.norm) {
		// SPEC: a comma list of url and at most one of ws, strip, nul
		int blanks = 0;
		bool bad = c.norm_spec.empty();
		for (size_t at = 0; at <= c.norm_spec.size() && !bad;) {
			const size_t comma = std::min(c.norm_spec.find(',', at), c.norm_spec.size());
			const std::string word = c.norm_spec.substr(at, comma - at);
			if (word == "url" && !(c.norm_flags & ACM_NORM_PERCENT)) {
				c.norm_flags |= ACM_NORM_PERCENT;
			} else if ((word == "ws" || word == "strip" || word == "nul") && !blanks++) {
				c.norm_flags |= word == "ws" ? ACM_NORM_SQUEEZE : ACM_NORM_STRIP;
				c.norm_nul = word == "nul";
			} else {
				bad = true;
			}
			at = comma + 1;
		}
		if (bad) {
			printf("ERROR: -z takes a comma list of 'url' and at most one of 'ws', 'strip' and 'nul', each once: not '%s'\n",
			    c.norm_spec.c_str());
			err++;
		}
		if (!c.segmented) {   // a blank run and a triple end with their text: the texts must be told apart
			printf("ERROR: -z needs -S: a file (with -t: a line) is normalised as a text of its own\n");
			err++;
		}
		// the passes that read the text or count in its coordinates are each a follow-up: which coordinates?
		const struct { bool on; const char *opt; } refused[] = {
			{ c.lineno != 0, "-n" }, { c.ctx != 0, "-C" }, { !c.ext_dir.empty(), "-T" }, { c.only != 0 && c.repl_path.empty(), "-o" },
			{ !c.repl_path.empty(), "-r" }, { !c.out_dir.empty(), "-O" }, { c.fmt_name != 0, "-H" }, { c.fmt_num != 0, "-N" },
			{ c.fmt_off != 0, "-b" }, { c.approx != 0, "-k" }, { c.edit != 0, "-e" }, { !c.pos_path.empty(), "-P" },
			{ !c.seq_path.empty(), "-Q" }, { c.rules != 0, "-K" }, { c.ext != 0, "-E" }, { c.grp != 0, "-X" }, { c.invert != 0, "-V" },
			{ c.follow != 0, "-F" },
		};
		for (const auto &r : refused)
			if (r.on) {
				printf("ERROR: -z cannot be combined with %s: lines, ranges, positions and signatures over a normalised scan are "
				       "not provided\n", r.opt);
				err++;
			}
	}
	if (err)
		usage();
	if (c.approx)   // the approx pass takes every pattern of every record: the planes -A would have printed
		c.all_patterns = 1;
	if (c.only)   // the select pass takes every pattern of every record: the planes -A would have printed
		c.all_patterns = 1;
	auto align16 = [](long &v, const char *what) {   // align_parameters, ocl_aho_grep.c:316-346
		if (v % 16) {
			printf("WARNING: %s '%ld' is not 16B aligned. ", what, v);
			v = (v + 15) & ~15L;
			printf("Will use '%ld' instead\n", v);
		}
	};
	align16(c.local_ws, "local work size");
	align16(c.global_ws, "global work size");
	align16(c.chunk, "max chunk size");
	printf("Local Work Size:  %ld\nGlobal Work Size: %ld\nMax Chunk Size:   %ld\n\n", c.local_ws,
	    c.global_ws, c.chunk);

	struct rlimit rl;
	if (getrlimit(RLIMIT_NOFILE, &rl) == 0 && rl.rlim_cur < rl.rlim_max) {
		rl.rlim_cur = rl.rlim_max;
		setrlimit(RLIMIT_NOFILE, &rl);
	}

	// inputs: a directory, one file, or comma-separated files
	std::vector<std::string> names;
	if (is_dir(c.data_path)) {
		names = regular_files_in(c.data_path);
	} else {
		size_t a = 0;
		while (a <= c.data_path.size()) {
			size_t b = c.data_path.find(',', a);
			if (b == std::string::npos)
				b = c.data_path.size();
			if (b > a)
				names.push_back(c.data_path.substr(a, b - a));
			a = b + 1;
		}
	}
	for (auto &f : names) {
		if (!is_readable_input(f))
			continue;
		int fd = open(f.c_str(), O_RDONLY);
		if (fd == -1) {
			fprintf(stderr, "ERROR: could not open '%s'\n\n", f.c_str());
			return 1;
		}
		sh.files.push_back(f);
		sh.fds.push_back(fd);
	}
	if (sh.files.empty()) {
		fprintf(stderr, "ERROR: Could not open input file(s) for reading.\n\n");
		return 1;
	}

	// one automaton, one copy per device, shared by the workers of that device
	acm_automaton *aut = acm_automaton_new();
	CK(acm_automaton_set_nocase(aut, c.nocase));
	// -k: the files are read into an automaton of their own, and every pattern is added from there: with a budget
	// where it is long enough for pieces of three bytes, as it is where not
	acm_automaton *read_into = c.approx ? acm_automaton_new() : aut;
	if (!c.pat_path.empty() && acm_automaton_load_file(read_into, c.pat_path.c_str(), c.hex, c.pat_limit) < 0) {
		fprintf(stderr, "ERROR: init_ocl_worker_ctx\n%s\n", acm_last_error());
		return 1;
	}
	if (!c.loose_path.empty() &&
	    acm_automaton_load_file_ex(read_into, c.loose_path.c_str(), c.hex, c.pat_limit, ACM_PATTERN_NOCASE) < 0) {
		fprintf(stderr, "ERROR: init_ocl_worker_ctx\n%s\n", acm_last_error());
		return 1;
	}
	if (c.approx) {
		int exact = 0;
		for (int i = 0; i < acm_automaton_num_patterns(read_into); i++) {
			int iid = 0, n = 0;
			const unsigned char *bytes = nullptr;
			acm_automaton_pattern(read_into, i, &iid, &n, &bytes, nullptr);
			const bool tolerant = n >= 3 * (c.approx + 1);
			exact += !tolerant;
			const unsigned flags = (unsigned)acm_automaton_pattern_flags(read_into, i);
			if ((c.edit ? acm_automaton_add_edit(aut, bytes, n, tolerant ? c.approx : 0, iid, flags)
			            : acm_automaton_add_approx(aut, bytes, n, tolerant ? c.approx : 0, iid, flags)) < 0) {
				fprintf(stderr, "ERROR: init_ocl_worker_ctx\n%s\n", acm_last_error());
				return 1;
			}
		}
		acm_automaton_free(read_into);
		if (exact)
			fprintf(stderr, "NOTE: %d patterns have fewer than %d bytes and stay exact under -k %d\n", exact, 3 * (c.approx + 1), c.approx);
	}
	const unsigned syntax = c.ext ? (c.grp ? ACM_SIG_EXTENDED | ACM_SIG_GROUPS : ACM_SIG_EXTENDED) : 0;
	if (!c.seq_path.empty() && acm_automaton_load_signature_file_ex(aut, c.seq_path.c_str(), 0, syntax) < 0) {
		fprintf(stderr, "ERROR: init_ocl_worker_ctx\n%s\n", acm_last_error());
		return 1;
	}
	if (c.rules && acm_automaton_load_logical_file(aut, c.rule_path.c_str(), 0, syntax) < 0) {
		fprintf(stderr, "ERROR: init_ocl_worker_ctx\n%s\n", acm_last_error());
		return 1;
	}
	for (int i = 0; i < acm_automaton_num_rules(aut); i++) {
		int iid = 0;
		acm_automaton_rule(aut, i, &iid, nullptr, nullptr, nullptr);
		sh.rule_iid.push_back(iid);
	}
	c.wild = c.ext && acm_automaton_wildcards(aut);
	for (int i = 0; i < acm_automaton_num_sequences(aut); i++) {
		int iid = 0, nparts = 0, post = 0;
		const int32_t *parts = nullptr;
		acm_automaton_sequence(aut, i, &iid, &nparts, &parts, nullptr, nullptr);
		sh.seq_iid.push_back(iid);
		if (nparts > 0)
			acm_automaton_pattern_wildcard(aut, parts[nparts - 1], nullptr, &post, nullptr, nullptr);
		sh.seq_post.push_back(post);
	}
	if (c.pos && acm_automaton_load_position_file(aut, c.pos_path.c_str()) < 0) {
		fprintf(stderr, "ERROR: init_ocl_worker_ctx\n%s\n", acm_last_error());
		return 1;
	}
	if (c.rewrite && acm_automaton_load_replacement_file(aut, c.repl_path.c_str()) < 0) {
		fprintf(stderr, "ERROR: init_ocl_worker_ctx\n%s\n", acm_last_error());
		return 1;
	}
	if (c.fmt) {   // the longest prefix: a path (-H), a line number and an offset of a buffer (int32), a separator each
		size_t longest = 0;
		for (const std::string &f : sh.files)
			longest = std::max(longest, f.size());
		if (c.fmt_name && longest > ACM_FORMAT_MAX_NAME) {
			fprintf(stderr, "ERROR: -H: an input path has %zu bytes, a name at most %d\n", longest, ACM_FORMAT_MAX_NAME);
			return 1;
		}
		c.fmt_width = (c.fmt_name ? longest + 1 : 0) + (c.fmt_num ? 11 : 0) + (c.fmt_off ? 11 : 0);
	}
	if (c.rewrite || c.extract) {   // a file of a directory or a list goes to <-O>/<its name> (-C: <-T>/<its name>)
		const char *opt_name = c.rewrite ? "-O" : "-T";
		for (const std::string &f : sh.files) {
			const size_t slash = f.rfind('/');
			sh.out_paths.push_back((c.rewrite ? c.out_dir : c.ext_dir) + "/" + (slash == std::string::npos ? f : f.substr(slash + 1)));
		}
		sh.out_begun.assign(sh.files.size(), 0);
		// two inputs of one name (a list over several directories) would share an output, and an output that is an
		// input (-O names the directory of -f) would be truncated while it is read: both are refused before anything runs
		std::map<std::string, size_t> seen;
		std::set<std::pair<dev_t, ino_t>> inputs;
		for (size_t f = 0; f < sh.files.size(); f++) {
			auto at = seen.emplace(sh.out_paths[f], f);
			if (!at.second) {
				fprintf(stderr, "ERROR: %s: '%s' and '%s' would both be written to '%s'\n", opt_name, sh.files[at.first->second].c_str(),
				    sh.files[f].c_str(), sh.out_paths[f].c_str());
				return 1;
			}
			struct stat st;
			if (fstat(sh.fds[f], &st) == 0)
				inputs.insert({ st.st_dev, st.st_ino });
		}
		for (size_t f = 0; f < sh.files.size(); f++) {
			struct stat st;
			if (stat(sh.out_paths[f].c_str(), &st) == 0 && inputs.count({ st.st_dev, st.st_ino })) {
				fprintf(stderr, "ERROR: %s: the output '%s' is an input file; give %s another directory\n", opt_name, sh.out_paths[f].c_str(),
				    opt_name);
				return 1;
			}
		}
	}
	CK(acm_automaton_compile(aut));
	const int states = acm_automaton_num_states(aut);
	const int np = acm_automaton_num_patterns(aut);
	for (int i = 0; i < np; i++) {
		int iid = 0, n = 0;
		const unsigned char *bytes = nullptr;
		acm_automaton_pattern(aut, i, &iid, &n, &bytes, nullptr);
		int x = -1, post = 0;
		if (acm_automaton_pattern_approx(aut, i, &x, nullptr, nullptr, &post) == 1)   // a piece: the -v line names its whole pattern
			acm_automaton_approx(aut, x, nullptr, &n, nullptr, nullptr, nullptr, &bytes);
		sh.pat_iid.push_back(iid);
		sh.pat_bytes.emplace_back((const char *)bytes, (size_t)n);
		sh.apx_post.push_back(post);
	}
	acm_automaton_approx_reach(aut, &sh.apx_back, nullptr);
	for (int dev : c.devs) {
		acm_dfa *dfa = nullptr;
		if (acm_dfa_upload(aut, dev, &dfa) != ACM_OK) {
			fprintf(stderr, "invalid dev pos\n%s\n", acm_last_error());
			return 1;
		}
		sh.dfas.push_back(dfa);
	}
	const size_t automaton_bytes = acm_dfa_device_bytes(sh.dfas[0]);
	sh.max_pattern_len = acm_automaton_max_pattern_len(aut);
	acm_automaton_free(aut);

	signal(SIGINT, on_sigint);
	std::vector<Worker> workers((size_t)c.threads);
	pthread_barrier_init(&sh.ready, nullptr, (unsigned)c.threads + 1);
	for (int i = 0; i < c.threads; i++) {
		workers[i].sh = &sh;
		workers[i].id = i;
		workers[i].dev = c.devs[(size_t)i % c.devs.size()];
		workers[i].dfa = sh.dfas[(size_t)i % c.devs.size()];
		if (pthread_create(&workers[i].thread, nullptr, worker_main, &workers[i]) != 0) {
			fprintf(stderr, "ERROR: creating thread: %d\n\n", i);
			return 1;
		}
	}
	pthread_barrier_wait(&sh.ready);
	const double t0 = now_us();
	size_t matches = 0, reported = 0, bytes = 0, lines = 0, rounds = 0;
	uint64_t undecided = 0, wild_undecided = 0, cut_texts = 0, sel_dropped = 0, apx_undecided = 0;
	for (auto &w : workers) {
		pthread_join(w.thread, nullptr);
		undecided += w.undecided;
		wild_undecided += w.wild_undecided;
		apx_undecided += w.apx_undecided;
		cut_texts += w.cut_texts;
		sel_dropped += w.sel_dropped;
		matches += w.matches;
		reported += w.reported;
		bytes += w.bytes;
		lines += w.lines;
		rounds += w.rounds;
	}
	const double secs = (now_us() - t0) / 1e6;
	for (size_t f = 0; (c.rewrite || c.extract) && f < sh.files.size(); f++)
		if (!sh.out_begun[f]) {   // a file of no bytes: no buffer held a piece of it
			make_parents(sh.out_paths[f]);
			if (FILE *fp = fopen(sh.out_paths[f].c_str(), "wb"))
				fclose(fp);
		}
	if (c.count) {
		std::vector<uint64_t> per_file(sh.files.size(), 0), per_pat(sh.pat_iid.size(), 0);
		for (auto &w : workers) {
			for (size_t i = 0; i < per_file.size(); i++)
				per_file[i] += w.file_total[i];
			for (size_t i = 0; i < per_pat.size(); i++)
				per_pat[i] += w.pat_total[i];
		}
		for (size_t i = 0; i < per_file.size(); i++)
			printf("Count file '%s': %lu\n", sh.files[i].c_str(), (unsigned long)per_file[i]);
		for (size_t i = 0; i < per_pat.size(); i++)
			if (per_pat[i])
				printf("Count pattern %d ('%s'): %lu\n", sh.pat_iid[i], sh.pat_bytes[i].c_str(), (unsigned long)per_pat[i]);
	}
	printf("-------------- STATS --------------\n");   // ocl_aho_grep.c:615-631
	printf("Matches:             %lu\n", (unsigned long)matches);
	printf("Matches reported:    %lu\n", (unsigned long)reported);
	printf("Time (secs):         %.5f\n", secs);
	printf("Automaton states:    %d\n", states);
	printf("Automaton size (MB): %.3f\n", (double)automaton_bytes / 1048576);
	printf("Processed bytes:     %lu\n", (unsigned long)bytes);
	if (lines || c.lineno)
		printf("Processed lines:     %lu\n", (unsigned long)lines);
	printf("Processed files:     %d\n", (int)sh.files.size());
	printf("Kernel launches:     %d\n", (int)rounds);
	printf("Throughput (Mbps):   %.3f\n", ((double)(bytes * 8) / 1048576) / secs);
	printf("-----------------------------------\n\n");
	for (acm_dfa *dfa : sh.dfas)
		acm_dfa_release(dfa);
	if (wild_undecided)   // no silent loss: a signature cut by a buffer border is not found, and here that is known
		fprintf(stderr, "NOTE: %lu wildcard candidates reach over a buffer border and were not decided (raise -B/-G)\n",
		    (unsigned long)wild_undecided);
	if (apx_undecided)   // no silent loss: a match cut by a buffer's end is not found, and here that is known
		fprintf(stderr, "NOTE: %lu approximate candidates reach behind a buffer's end and were not decided (raise -B/-G)\n",
		    (unsigned long)apx_undecided);
	if (cut_texts)   // no silent loss: the rules of these texts were not evaluated
		fprintf(stderr, "NOTE: %lu texts are cut by a buffer border and their rules were not evaluated (use a larger -G/-B)\n",
		    (unsigned long)cut_texts);
	if (sel_dropped)   // no silent loss: a match that began in the buffer in front could have been the leftmost
		fprintf(stderr, "NOTE: %lu matches began in the buffer in front and were not candidates of -o (use a larger -G/-B)\n",
		    (unsigned long)sel_dropped);
	if (undecided) {   // no silent loss: the counts and records above are without them
		printf("ERROR: %lu end-anchored candidates lie in files that span buffers (raise -B/-G)\n", (unsigned long)undecided);
		return 1;
	}
	return 0;
}
