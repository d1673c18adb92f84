"""acm_grep -K -E -X -S and -Q -E -X -S over several buffers: the generated database with groups of
test_gpu_signature_chain_groups.py (signature_oracle.make(group_share=...)) and 300 short texts of its corpus
written as files.  What must be printed comes from tests/signature_oracle.py alone.  A rule or signature file has
one case flag for all its lines and the command line sets no windows, so the oracle runs the database without its
windows and with no body ignoring case.

The wildcard pass of acm_grep is given no bytes of the buffer in front and the sequence pass joins no parts across
buffers, so of a file that a buffer border cuts -Q finds for certain only the matches that one buffer's share of the
file holds whole: the oracle's matches with every such share as a text of its own.  The others, matches that need
bytes of two buffers, may be missing (one is printed where a plain first part's anchor alone lies across the
border: the scan carries its state over).  -K does not evaluate a cut file at all."""
import os
import re
from collections import Counter

import pytest

import signature_oracle as so
import wildcard_model as wm
from test_gpu_rules_cli import run as run_rules
from test_gpu_sequences_cli import run as run_sequences
from test_gpu_signature_chain import SEED
from test_gpu_signature_chain_cli import B, CUT, LARGE_G, SMALL_G, cut_files
from test_gpu_signature_chain_groups import GROUP_MAKE

pytestmark = pytest.mark.gpu

UNDECIDED = re.compile(r"^NOTE: (\d+) wildcard candidates reach over a buffer border", re.M)


class Inputs:
    def __init__(self, tmp):
        g = so.make(SEED, **GROUP_MAKE)
        self.lines = g.lines
        self.texts, self.chunks = so.small_slice(g.texts, chunk=B, longest=1200)      # (of at most 1200 bytes: see the test below)
        d = tmp / "in"
        d.mkdir()
        self.names = ["f%03d.bin" % i for i in range(len(self.texts))]
        for name, t in zip(self.names, self.texts):
            (d / name).write_bytes(t)
        self.path = ",".join(os.path.join(str(d), n) for n in self.names)      # -f a,b,...: the files in this order
        self.rules = str(tmp / "rules.ldb")
        with open(self.rules, "w") as f:
            f.write("# generated\n" + "".join("%d:%s\n" % (1000 + r, line) for r, line in enumerate(g.lines)))
        self.bodies = [b for line in g.lines for b in so.split_line(line)[1]]
        self.sigs = str(tmp / "sigs.ndb")
        with open(self.sigs, "w") as f:
            f.write("".join("%d:%s\n" % (500 + q, b) for q, b in enumerate(self.bodies)))
        self.db = so.Database(self.lines, groups=True)
        self.corpus = so.Corpus(self.texts)
        self.found = so.sequences(self.db, self.corpus)

    def rule_lines(self):
        return sorted((self.names[t], 1000 + r, 0) for r, t, _ in so.rules(self.db, self.corpus, self.found))

    def signature_lines(self, shares=None):
        """the -Q lines: the match's end relative to the chunk that holds the end of its last part's anchor.  shares:
        {file name: [where a buffer's share of the file begins, ...]}: every share is a text of its own"""
        texts, names = [], []
        for name, t in zip(self.names, self.texts):
            cuts = [0] + list((shares or {}).get(name, [])) + [len(t)]
            for a, b in zip(cuts, cuts[1:]):
                texts.append(t[a:b])                     # (a share begins a chunk: offsets keep their place in it)
                names.append(name)
        c = so.Corpus(texts) if shares else self.corpus
        found = so.sequences(self.db, c) if shares else self.found
        return sorted((names[int(c.text_of[a])], 500 + int(q), int((a - c.t0[a]) % B + e - a)) for e, a, q in zip(*found))

    def args(self, flag, file, G, w, groups=True):
        return ["-f", self.path, flag, file, "-E"] + (["-X"] if groups else []) + \
            ["-S", "-B", str(B), "-D", "0", "-G", str(G), "-L", "64", "-w", str(w), "-R", "128", "-v"]


@pytest.fixture(scope="module")
def inputs(gpu, tmp_path_factory):
    return Inputs(tmp_path_factory.mktemp("chain_groups"))


def shares_of(inputs, w, G=SMALL_G):
    """{file: the offsets in it at which another buffer begins}, by the deal that cut_files describes: worker i takes
    files i, i + w, ... and lays them chunk by chunk into buffers of G chunks"""
    out = {}
    for i in range(w):
        at = 0
        for k in range(i, len(inputs.texts), w):
            n = -(-len(inputs.texts[k]) // B)
            where = [c * B for c in range(1, n) if (at + c) % G == 0]
            if where:
                out[inputs.names[k]] = where
            at += n
    return out


def reach_in_front(inputs, shares):
    """the candidates of the wildcard pass (an anchor of a part, whatever lies around it) whose anchor lies in a buffer,
    whose span lies in the file and has a group reaching into the buffer in front: a lower bound of what the pass
    cannot decide (no file is larger than a buffer: a border cuts a file once)"""
    c, n = inputs.corpus, 0
    for parts, _ in inputs.db.sigs:
        for p in parts:
            if not p.groups:
                continue
            k = so.occurrences(c, p.tables()[p.at:p.at + p.L]) - p.at    # the part's first position, were it to hold
            for name, where in shares.items():
                f = inputs.names.index(name)
                t0, tend = int(c.starts[f]), int(c.starts[f]) + len(inputs.texts[f])
                (s,) = where
                here = k[(k + p.at >= t0 + s) & (k >= t0) & (k + p.n <= tend)]
                n += int((here + p.groups[0][0] < t0 + s).sum())
    return n


def test_the_files_are_worth_running(inputs):
    """from sizes and the oracle alone.  (With the texts of at most 900 bytes that small_slice takes by default, no
    file that a border cuts with -w 1 has a rule line; the longest text of this corpus behind the long one has 978.)"""
    assert len(inputs.texts) == 300 and inputs.chunks * B <= LARGE_G * B and max(len(t) for t in inputs.texts) < SMALL_G * B
    rules, sigs = inputs.rule_lines(), inputs.signature_lines()
    print("%d bytes in %d chunks; %d rule lines, %d signature lines" % (inputs.corpus.N, inputs.chunks, len(rules), len(sigs)))
    assert len(rules) > 30 and len({i for _, i, _ in rules}) > 15 and len(sigs) > 200 and max(r for _, _, r in sigs) >= B
    loose = so.sequences(inputs.db, inputs.corpus, groups=False)
    assert loose[0].size > inputs.found[0].size                           # the groups decide
    for w in (1, 2):
        cut, shares = cut_files(inputs, w), shares_of(inputs, w)
        assert set(shares) == cut and 10 <= len(cut) <= len(inputs.texts) // 10
        assert {n for n, _, _ in rules} & cut                             # a cut file with a line of the oracle's
        whole, split = set(sigs), set(inputs.signature_lines(shares))
        print("-w %d: %d files cut; %d of the %d signature lines need bytes of two buffers; %d candidates with a group "
              "that reaches the buffer in front" % (w, len(cut), len(whole - split), len(whole), reach_in_front(inputs, shares)))
        assert split < whole and {n for n, _, _ in whole - split} <= cut
        assert reach_in_front(inputs, shares) > 0
    assert cut_files(inputs, 1) != cut_files(inputs, 2)


def test_rules_in_one_buffer(inputs):
    exp = inputs.rule_lines()
    for w in (1, 2):
        hits, stats, p = run_rules(inputs.args("-K", inputs.rules, LARGE_G, w))
        assert hits == exp and int(stats["Matches"]) == len(exp) and "NOTE" not in p.stderr, w


def test_signatures_in_one_buffer(inputs):
    exp = inputs.signature_lines()
    for w in (1, 2):
        hits, stats, p = run_sequences(inputs.args("-Q", inputs.sigs, LARGE_G, w))
        got = sorted((os.path.basename(h[1]), int(h[0]), int(h[3]) - 1) for h in hits)
        assert got == exp and int(stats["Matches"]) == int(stats["Matches reported"]) == len(exp) and "NOTE" not in p.stderr, w


@pytest.mark.parametrize("w", [1, 2])
def test_rules_over_many_buffers(inputs, w):
    """buffers of 32 chunks: the lines printed are exactly the oracle's lines of the files that no border cuts, and
    the NOTE counts the others"""
    exp = inputs.rule_lines()
    cut = cut_files(inputs, w)
    hits, _, p = run_rules(inputs.args("-K", inputs.rules, SMALL_G, w))
    note = CUT.search(p.stderr)
    assert len(set(hits)) == len(hits) and set(hits) == {x for x in exp if x[0] not in cut}, sorted(set(hits) ^ set(exp))[:8]
    assert note and int(note.group(1)) == len(cut)


@pytest.mark.parametrize("w", [1, 2])
def test_signatures_over_many_buffers(inputs, w):
    """every printed line is one of the oracle's, every line that one buffer's share of a file holds whole is
    printed, and the note on stderr counts at least the candidates whose group reaches the buffer in front"""
    whole = Counter(inputs.signature_lines())            # (two matches a multiple of a chunk apart make one line twice)
    shares = shares_of(inputs, w)
    split = Counter(inputs.signature_lines(shares))
    hits, stats, p = run_sequences(inputs.args("-Q", inputs.sigs, SMALL_G, w))
    got = Counter((os.path.basename(h[1]), int(h[0]), int(h[3]) - 1) for h in hits)
    assert not got - whole, sorted(got - whole)[:8]
    missing = whole - got
    print("-w %d: %d lines of %d; of the %d that need bytes of two buffers %d are missing" % (
        w, sum(got.values()), sum(whole.values()), sum((whole - split).values()), sum(missing.values())))
    assert not split - got, sorted(split - got)[:8]                       # equality on the complement
    assert missing                                                        # (several buffers indeed)
    note = UNDECIDED.search(p.stderr)
    assert note and int(note.group(1)) >= reach_in_front(inputs, shares) > 0


def test_without_the_groups_bit_the_file_is_refused(inputs):
    """-E without -X: the first line with an alternative of more than one byte is named, and nothing is printed"""
    first = next(q for q, b in enumerate(inputs.bodies) if re.search(r"\((?:[0-9a-f]{2}){2,}[|)]", b))
    with pytest.raises(wm.BodyError) as e:
        wm.parse_body_ex(inputs.bodies[first])
    for q in range(first):
        wm.parse_body_ex(inputs.bodies[q])
    column = e.value.column + len("%d:" % (500 + first))
    hits, _, p = run_sequences(inputs.args("-Q", inputs.sigs, LARGE_G, 1, groups=False), ok=False)
    assert p.returncode != 0 and "sigs.ndb:%d: column %d:" % (first + 1, column) in p.stderr and hits == [], p.stderr[-300:]
    hits, _, p = run_rules(inputs.args("-K", inputs.rules, LARGE_G, 1, groups=False), ok=False)
    assert p.returncode != 0 and re.search(r"rules\.ldb:\d+: column \d+", p.stderr) and hits == []
