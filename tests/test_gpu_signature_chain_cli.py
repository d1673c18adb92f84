"""acm_grep -K -E -S and -Q -E -S over several buffers: the generated database of test_gpu_signature_chain.py
(signature_oracle.make) and 300 short texts of its corpus written as files, about 45 KiB.  What must be printed
comes from tests/signature_oracle.py alone.  A rule or signature file has one case flag for all its lines and the
command line sets no windows, so the oracle runs the database without its windows, and with every body or no body
ignoring case (-i)."""
import os
import re

import pytest

import signature_oracle as so
from test_gpu_rules_cli import run as run_rules
from test_gpu_sequences_cli import run as run_sequences
from test_gpu_signature_chain import SEED

pytestmark = pytest.mark.gpu

B = 64                        # -B: a file begins a chunk of its own
SMALL_G, LARGE_G = 32, 1024   # buffers of 2 KiB, and of 64 KiB: the whole input
CUT = re.compile(r"^NOTE: (\d+) texts are cut by a buffer border", re.M)


class Inputs:
    def __init__(self, tmp):
        g = so.make(SEED, rules=70)
        self.lines = g.lines
        self.texts, self.chunks = so.small_slice(g.texts, chunk=B)
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
        self.corpus = so.Corpus(self.texts)

    def expected(self, nocase):
        """(rule lines, signature lines) as the run helpers parse them"""
        db = so.Database(self.lines, [nocase] * len(self.bodies))
        found = so.sequences(db, self.corpus)
        c = self.corpus
        rules = sorted((self.names[t], 1000 + r, 0) for r, t, _ in so.rules(db, c, found))
        # a -Q line: the match's end relative to the chunk that holds the end of its last part's anchor
        sigs = sorted((self.names[int(c.text_of[a])], 500 + int(q), int((a - c.t0[a]) % B + e - a))
                      for e, a, q in zip(*found))
        return rules, sigs

    def args(self, flag, file, G, w):
        return ["-f", self.path, flag, file, "-E", "-S", "-B", str(B), "-D", "0", "-G", str(G), "-L", "64", "-w", str(w),
                "-R", "128", "-v"]


@pytest.fixture(scope="module")
def inputs(gpu, tmp_path_factory):
    return Inputs(tmp_path_factory.mktemp("chain"))


def test_rules_in_one_buffer(inputs):
    exp, _ = inputs.expected(False)
    assert len(exp) > 50 and len({i for _, i, _ in exp}) > 25 and len({n for n, _, _ in exp}) > 50
    assert inputs.chunks * B <= LARGE_G * B and 40 * 1024 <= inputs.corpus.N <= 50 * 1024
    hits, stats, p = run_rules(inputs.args("-K", inputs.rules, LARGE_G, 1))
    assert hits == exp and int(stats["Matches"]) == len(exp) and "NOTE" not in p.stderr
    expi, _ = inputs.expected(True)
    assert set(expi) != set(exp)
    hits, _, p = run_rules(inputs.args("-K", inputs.rules, LARGE_G, 1) + ["-i"])
    assert hits == expi and "NOTE" not in p.stderr


def cut_files(inputs, w, G=SMALL_G):
    """the files a buffer border cuts, from acm_grep's own description of how it reads: worker i takes files i,
    i + w, ... and lays them chunk by chunk into buffers of G chunks; a file whose chunks lie in two buffers is cut
    (one that ends with its buffer is whole; an empty file has no chunk)"""
    cut = set()
    for i in range(w):
        at = 0
        for k in range(i, len(inputs.texts), w):
            n = -(-len(inputs.texts[k]) // B)
            if n and at // G != (at + n - 1) // G:
                cut.add(inputs.names[k])
            at += n
    return cut


def many_buffers(inputs, w):
    """(printed lines, the NOTE's count) with buffers of 2 KiB; every printed line is one of the oracle's"""
    exp, _ = inputs.expected(False)
    hits, _, p = run_rules(inputs.args("-K", inputs.rules, SMALL_G, w))
    cut = CUT.search(p.stderr)
    n = int(cut.group(1)) if cut else 0
    assert set(hits) <= set(exp) and len(set(hits)) == len(hits), w
    return set(hits), n


@pytest.fixture(scope="module")
def small_runs(inputs):
    return {w: many_buffers(inputs, w) for w in (1, 2)}


@pytest.mark.parametrize("w", [1, 2])
def test_rules_over_many_buffers(inputs, small_runs, w):
    """Buffers of 32 chunks.  A buffer border cuts at most one file (the one that goes on in the next buffer), and its
    rules are not evaluated.  The files take inputs.chunks <= 28 * 32 chunks when each begins a chunk of its own, so
    one worker fills at most 28 buffers and two workers together at most 29: at most 29 cut files, under a tenth
    of the 300.  No file is larger than a buffer.  Which files are cut follows from their sizes and the deal
    (cut_files): the lines printed are exactly the oracle's lines of the other files."""
    assert inputs.chunks <= 28 * SMALL_G and max(len(t) for t in inputs.texts) < SMALL_G * B and len(inputs.texts) == 300
    exp, _ = inputs.expected(False)
    hits, n = small_runs[w]
    missing = {name for name, _, _ in set(exp) - hits}
    cut = cut_files(inputs, w)
    print("-w %d: %d lines of %d, %d files short of a line, NOTE %d, %d files cut by their sizes" % (
        w, len(hits), len(exp), len(missing), n, len(cut)))
    assert len(missing) <= n <= len(inputs.texts) // 10, (w, len(missing), n)
    assert n >= 10                                                            # (several buffers indeed)
    assert n == len(cut) and hits == {x for x in exp if x[0] not in cut}, (sorted(missing), sorted(cut))
    assert missing and missing <= cut                                        # a cut file with a line of the oracle's is among them


def test_one_and_two_workers_print_the_same(inputs, small_runs):
    """Worker i reads files i, i + w, ...: one and two workers cut different files, and a cut file's rules are not
    evaluated.  The lines of the files that neither deal cuts are the same set, and with buffers that cut nothing
    the whole outputs are."""
    either = cut_files(inputs, 1) | cut_files(inputs, 2)
    assert cut_files(inputs, 1) != cut_files(inputs, 2)
    one, two = ({x for x in small_runs[w][0] if x[0] not in either} for w in (1, 2))
    assert one == two and len(one) > 40
    exp, _ = inputs.expected(False)
    hits, _, p = run_rules(inputs.args("-K", inputs.rules, LARGE_G, 2))
    assert hits == exp and "NOTE" not in p.stderr


def test_signatures_in_one_buffer(inputs):
    _, exp = inputs.expected(False)
    assert len(exp) > 300 and len({i for _, i, _ in exp}) > 120 and max(r for _, _, r in exp) >= B
    hits, stats, p = run_sequences(inputs.args("-Q", inputs.sigs, LARGE_G, 1))
    got = sorted((os.path.basename(h[1]), int(h[0]), int(h[3]) - 1) for h in hits)
    assert got == exp and int(stats["Matches"]) == int(stats["Matches reported"]) == len(exp) and "NOTE" not in p.stderr
