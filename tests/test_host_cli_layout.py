"""tests/cli_layout.py on the host: the layout against hand-written cases, the expectations per mode against the helpers
of the one-buffer CLI tests for those tests' inputs, and, where grep is installed, against GNU grep over each file alone
for the inputs of test_gpu_cli_buffers.py: the model is right for those inputs whether or not the GPU machine has grep."""
import os
import subprocess

import numpy as np
import pytest

import cli_layout as lay
import normalize_model as nm
import test_gpu_cli_buffers as cb
import test_gpu_extract_cli as xc
import test_gpu_format_cli as fc
import test_gpu_normalize_cli_buffers as nb
import test_gpu_rewrite_cli as rc
import test_gpu_select_cli as sc

B, G = 4, 3
needs_grep = pytest.mark.skipif(not xc.GREP, reason="grep is not installed")


def shape(files, workers, b=B, g=G):
    """per worker, per buffer: (stream, starts, packed, cut)"""
    return [[(x.stream, x.starts, x.packed, x.cut) for x in bufs] for bufs in lay.layout(files, b, g, workers)]


def test_exact_fit_and_one_byte_more():
    fit = [("a", b"0123456789AB"), ("b", b"xy")]
    assert shape(fit, 1) == [[(b"0123456789AB", [(0, 0)], True, False), (b"xy", [(0, 1)], True, False)]]
    assert lay.cut_files(fit, B, G, 1) == []
    more = [("a", b"0123456789ABC"), ("b", b"xy")]
    assert shape(more, 1) == [[(b"0123456789AB", [(0, 0)], True, False), (b"Cxy", [(0, 0), (1, 1)], False, True)]]
    assert lay.cut_files(more, B, G, 1) == [0]
    # the second worker's second file
    both = [("w0", b"p"), ("w1", b"0123456789AB"), ("w0b", b"q"), ("w1b", b"0123456789ABC")]
    assert lay.cut_files(both, B, G, 2) == [3]
    assert [x[3] for x in shape(both, 2)[1]] == [False, False, True] and shape(both, 2)[0] == [(b"pq", [(0, 0), (1, 2)], False, False)]


def test_as_many_files_as_chunks():
    files = [("f%d" % i, bytes([65 + i]) * (1 + i % B)) for i in range(G)]
    (stream, starts, packed, cut), = shape(files, 1)[0]
    assert stream == b"ABBCCC" and starts == [(0, 0), (1, 1), (3, 2)] and not packed and not cut
    full = [("f%d" % i, bytes([65 + i]) * B) for i in range(G + 1)]
    assert shape(full, 1) == [[(b"AAAABBBBCCCC", [(0, 0), (4, 1), (8, 2)], True, False), (b"DDDD", [(0, 3)], True, False)]]


def test_empty_files_have_no_chunk():
    for at in range(3):
        files = [("a", b"01234"), ("b", b"xyz")]
        files.insert(at, ("none", b""))
        ids = [f for f, (n, _) in enumerate(files) if n != "none"]
        assert shape(files, 1) == [[(b"01234xyz", [(0, ids[0]), (5, ids[1])], False, False)]]
    assert shape([("none", b"")], 1) == [[]]
    # a short chunk at the buffer's end leaves it packed
    assert shape([("a", b"0123"), ("b", b"xyz")], 1)[0][0][2] is True


def test_more_workers_than_files():
    files = [("a", b"01234"), ("b", b"xyz")]
    assert shape(files, 3) == [[(b"01234", [(0, 0)], True, False)], [(b"xyz", [(0, 1)], True, False)], []]
    assert [s[1] for s in lay.streams(files, 3)] == [b"01234", b"xyz", b""]
    # worker w takes files w, w + workers, ...
    many = [("f%d" % i, bytes([65 + i])) for i in range(5)]
    assert [s[0] for s in lay.streams(many, 2)] == [[0, 2, 4], [1, 3]] and [s[1] for s in lay.streams(many, 2)] == [b"ACE", b"BD"]


def test_a_file_over_three_buffers():
    files = [("a", b"ab"), ("long", bytes(range(48, 48 + 26))), ("z", b"Z")]
    got = shape(files, 1)
    assert [x[0] for x in got[0]] == [b"ab" + bytes(range(48, 56)), bytes(range(56, 68)), bytes(range(68, 74)) + b"Z"]
    assert [x[1] for x in got[0]] == [[(0, 0), (2, 1)], [(0, 1)], [(0, 1), (6, 2)]]
    assert [x[2:] for x in got[0]] == [(False, False), (True, True), (False, True)]
    assert [b.base for b in lay.layout(files, B, G, 1)[0]] == [0, 10, 22]


def test_entries_are_those_of_the_select_test():
    texts = [sc.make_file(s, 300) for s in (1, 2, 3)]
    for nocase in (False, True):
        for words in (False, True):
            for t in (texts, [b"".join(texts)]):
                mine, theirs = lay.entries(t, sc.PATS, nocase, words), sc.entries(t, nocase, words)
                assert mine[0].tolist() == theirs[0].tolist() and mine[1].tolist() == theirs[1].tolist() and mine[0].size > 30


def full_paths(path, files):
    return [(os.path.join(path, name), t) for name, t in files]


def test_lines_expectations_are_those_of_the_one_buffer_tests(tmp_path):
    path, pats, files = xc.write_inputs(tmp_path)
    for _, before, after, invert in xc.CASES + fc.CASES:
        assert lay.lines_expected(full_paths(path, files), 64, 256, 1, xc.PATS, before, after, invert) == xc.expected(files, before, after, invert)
        for flags in fc.SUBSETS[1:]:
            assert lay.lines_expected(full_paths(path, files), 64, 256, 1, xc.PATS, before, after, invert, flags) == \
                fc.expected_prefixed(path, files, before, after, invert, flags)


def test_rewrite_and_select_expectations_are_those_of_the_one_buffer_tests(tmp_path):
    path, pats, files = sc.write_inputs(tmp_path, [(1, 300), (2, 290), (3, 310)])
    for flags in rc.CASES:
        kw = dict(segmented="-S" in flags, nocase="-i" in flags, words="-W" in flags)
        exp, buffers = rc.expected_files(files, 16, *kw.values())
        assert lay.rewrite_expected(files, sc.B, 16, 1, sc.PATS, rc.REPL, **kw) == (exp, 0, 1) and buffers == 1
        assert lay.select_expected(files, sc.B, 16, 1, sc.PATS, **kw) == sc.expected(files, 16, *kw.values())
    # and of their file over three buffers
    t = bytearray(sc.make_file(7, 3072))
    for cut in (1024, 2048):
        t[cut - 2:cut + 2] = b"abcd"
    files = [(str(tmp_path / "cut.txt"), bytes(t))]
    exp, dropped, buffers = sc.expected(files, 16)
    assert lay.select_expected(files, sc.B, 16, 1, sc.PATS) == (exp, dropped, buffers) and buffers == 3 and dropped >= 4
    assert lay.rewrite_expected(files, sc.B, 16, 1, sc.PATS, rc.REPL) == (rc.expected_files(files, 16)[0], dropped, 3)


def test_the_sets_lie_as_meant(tmp_path):
    for workers in (1, 2, 3):
        files, _ = cb.write_set(tmp_path / ("L%d" % workers), cb.set_L(workers), cb.LPATS)
        bufs = cb.check_L(files, workers)
        for mine in bufs:
            # in every buffer some file has a match in its first and in its last line; some file of the worker has none
            for b in mine:
                assert any(lay.entries([files[f][1].split(b"\n")[0]], cb.LPATS)[0].size and
                           lay.entries([files[f][1].rstrip(b"\n").split(b"\n")[-1]], cb.LPATS)[0].size for _, f in b.starts)
            assert any(t and not lay.entries([t], cb.LPATS)[0].size for f, t in (files[f] for b in mine for _, f in b.starts))
    for workers in (1, 2):
        files, _ = cb.write_set(tmp_path / ("R%d" % workers), cb.set_R(workers), cb.RPATS)
        for mine in cb.check_R(files, workers):
            assert mine[0].stream.endswith(b" ab") and mine[1].stream.startswith(b"cd")          # the byte behind is a word byte
            assert mine[1].stream.endswith(b"ab") and mine[2].stream.startswith(b"cd")
            assert mine[2].stream.endswith(b" ab") and mine[3].stream.startswith(b" ")           # the byte behind is a space
        # the entries that begin in the buffer in front are counted, and the cut changes what is selected
        exp, dropped, buffers = lay.rewrite_expected(files, cb.B, cb.G, workers, cb.RPATS, rc.REPL)
        assert dropped >= 2 * workers and buffers == 4 * workers
        assert exp != lay.rewrite_expected(files, cb.B, 1 << 20, workers, cb.RPATS, rc.REPL)[0]
    # the single-worker order of set L holds the same files and cuts none
    files, _ = cb.write_set(tmp_path / "S", cb.set_L(3, single=True), cb.LPATS)
    assert lay.cut_files(files, cb.B, cb.G, 1) == [] and lay.no_match_spans_files(files, 1, cb.LPATS)
    assert sorted(n for n, _ in cb.set_L(3, single=True)) == sorted(n for n, _ in cb.set_L(3))


def test_the_deferred_byte_decides(tmp_path):
    """the expectations of -W differ from those of a word pass that does not look behind a buffer, in set L and in set R,
    and exactly where the test says"""
    for workers in (1, 2):
        files, _ = cb.write_set(tmp_path / ("L%d" % workers), cb.set_L(workers), cb.LPATS)
        exp = lay.lines_expected(files, cb.B, cb.G, workers, cb.LPATS, 1, 1, False, words=True)
        blind = lay.lines_expected(files, cb.B, cb.G, workers, cb.LPATS, 1, 1, False, words=True, blind=True)
        assert not exp["w0_b10_open.txt"].endswith(b"chaff pin\n") and blind["w0_b10_open.txt"].endswith(b"chaff pin\n")
        assert exp["w0_l_open.txt"].endswith(b"straw hay\n")
        files, _ = cb.write_set(tmp_path / ("R%d" % workers), cb.set_R(workers), cb.RPATS)
        exp = lay.rewrite_expected(files, cb.B, cb.G, workers, cb.RPATS, rc.REPL, words=True)[0]
        blind = lay.rewrite_expected(files, cb.B, cb.G, workers, cb.RPATS, rc.REPL, words=True, blind=True)[0]
        assert b" abcd" in exp["w0_B.txt"] and exp["w0_B.txt"] != blind["w0_B.txt"]
        assert exp["w0_C.txt"].endswith(b" <AB>")


@needs_grep
@pytest.mark.parametrize("workers", [1, 2, 3])
def test_set_L_against_grep(tmp_path, workers):
    files, pats = cb.write_set(tmp_path, cb.set_L(workers), cb.LPATS)
    for before, after, invert in ((1, 2, False), (0, 0, True), (1, 1, False)):
        exp = lay.lines_expected(files, cb.B, cb.G, workers, cb.LPATS, before, after, invert)
        for path, _ in files:
            assert exp[os.path.basename(path)] == xc.grep_file(path, pats, before, after, invert), path
    for n, invert, flags in ((2, False, ["-H", "-N", "-b"]), (0, True, ["-N", "-b"]), (1, False, ["-H", "-N", "-b"])):
        exp = lay.lines_expected(files, cb.B, cb.G, workers, cb.LPATS, n, n, invert, flags)
        for path, _ in files:
            assert exp[os.path.basename(path)] == fc.grep_file(path, pats, n, n, invert, flags), path
    # the files of the exact fits
    for k, open_end in enumerate((False, True)):
        named = [("fit.txt", cb.sized(11, cb.G * cb.B, open_end, first=b"hay first", last=b"the last pin")),
                 ("next.txt", cb.sized(12, 90, False, first=b"pin"))]
        fit, pats = cb.write_set(tmp_path / ("fit%d" % k), named, cb.LPATS)
        exp = lay.lines_expected(fit, cb.B, cb.G, 1, cb.LPATS, 1, 1, False)
        for path, _ in fit:
            assert exp[os.path.basename(path)] == xc.grep_file(path, pats, 1, 1, False), path


@needs_grep
def test_set_R_against_grep(tmp_path):
    """grep -o -b prints the leftmost-longest non-overlapping matches of a file: the select expectation of a run that
    holds every file whole (one buffer, -S)"""
    files, pats = cb.write_set(tmp_path, cb.set_R(2), cb.RPATS)
    got = {}
    for b, ep, eo, info in lay._selected(files, cb.B, 1 << 20, 1, cb.RPATS, True, False, False, False):
        assert info[1] == 0
        at = [s for s, _ in b.starts]
        for p, o in zip(ep.tolist(), eo.tolist()):
            k = max(i for i, s in enumerate(at) if s <= o)
            got.setdefault(files[b.starts[k][1]][0], []).append(b"%d:%s" % (o - len(cb.RPATS[p]) + 1 - at[k], cb.RPATS[p]))
    for path, t in files:
        r = subprocess.run([xc.GREP, "-a", "-o", "-b", "-F", "-f", pats, path], capture_output=True, env=dict(os.environ, LC_ALL="C"), timeout=60)
        assert r.stdout.splitlines() == got.get(path, []), path
        assert bool(t) == (len(got.get(path, [])) > 20)


# ------------------------------------------------------------------ normalized_hits (-S -z)


def whole_file_hits(named, pats, flags, blanks=None, nocase=False, words=False):
    """every file normalised whole: (pattern, file, offset of the last byte)"""
    out = set()
    for f, (_, t) in enumerate(named):
        x = nm.normalize(t, flags, blanks)
        cells, offs = lay.entries([x.out], pats, nocase, words)
        out |= {(p, f, int(x.last[e])) for p, e in zip(cells.tolist(), offs.tolist())}
    return out


def stream_cut_hits(named, pats, b, g, workers, flags):
    """the brute force over the worker's stream: it is cut where a buffer or a file begins, every stream[a:b] is
    normalised alone, the pieces of a file are joined"""
    out = set()
    for (mine, stream, bounds), bufs in zip(lay.streams(named, workers), lay.layout(named, b, g, workers)):
        cuts = sorted({x.base for x in bufs} | set(bounds.tolist()))
        for k, f in enumerate(mine):
            edges = [c for c in cuts if bounds[k] <= c <= bounds[k + 1]]
            norm = [(a, nm.normalize(stream[a:z], flags)) for a, z in zip(edges, edges[1:])]
            text, at = b"".join(x.out for _, x in norm), np.cumsum([0] + [x.m for _, x in norm])
            for p, e in zip(*(v.tolist() for v in lay.entries([text], pats))):
                j = int(np.searchsorted(at, e, side="right")) - 1
                out.add((p, f, norm[j][0] + int(norm[j][1].last[e - at[j]]) - int(bounds[k])))
    return out


def flat(hits):
    return {(h.pattern, h.file, h.offset) for h in hits}


def test_normalized_hits_of_whole_files():
    """where no buffer cuts a file the hits are those of every file normalised whole, whatever the layout"""
    for workers in (1, 2, 3):
        named = nb.whole_set(workers)
        for spec in ("url,ws", "strip,url", "nul", "url"):
            flags, blanks = nb.SPECS[spec]
            for kw in (dict(), dict(nocase=True), dict(words=True)):
                want = whole_file_hits(named, nb.EVERY, flags, blanks, **kw)
                for b, g in ((nb.B, nb.G_WHOLE), (4096, 16), (64, 1 << 12)):
                    assert not lay.cut_files(named, b, g, workers)
                    got = lay.normalized_hits(named, nb.EVERY, b, g, workers, flags, blanks, **kw)
                    assert flat(got) == want and len(got) == len(want) > 10 and not any(h.spans for h in got)
    # the slot is the chunk of the buffer that holds the byte
    named = [("a", b"x" * 70 + b"a href"), ("b", b"a%20href")]
    assert lay.normalized_hits(named, [b"a href"], 64, 16, 1, nm.PERCENT) == [lay.Hit(0, 0, 75, 1, False), lay.Hit(0, 1, 7, 2, False)]


def test_normalized_hits_of_cut_files():
    for workers in (1, 2):
        named, planted = nb.cut_set(workers)
        for flags in (nm.PERCENT | nm.SQUEEZE, nm.PERCENT | nm.STRIP, nm.SQUEEZE):
            for b, g in ((nb.B, nb.G_CUT), (16, 16), (1024, 1)):
                got = lay.normalized_hits(named, nb.EVERY, b, g, workers, flags)
                assert flat(got) == stream_cut_hits(named, nb.EVERY, b, g, workers, flags) and len(got) > 1000
        assert flat(lay.normalized_hits(named, nb.ONE, nb.B, nb.G_CUT, workers, 3)) != whole_file_hits(named, nb.ONE, 3)
    # by hand: the triple and the run that a cut divides are not joined, the match that it divides is found
    named = [("f", b".....a%2" + b"0href.a " + b" href.a " + b"href....")]
    assert [(h.offset, h.spans) for h in lay.normalized_hits(named, [b"a href"], 8, 1, 1, 3)] == [(27, True)]
    assert sorted(o for _, _, o in whole_file_hits(named, [b"a href"], 3)) == [12, 20, 27]


def test_normalized_hits_of_lines():
    named = [("f", b"a\nhref a \n href%0ab\n\na b"), ("g", b"a href\r\na%20b")]
    one = lay.normalized_hits(named, [b"a href", b"a b"], 64, 16, 1, 3, lines=True)
    assert [(h.pattern, h.file, h.offset) for h in one] == [(0, 1, 5), (1, 0, 23), (1, 1, 12)]
    assert (0, 0, 5) in whole_file_hits(named, [b"a href", b"a b"], 3)
    # a line that a buffer cuts goes on
    assert [h[:3] for h in lay.normalized_hits([("f", b"xxxxxxa href\n")], [b"a href"], 8, 1, 1, 3, lines=True)] == [(0, 0, 11)]


def test_the_normalized_sets_lie_as_meant():
    """the conditions test_gpu_normalize_cli_buffers.py states about its inputs, without a device"""
    for workers in (1, 2, 3):
        nb.check_whole(nb.whole_set(workers), workers)
        nb.whole_expected(workers, "url,ws", ["-v"])
        nb.whole_expected(workers, "strip,url", ["-v", "-i"])
        nb.whole_expected(workers, "nul", ["-v", "-c", "-A"])
    nb.check_whole(nb.whole_set(2, True), 2, True)
    for workers in (1, 2):
        for every in (False, True):
            nb.word_expected(workers, every)                               # word borders that exist on one side only
            nb.cut_expected(workers, every)                                # hits across cuts, and others than whole files give
        nb.case_expected(workers)                                          # exact dropped, folding kept
        nb.line_expected(workers, "url,ws", ["-v"])
        nb.line_expected(workers, "strip,url", ["-v", "-A"])
