"""The layout of an acm_grep run in binary mode, computed on the host (test infrastructure only, not a conftest): which
bytes every buffer of every worker holds, where the files begin in it, whether its chunks lie back to back and whether
it goes on with the file of the buffer in front.  Written from the rules of the feeder, not from its code:

  * worker w takes files w, w + workers, ... of the list, in the order given (-f a,b,c: the test's order, not readdir's);
  * a file of n bytes is ceil(n / B) chunks, the last one short; a file of no bytes has no chunk;
  * a buffer closes at G chunks; the worker's last buffer may be shorter;
  * a start at a buffer's chunk 0 (also when it goes on with a file) and at every chunk of another file than the chunk
    before it; the buffer is packed while no short chunk has another chunk behind it.

layout() needs nothing of the project.  On top of it one function per file-writing mode gives {file name: expected
bytes}: the models (extract_model, format_model, select_model, rewrite_model) over the records bytes.find gives.
normalized_hits() gives the -v lines of a run with -S -z: every piece of a file that a buffer holds normalised alone by
normalize_model, the pieces of a text joined, bytes.find over that."""
import collections
import os

import numpy as np

WORD = frozenset(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_")

Buffer = collections.namedtuple("Buffer", "worker index base stream chunks starts packed cut")
Buffer.__doc__ = """worker, index: the index-th buffer of that worker; base: where it begins in the worker's stream; stream:
its bytes; chunks: (file, bytes) of every chunk, file an index into the list given; starts: (stream offset, file) of
every file start; packed; cut: chunk 0 goes on with the file the buffer in front ended in"""


def layout(files, B, G, workers):
    """one list of Buffers per worker (a worker without a byte has none)"""
    out = []
    for w in range(workers):
        chunks = [(f, files[f][1][k:k + B]) for f in range(w, len(files), workers) for k in range(0, len(files[f][1]), B)]
        bufs, base = [], 0
        for i in range(0, len(chunks), G):
            mine = chunks[i:i + G]
            starts, at = [], 0
            for k, (f, data) in enumerate(mine):
                if k == 0 or f != mine[k - 1][0]:
                    starts.append((at, f))
                at += len(data)
            bufs.append(Buffer(w, len(bufs), base, b"".join(d for _, d in mine), [(f, len(d)) for f, d in mine], starts,
                               all(len(d) == B for _, d in mine[:-1]), i > 0 and chunks[i - 1][0] == mine[0][0]))
            base += at
        out.append(bufs)
    return out


def cut_files(files, B, G, workers):
    """the files some buffer goes on with: what -C refuses"""
    return sorted({b.chunks[0][0] for bufs in layout(files, B, G, workers) for b in bufs if b.cut})


def streams(files, workers):
    """per worker: (the indices of its files, its stream, where each of its files begins in it and the stream's end)"""
    out = []
    for w in range(workers):
        mine = list(range(w, len(files), workers))
        out.append((mine, b"".join(files[f][1] for f in mine), np.cumsum([0] + [len(files[f][1]) for f in mine]).astype(np.int64)))
    return out


def entries(texts, pats, nocase=False, words=False):
    """(pattern, end in the stream) planes of every occurrence of every pattern, each text alone, ordered by end then
    pattern; words: only where the bytes around it are no word bytes or its text's border"""
    out, base = [], 0
    for t in texts:
        hay = t.upper() if nocase else t
        for i, p in enumerate(pats):
            needle = p.upper() if nocase else p
            k = hay.find(needle)
            while k >= 0:
                e = k + len(p) - 1
                if not words or ((k == 0 or t[k - 1] not in WORD) and (e + 1 == len(t) or t[e + 1] not in WORD)):
                    out.append((base + e, i))
                k = hay.find(needle, k + 1)
        base += len(t)
    out.sort()
    return np.array([c for _, c in out], dtype=np.int64), np.array([o for o, _ in out], dtype=np.int64)


def records(files, B, G, workers, pats, segmented=False, nocase=False, words=False, blind=False):
    """per worker (cells, offsets in its stream) of the records the passes in front of -o, -r and -C see.  blind: every
    buffer's stream taken for a whole text -- what -W gives when the byte behind a buffer is not looked at"""
    out = []
    for (mine, stream, bounds), bufs in zip(streams(files, workers), layout(files, B, G, workers)):
        if blind:
            cells, offs = entries([b.stream for b in bufs], pats, nocase, words)
        else:
            cells, offs = entries([files[f][1] for f in mine] if segmented else [stream], pats, nocase, words)
        out.append((cells, offs))
    return out


def no_match_spans_files(files, workers, pats, nocase=False):
    """every occurrence in a worker's stream lies in one file: a file alone then has the records of its stream"""
    for mine, stream, _ in streams(files, workers):
        if entries([stream], pats, nocase)[1].tolist() != entries([files[f][1] for f in mine], pats, nocase)[1].tolist():
            return False
    return True


def lines_expected(files, B, G, workers, pats, before, after, invert, flags=(), segmented=False, nocase=False, words=False,
                   blind=False):
    """-C before,after -T [-V] [-H -N -b]: {file name: its lines}, the extract model (with a prefix flag: the format model)
    over every file alone, the records those of its worker's stream.  No file may be cut and no match may span two files."""
    import extract_model as xm
    import format_model as fm
    assert not cut_files(files, B, G, workers), "a file is cut across two buffers: -C refuses the run"
    assert no_match_spans_files(files, workers, pats, nocase), "a match spans two files: the files of this test must not make one"
    out = {}
    for (mine, stream, bounds), (cells, offs) in zip(streams(files, workers),
                                                     records(files, B, G, workers, pats, segmented, nocase, words, blind)):
        ends = np.unique(offs)
        for k, f in enumerate(mine):
            path, t = files[f]
            own = (ends[(ends >= bounds[k]) & (ends < bounds[k + 1])] - bounds[k]).tolist()
            if flags:
                out[os.path.basename(path)] = fm.grep_like(t, own, before, after, invert, names=[path.encode()], with_name="-H" in flags,
                                                           line_number="-N" in flags, byte_offset="-b" in flags)[0]
            else:
                out[os.path.basename(path)] = xm.grep_like(t, own, before, after, invert)[0]
    return out


def _selected(files, B, G, workers, pats, segmented, nocase, words, blind):
    """per buffer of every worker: (the buffer, the select model's patterns, offsets in the buffer and info)"""
    import select_model as sel
    model = sel.SelectModel([len(p) for p in pats])
    for bufs, (cells, offs) in zip(layout(files, B, G, workers), records(files, B, G, workers, pats, segmented, nocase, words, blind)):
        for b in bufs:
            inside = (offs >= b.base) & (offs < b.base + len(b.stream))
            ep, eo, _, info = model.run(cells[inside], offs[inside] - b.base, 0)
            yield b, ep, eo, info


def select_expected(files, B, G, workers, pats, segmented=False, nocase=False, words=False, blind=False):
    """-o: (sorted (file name, pattern, position in its file modulo B) of every selected match, the entries that began in
    front of a buffer summed over the workers, the buffers of all workers)"""
    out, dropped, buffers = [], 0, 0
    for b, ep, eo, info in _selected(files, B, G, workers, pats, segmented, nocase, words, blind):
        dropped += info[1]
        buffers += 1
        at = np.array([s for s, _ in b.starts], dtype=np.int64)
        for p, o in zip(ep.tolist(), eo.tolist()):
            k = int(np.searchsorted(at, o, side="right")) - 1
            # a file's chunks begin at multiples of B in it: the position in the chunk is the one in the file modulo B
            in_chunk, c = o - int(at[k]), [n for f, n in b.chunks if f == b.starts[k][1]]
            while in_chunk >= c[0]:
                in_chunk -= c.pop(0)
            out.append((os.path.basename(files[b.starts[k][1]][0]), pats[p].decode(), in_chunk))
    return sorted(out), dropped, buffers


def rewrite_expected(files, B, G, workers, pats, repl, segmented=False, nocase=False, words=False, blind=False):
    """-r -O: ({file name: rewritten bytes}, the entries that began in front of a buffer summed over the workers, the
    buffers of all workers): every buffer selected and rewritten alone, its output cut at the file starts and appended
    per file.  repl: per pattern None, bytes or ("fill", byte)"""
    import rewrite_model as rw
    model = rw.RewriteModel([len(p) for p in pats],
                            [None if r is None else (bytes([r[1]]), True) if isinstance(r, tuple) else (r, False) for r in repl])
    out, dropped, buffers = {os.path.basename(path): b"" for path, _ in files}, 0, 0
    for b, ep, eo, info in _selected(files, B, G, workers, pats, segmented, nocase, words, blind):
        dropped += info[1]
        buffers += 1
        data, _, _, seg = model.run(b.stream, ep, eo, seg_start=[s for s, _ in b.starts])
        for k, (_, f) in enumerate(b.starts):
            out[os.path.basename(files[f][0])] += data[seg[k]:seg[k + 1] if k + 1 < len(seg) else len(data)]
    return out, dropped, buffers


Hit = collections.namedtuple("Hit", "pattern file offset slot spans")
Hit.__doc__ = """pattern: its index; file: an index into the list given; offset: of the match's last byte in its file (the last
byte of the unit that emitted the match's last byte); slot: the chunk of its buffer that byte lies in; spans: the
match began in an earlier piece than it ends in"""


def pieces(files, B, G, workers, lines=False):
    """per worker the pieces a run with -S -z normalises each alone, in stream order: (file, offset in the file, bytes,
    it begins a text, the index of its buffer, its offset in that buffer's stream).  A buffer's stream is cut at its
    starts; with lines also behind every newline.  A piece begins a text when it is of another file than the piece in
    front of it, or with lines when that piece ended a line; else it goes on with the text in front: a file that a
    buffer cuts, a line that one cuts.  (With lines the layout is still the one of binary mode: it is the layout of a
    run with -t only where it cuts no line.)"""
    out = []
    for bufs in layout(files, B, G, workers):
        mine, done, last_file, line_open = [], collections.Counter(), None, False
        for b in bufs:
            at = [s for s, _ in b.starts] + [len(b.stream)]
            for k, (s, f) in enumerate(b.starts):
                raw = b.stream[s:at[k + 1]]
                parts = raw.split(b"\n") if lines else [raw]         # (only \n ends a line: not bytes.splitlines)
                for p in [p + b"\n" for p in parts[:-1]] + parts[-1:]:
                    if not p:
                        continue
                    mine.append((f, done[f], p, f != last_file or (lines and not line_open), b.index, s))
                    done[f] += len(p)
                    s += len(p)
                    last_file, line_open = f, not p.endswith(b"\n")
        out.append(mine)
    return out


def normalized_hits(files, pats, B, G, workers, flags, blanks=None, nocase=False, words=False, lines=False):
    """-S -z: the sorted Hits of a run.  Every piece (pieces()) is normalised alone by the model; a text for matching is
    the concatenation of the normalised pieces of one file (with lines: of one line), since the scan goes on from one
    piece into the next in the state the piece in front left; every pattern is found in it with bytes.find (entries();
    nocase: one flag, or one per pattern); a hit lies where the model's last[] of the piece that holds its last byte
    says.  Without -A a run reports one pattern per end: give patterns none of which is a suffix of another."""
    import normalize_model as nm
    fold = list(nocase) if isinstance(nocase, (list, tuple)) else [bool(nocase)] * len(pats)
    hits = []
    for w, mine in enumerate(pieces(files, B, G, workers, lines)):
        bufs = layout(files, B, G, workers)[w]
        texts = []
        for p in mine:
            if p[3]:
                texts.append([])
            texts[-1].append((p, nm.normalize(p[2], flags, blanks)))
        for text in texts:
            out = b"".join(x.out for _, x in text)
            ends = np.cumsum([x.m for _, x in text])                   # the normalised text in front of the end of every piece
            for i, pat in enumerate(pats):
                for e in entries([out], [pat], fold[i], words)[1].tolist():
                    j = int(np.searchsorted(ends, e, side="right"))
                    js = int(np.searchsorted(ends, e - len(pat) + 1, side="right"))
                    (f, at, raw, _, index, s), x = text[j]
                    last = int(x.last[e - (int(ends[j - 1]) if j else 0)])
                    sizes = np.cumsum([n for _, n in bufs[index].chunks])
                    hits.append(Hit(i, f, at + last, int(np.searchsorted(sizes, s + last, side="right")), js < j))
    return sorted(hits)


def numbered_expected(files, workers, pats):
    """-n -v: Counter of (file path, pattern, 1-based line of the match's last byte in its file) over every worker's
    stream, as test_gpu_lines_cli.expected counts them (the pattern by its bytes: these patterns have no ids of their own)"""
    out = collections.Counter()
    for mine, stream, bounds in streams(files, workers):
        cells, offs = entries([stream], pats)
        for p, x in zip(cells.tolist(), offs.tolist()):
            k = int(np.searchsorted(bounds, x, side="right")) - 1
            path, t = files[mine[k]]
            out[(path, pats[p].decode(), 1 + t[:x - int(bounds[k])].count(b"\n"))] += 1
    return out
