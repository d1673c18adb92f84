"""Poisoned memory for the scan paths (a test helper, not a conftest).

Real callers hand the library recycled memory: a text view whose bytes past n are more text (acm_grep -t
scans its packed chunks, whose buffer still holds an earlier round's stream), workspaces from a caching
allocator, planes that still hold another scan's records.  The helpers here build such memory on
purpose -- never smaller than the ABI asks for, only with the wrong contents:

  text_view    t[:n] followed by a tail: more of t ("continue"), the completion of the pattern prefix that
               ends t[:n] and further whole patterns ("complete"), or 0xFF bytes ("ff"), at least 4 KiB
               past round16(n)
  fill         a workspace or plane filled with a byte before a launch, or left as a denser scan left it
  check_planes count, records and trailer exact, every cell behind the trailer still the poison
  cuts         where test_gpu_poison.py cuts a row's text (test_host_poison.py checks that every one of
               them can tell a scan that reads past n from one that does not)
"""
import numpy as np

from gpu_pattern_matching_amd import DeviceArray

TAIL_KINDS = ("continue", "complete", "ff")
FILLS = ("stale", 0xFF, 0xA5)
PLANE_POISON = 0xEE
PAST_PAD = 4096          # poisoned bytes past round16(n): the ABI's readable pad and well beyond it
SMALL = 256 * 1024 + 37  # test_gpu_variants.SMALL: rows above it cut their text once


def round16(n):
    return (n + 15) & ~15


def cell(byte):
    """the int32 a plane cell holds after fill(byte)"""
    return int(np.frombuffer(bytes([byte]) * 4, dtype=np.int32)[0])


def _folded(b, fold):
    return fold(b) if fold is not None else b


_PREFIXES = {}


def _prefixes(pats, fold):
    """proper prefix (folded) -> the longest pattern that has it"""
    key = (id(pats), len(pats), fold)
    if key not in _PREFIXES:
        d = {}
        for p in sorted(set(pats), key=len):
            fp = _folded(p, fold)
            for j in range(1, len(p)):
                d[fp[:j]] = p
        _PREFIXES.clear()
        _PREFIXES[key] = (d, max(len(p) for p in pats), pats)
    return _PREFIXES[key][:2]


def completion(pats, head, fold=None):
    """bytes c such that head + c ends with a whole pattern: the rest of the pattern whose proper prefix
    is the longest suffix of head (of the longest such pattern; compared through fold for a nocase set),
    else the shortest pattern whole"""
    d, longest = _prefixes(pats, fold)
    h = _folded(bytes(head[-longest:]), fold)
    for j in range(min(len(h), longest - 1), 0, -1):
        p = d.get(h[-j:])
        if p is not None:
            return p[j:]
    return min(pats, key=len)


def tail_bytes(kind, t, n, size, pats=None, fold=None, seed=0):
    """the size bytes that follow t[:n] in a view of tail kind"""
    if kind == "continue":
        rest = np.asarray(t[n:n + size], dtype=np.uint8)
        if rest.size < size:
            rest = np.concatenate([rest, np.resize(np.asarray(t, dtype=np.uint8), size - rest.size)])
        return rest
    if kind == "ff":
        return np.full(size, 0xFF, dtype=np.uint8)
    if kind == "complete":
        rng = np.random.default_rng(seed)
        out = bytearray(completion(pats, t[max(0, n - 320):n], fold))
        while len(out) < size:
            out += pats[int(rng.integers(len(pats)))]
        return np.frombuffer(bytes(out[:size]), dtype=np.uint8)
    raise KeyError(kind)


def view_host(t, n, kind, pats=None, fold=None, seed=0, past=PAST_PAD):
    """host image of text_view: t[:n] and a tail up to round16(n) + past (a multiple of 16)"""
    size = round16(n) + past
    h = np.empty(size, dtype=np.uint8)
    h[:n] = t[:n]
    h[n:] = tail_bytes(kind, t, n, size - n, pats, fold, seed)
    return h


def text_view(t, n, tail_kind, pats=None, fold=None, seed=0):
    """(device buffer, n): t[:n] followed by a tail of tail_kind, readable (and poisoned) at least 4 KiB
    past round16(n).  pats/fold: the set's patterns and its case fold, for the "complete" tail."""
    return DeviceArray.from_numpy(view_host(t, n, tail_kind, pats, fold, seed)), n


def fill(bufs, how, stale=None):
    """poison bufs before a launch: a byte (acm_rt_memset over every byte), or "stale": stale() runs a
    denser scan that leaves its contents in them"""
    if how == "stale":
        stale()
        return
    for b in bufs:
        b.fill(how)


def check_planes(pat, off, cap, exp, poison=PLANE_POISON, what="", pat_cells=True, stream=None):
    """The planes of cap cells hold exp = (offsets, pattern ids, final state) in the scan's layout: cells
    [0, min(m + 2, cap)) exact -- count, records, trailer (at cap - 1 on overflow) -- and every cell
    behind the trailer still the poison byte.  pat_cells=False: the pattern plane holds states
    (REPORT_STATE); its records are not compared.  stream: the stream the scan was enqueued on (the
    download is ordered behind it)."""
    pos, ids, last = exp
    m = len(pos)
    p = pat.to_numpy(np.int32, cap, stream=stream)
    o = off.to_numpy(np.int32, cap, stream=stream)
    stored = min(m, cap - 2)
    t = stored + 1
    assert int(p[0]) == m and int(o[0]) == m, "%s: count cells %d/%d, expected %d" % (what, p[0], o[0], m)
    assert np.array_equal(o[1:t].astype(np.uint32), np.asarray(pos[:stored], dtype=np.uint32)), \
        "%s: offsets differ" % what
    if pat_cells:
        assert np.array_equal(p[1:t], np.asarray(ids[:stored], dtype=np.int32)), "%s: pattern ids differ" % what
    assert int(p[t]) == last and int(o[t]) == last, \
        "%s: trailer %d/%d at cell %d, expected %d" % (what, p[t], o[t], t, last)
    v = cell(poison)
    for name, plane in (("pattern", p), ("offset", o)):
        bad = np.flatnonzero(plane[t + 1:] != v)
        assert bad.size == 0, "%s: %s plane cell %d behind the trailer (cell %d) was written: %d" % (
            what, name, t + 1 + int(bad[0]), t, plane[t + 1 + int(bad[0])])


def plant(t, p, at):
    t[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)


def row_text(vs, n_row, seed, kind="planted"):
    """(text of n_row + 8 KiB bytes, match cut): a row's text from variants.text (at most SMALL + 8 KiB
    of it, repeated beyond that), the set's longest pattern planted so that it straddles the cut, 64
    bytes before n_row"""
    import variants
    base_n = min(n_row, SMALL) + 8192
    base = variants.text(vs, base_n, seed, kind if n_row <= SMALL else "random")
    t = base if n_row <= SMALL else np.resize(base, n_row + 8192)
    longest = max(vs.patterns, key=len)
    cut = n_row - 64
    at = cut - max(1, len(longest) // 2)
    plant(t, longest, at)
    return t, cut


def cuts(n_row, S, match_cut):
    """the text sizes a row is scanned at: inside the longest pattern's match; n % 16 = 0, 1, 15; one byte
    either side of a tile border (4096) and, with S, of a chain border S past it; 1..17 bytes.  Rows
    above SMALL: the match cut only."""
    if n_row > SMALL:
        return [match_cut]
    base = (n_row * 2 // 3) & ~15
    border = (n_row // 2) & ~4095
    out = [match_cut, base, base + 1, base + 15, border - 1, border + 1]
    if S:
        out += [border + S - 1, border + S + 1]
    return out + list(range(1, 18))


def row_seed(regime):
    import variants
    return 100 + variants.REGIMES[regime]["seed"]


def init_states(seed, count, num_states):
    """the carried-in state of each cut"""
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(0, num_states, size=count)]


def oracle_of(vs):
    """the oracle of a VariantSet (of its folded patterns when nocase), ids index + 1, no device library"""
    import orc
    import variants
    o = orc.Oracle()
    for i, p in enumerate(vs.patterns):
        o.add(variants.fold(p) if vs.nocase else p, i + 1)
    o.compile()
    return o
