"""numpy model of the line passes (acm_line_index_async, acm_line_number_async, acm_line_select_async)
and of chaining pieces through d_info.  Written from the rules in include/acmatch.h, not from the
kernels: the GPU tests compare the library with it cell for cell, test_host_lines.py checks it against a
brute force (a test helper, not a conftest)."""
import numpy as np

SENTINEL = np.int32(0x7FFFFFFF)


def delim_byte(delimiter):
    return delimiter[0] if isinstance(delimiter, (bytes, bytearray)) else int(delimiter)


def index(text, origin=0, delimiter=0x0A, prev_byte=-1, prev_info=None, capacity=None):
    """(line_start int32[capacity], info int32[8], starts int64[m]) of one piece.  prev_info: the info of
    the piece in front (prev_byte is then ignored)."""
    t = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) \
        else np.ascontiguousarray(text, dtype=np.uint8)
    n = int(t.size)
    d = delim_byte(delimiter)
    if prev_info is not None:
        begins = bool(prev_info[3])
        front = (int(np.uint32(prev_info[4])) | int(np.uint32(prev_info[5])) << 32) + int(np.uint32(prev_info[1]))
    else:
        begins = prev_byte == -1 or prev_byte == d
        front = 0
    hits = np.flatnonzero(t == d).astype(np.int64)
    starts = origin + hits[hits + 1 < n] + 1
    org = 1 if (n > 0 and begins) else 0
    if org:
        starts = np.concatenate([np.array([origin], dtype=np.int64), starts])
    m = int(starts.size)
    info = np.zeros(8, dtype=np.int32)
    info[0] = m
    info[1] = hits.size
    info[2] = org
    info[3] = int(t[n - 1] == d) if n else int(begins)
    info[4] = np.uint32(front & 0xFFFFFFFF).astype(np.int32)
    info[5] = np.uint32(front >> 32).astype(np.int32)
    cap = m if capacity is None else capacity
    line_start = np.full(cap, SENTINEL, dtype=np.int32)
    k = min(m, cap)
    line_start[:k] = starts[:k]
    return line_start, info, starts


def chain(pieces, origin=0, delimiter=0x0A, prev_byte=-1, capacity=None):
    """index() over consecutive pieces, each handed the info of the one in front: a list of its results"""
    out, info, o = [], None, origin
    for p in pieces:
        r = index(p, o, delimiter, prev_byte, info, capacity)
        out.append(r)
        info = r[1]
        o += len(p)
    return out


def stream_delims(info):
    """delimiters of the stream in front of a piece's origin"""
    return int(np.uint32(info[4])) | int(np.uint32(info[5])) << 32


def number(starts, info, offsets):
    """delimiters in [origin, offset) of each offset: k + 1 - info[2], k the last start <= offset"""
    st = np.asarray(starts, dtype=np.int64)
    return (np.searchsorted(st, np.asarray(offsets, dtype=np.int64), side="right") - int(info[2])).astype(np.int32)


def lines_of(starts, info, origin, end):
    """(rel, begin, next) int64 arrays of the lines of a piece, the lead first when there is one"""
    st = np.asarray(starts, dtype=np.int64)
    lead = end > origin and int(info[2]) == 0
    begin = np.concatenate([np.array([origin], dtype=np.int64), st]) if lead else st
    nxt = np.concatenate([begin[1:], np.array([end], dtype=np.int64)]) if begin.size else begin
    return np.arange(begin.size, dtype=np.int64), begin, nxt


def select(starts, info, origin, end, offsets, invert=False):
    """(rel, begin, next) of the lines that hold an offset of offsets (invert: that hold none)"""
    rel, begin, nxt = lines_of(starts, info, origin, end)
    offs = np.asarray(offsets, dtype=np.int64)
    offs = offs[(offs >= origin) & (offs < end)]
    hit = np.zeros(begin.size, dtype=bool)
    if begin.size and offs.size:
        j = np.searchsorted(begin, offs, side="right") - 1
        hit[j[j >= 0]] = True
    keep = ~hit if invert else hit
    return rel[keep], begin[keep], nxt[keep]


def planes(entries, cap, poison):
    """the three planes of cap cells a select call must leave: [0] = count, the entries that fit, a 0
    trailer at min(count + 1, cap - 1), the poison cell value everywhere else"""
    out = []
    m = len(entries[0])
    stored = min(m, cap - 2)
    for e in entries:
        p = np.full(cap, poison, dtype=np.int32)
        p[0] = m
        p[1:1 + stored] = np.asarray(e[:stored], dtype=np.int64).astype(np.int32)
        p[min(m + 1, cap - 1)] = 0
        out.append(p)
    return out
