"""numpy / plain-Python model of the context pass (acm_line_context_async) and of the extract pass
(acm_extract_async).  Written from the rules in include/acmatch.h, not from the kernels: the GPU tests compare
the library with it cell for cell and byte for byte, test_host_extract.py checks it against a brute force and
against GNU grep (a test helper, not a conftest).  It builds on line_model.py."""
import numpy as np

import line_model as lm

INT32_MAX = 0x7FFFFFFF


def _sat32(v):
    return max(-(1 << 31), min(int(v), INT32_MAX))


def context(starts, info, origin, end, offsets, invert=False, before=0, after=0, seg_start=()):
    """(rel, begin, next, lines) int64 arrays of the groups, and ctx_info int32[4]"""
    rel, begin, nxt = lm.lines_of(starts, info, origin, end)
    n_lines = int(begin.size)
    offs = np.asarray(offsets, dtype=np.int64)
    offs = offs[(offs >= origin) & (offs < end)]
    hit = np.zeros(n_lines, dtype=bool)
    if n_lines and offs.size:
        j = np.searchsorted(begin, offs, side="right") - 1
        hit[j[j >= 0]] = True
    sel = ~hit if invert else hit
    seg = np.asarray(seg_start, dtype=np.int64)
    tid = np.searchsorted(seg, begin, side="right") if seg.size else np.zeros(n_lines, dtype=np.int64)
    # the lines of each line's text (text ids ascend with the lines), the window clamped to them
    lo = np.searchsorted(tid, tid, side="left")
    hi = np.searchsorted(tid, tid, side="right")
    j = np.arange(n_lines, dtype=np.int64)
    a = np.maximum(lo, j - int(after))
    b = np.minimum(hi - 1, j + int(before))
    csum = np.concatenate([[0], np.cumsum(sel)]).astype(np.int64)
    kept = (csum[b + 1] - csum[a]) > 0 if n_lines else np.zeros(0, dtype=bool)
    joined = np.zeros(n_lines, dtype=bool)       # line j continues the group of line j - 1
    if n_lines > 1:
        joined[1:] = kept[1:] & kept[:-1] & (tid[1:] == tid[:-1])
    heads = np.flatnonzero(kept & ~joined)
    tails = np.flatnonzero(kept & ~np.concatenate([joined[1:], [False]])) if n_lines else heads
    ctx_info = np.array([int(sel.sum()), int(kept.sum()), int(heads.size), 0], dtype=np.int32)
    return (rel[heads], begin[heads], nxt[tails], (tails - heads + 1).astype(np.int64)), ctx_info


def plane_of(values, count=None, trailer=0):
    """a plane in the scan's cell layout that holds values: [count, values..., trailer]"""
    v = np.asarray(values, dtype=np.int64)
    return np.concatenate([[v.size if count is None else count], v, [trailer]]).astype(np.int32)


def extract(text, origin, begin_plane, end_plane, max_ranges, inclusive=False, glue=b"", terminator=-1, seg_start=None,
            limit=None):
    """The extract pass over the planes as they are (cells may hold anything).  Returns a dict: out (the first
    min(m, limit) bytes; limit None: all), m, at (list, saturated), seg_out (int32 array or None), info (int32[8]
    for an output buffer of limit bytes; limit None: never cut)."""
    t = bytes(text)
    n = len(t)
    end_text = origin + n
    bp = np.asarray(begin_plane, dtype=np.int64)
    ep = np.asarray(end_plane, dtype=np.int64)
    count = min(max(int(bp[0]), 0), max_ranges)
    seg = np.asarray(seg_start, dtype=np.int64) if seg_start is not None else None
    glue = bytes(glue)
    parts, at, sizes, bs = [], [], [], []
    used = skipped = terms = 0
    m = src = 0
    prev_tid = None
    for i in range(count):
        b = int(bp[1 + i])
        e = int(ep[1 + i]) + (1 if inclusive else 0)
        if not (origin <= b < e <= end_text):
            skipped += 1
            continue
        tid = int(np.searchsorted(seg, b, side="right")) if seg is not None else 0
        size = 0
        if prev_tid is not None and prev_tid == tid:
            parts.append(glue)
            size += len(glue)
        at.append(_sat32(m + size))
        parts.append((b - origin, e - origin))          # (sliced when the output is put together: it may be cut)
        size += e - b
        src += e - b
        if terminator >= 0 and t[e - origin - 1] != terminator:
            parts.append(bytes([terminator]))
            size += 1
            terms += 1
        used += 1
        m += size
        sizes.append(size)
        bs.append(b)
        prev_tid = tid
    want = m if limit is None else min(m, limit)
    out, have = bytearray(), 0
    for p in parts:
        if have >= want:
            break
        out += p[:want - have] if isinstance(p, bytes) else t[p[0]:min(p[1], p[0] + want - have)]
        have = len(out)
    seg_out = None
    if seg is not None:
        sz, bb = np.asarray(sizes, dtype=np.int64), np.asarray(bs, dtype=np.int64)
        seg_out = np.array([_sat32(int(sz[bb < x].sum())) for x in seg], dtype=np.int32)
    info = np.array([used, skipped, m & 0xFFFFFFFF, m >> 32, src & 0xFFFFFFFF, src >> 32,
                     1 if (limit is not None and m > limit) else 0, min(terms, INT32_MAX)], dtype=np.uint32).astype(np.int32)
    return dict(out=bytes(out), m=m, at=at, seg_out=seg_out, info=info)


def at_plane(at, cap, poison):
    """the d_at_out plane of cap cells a call must leave"""
    return lm.planes((at,), cap, poison)[0]


def grep_like(text, offsets, before=0, after=0, invert=False, delimiter=0x0A, seg_start=(), glue=None, terminator=None):
    """index + context + extract over one whole text: (output bytes, groups, extract dict)"""
    t = bytes(text)
    _, info, st = lm.index(t, 0, delimiter)
    groups, ctx_info = context(st, info, 0, len(t), offsets, invert, before, after, seg_start)
    if glue is None:
        glue = b"--" + bytes([delimiter]) if before + after > 0 else b""
    term = delimiter if terminator is None else terminator
    ex = extract(t, 0, plane_of(groups[1]), plane_of(groups[2]), len(groups[1]), glue=glue, terminator=term,
                 seg_start=seg_start if len(seg_start) else None)
    return ex["out"], groups, ex
