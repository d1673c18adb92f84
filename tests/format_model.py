"""numpy / plain-Python model of the per-line context pass (acm_line_context_lines_async) and of the formatting
extract (acm_format_async).  Written from the rules in include/acmatch.h, not from the kernels: the GPU tests compare
the library with it cell for cell and byte for byte, test_host_format.py checks it against a brute force and against
GNU grep (a test helper, not a conftest).  It builds on line_model.py and extract_model.py."""
import numpy as np

import extract_model as xm
import line_model as lm

INT32_MAX = 0x7FFFFFFF
SELECTED, HEAD = 1, 2
END_INCLUSIVE, NAME, NUMBER, OFFSET = 1, 2, 4, 8
MAX_NAME = 4096

plane_of = xm.plane_of


def context_lines(starts, info, origin, end, offsets, invert=False, before=0, after=0, seg_start=()):
    """(rel, begin, next, kind) int64 arrays of the kept lines, and ctx_info int32[4]"""
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
    head = kept & ~joined
    kind = (sel.astype(np.int64) * SELECTED + head.astype(np.int64) * HEAD)[kept]
    ctx_info = np.array([int(sel.sum()), int(kept.sum()), int(head.sum()), 0], dtype=np.int32)
    return (rel[kept], begin[kept], nxt[kept], kind), ctx_info


def groups_of(lines):
    """the group planes (rel, begin, next, lines) of acm_line_context_async rebuilt from the per-line entries"""
    rel, begin, nxt, kind = (np.asarray(x, dtype=np.int64) for x in lines)
    heads = np.flatnonzero(kind & HEAD)
    tails = np.concatenate([heads[1:] - 1, [rel.size - 1]]).astype(np.int64) if heads.size else heads
    return rel[heads], begin[heads], nxt[tails], tails - heads + 1


def name_of(names, name_off, names_bytes, t):
    a, z = int(name_off[t]), int(name_off[t + 1])
    if 0 <= a <= z <= names_bytes and z - a <= MAX_NAME:
        return bytes(names[a:z])
    return b""


def format(text, origin, begin_plane, end_plane, max_ranges, flags=0, kind_plane=None, num_plane=None, seg_num=None,
           number_base=0, offset_base=0, sel_sep=0x3A, ctx_sep=0x2D, names=b"", name_off=None, names_bytes=None, glue=b"",
           terminator=-1, seg_start=None, limit=None):
    """The format pass over the planes as they are (cells may hold anything).  Returns extract_model.extract's dict:
    out (the first min(m, limit) bytes; limit None: all), m, at, seg_out, info."""
    t = bytes(text)
    n = len(t)
    end_text = origin + n
    bp = np.asarray(begin_plane, dtype=np.int64)
    ep = np.asarray(end_plane, dtype=np.int64)
    kp = np.asarray(kind_plane, dtype=np.int64) if kind_plane is not None else None
    nump = np.asarray(num_plane, dtype=np.int64) if num_plane is not None else None
    count = min(max(int(bp[0]), 0), max_ranges)
    seg = np.asarray(seg_start, dtype=np.int64) if seg_start is not None and len(seg_start) else None
    names = bytes(names)
    names_bytes = len(names) if names_bytes is None else names_bytes
    glue = bytes(glue)
    inclusive = bool(flags & END_INCLUSIVE)
    out = bytearray()
    at, sizes, bs = [], [], []
    used = skipped = terms = 0
    src = 0
    prev_tid = None
    for i in range(count):
        b = int(bp[1 + i])
        e = int(ep[1 + i]) + (1 if inclusive else 0)
        if not (origin <= b < e <= end_text):
            skipped += 1
            continue
        tid = int(np.searchsorted(seg, b, side="right")) if seg is not None else 0
        kind = int(kp[1 + i]) & 3 if kp is not None else SELECTED
        sep = bytes([sel_sep if kind & SELECTED else ctx_sep])
        part = bytearray()
        if kind & HEAD and prev_tid is not None and prev_tid == tid:
            part += glue
        if flags & NAME:
            part += name_of(names, name_off, names_bytes, tid) + sep
        if flags & NUMBER:
            first = int(seg_num[tid - 1]) if tid > 0 and seg_num is not None else 0
            part += b"%d" % max(number_base + int(nump[1 + i]) - first, 0) + sep
        if flags & OFFSET:
            first = int(seg[tid - 1]) if tid > 0 else origin
            part += b"%d" % max(offset_base + b - first, 0) + sep
        at.append(xm._sat32(len(out) + len(part)))
        part += t[b - origin:e - origin]
        src += e - b
        if terminator >= 0 and t[e - origin - 1] != terminator:
            part.append(terminator)
            terms += 1
        used += 1
        out += part
        sizes.append(len(part))
        bs.append(b)
        prev_tid = tid
    m = len(out)
    seg_out = None
    if seg is not None:
        sz, bb = np.asarray(sizes, dtype=np.int64), np.asarray(bs, dtype=np.int64)
        seg_out = np.array([xm._sat32(int(sz[bb < x].sum())) for x in seg], dtype=np.int32)
    info = np.array([used, skipped, m & 0xFFFFFFFF, m >> 32, src & 0xFFFFFFFF, src >> 32,
                     1 if (limit is not None and m > limit) else 0, min(terms, INT32_MAX)], dtype=np.uint32).astype(np.int32)
    return dict(out=bytes(out if limit is None else out[:limit]), m=m, at=at, seg_out=seg_out, info=info)


def name_table(names, segments):
    """(bytes, int32 offsets[segments + 2]) of a list of segments + 1 names"""
    assert len(names) == segments + 1
    off = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.int32)
    return b"".join(names), off


def grep_like(text, offsets, before=0, after=0, invert=False, seg_start=(), names=None, with_name=False, line_number=False,
              byte_offset=False, glue=None, terminator=None, delimiter=0x0A):
    """index + per-line context + format over one whole text, as Matcher.scan_format runs them: (output bytes, the
    lines, format dict).  names: one per text (len(seg_start) of them, or one without texts)"""
    t = bytes(text)
    _, info, st = lm.index(t, 0, delimiter)
    lines, ctx_info = context_lines(st, info, 0, len(t), offsets, invert, before, after, seg_start)
    if glue is None:
        glue = b"--" + bytes([delimiter]) if before + after > 0 else b""
    term = delimiter if terminator is None else terminator
    seg = [int(x) for x in seg_start]
    flags = (NAME if with_name else 0) | (NUMBER if line_number else 0) | (OFFSET if byte_offset else 0)
    tab, off = name_table([b""] + [bytes(x) for x in names] if seg else [bytes(names[0])], len(seg)) if with_name else (b"", None)
    seg_num = lm.number(st, info, seg) if seg else None
    fm = format(t, 0, plane_of(lines[1]), plane_of(lines[2]), len(lines[1]), flags, plane_of(lines[3]), plane_of(lines[0]),
                seg_num, 1, 0, 0x3A, 0x2D, tab, off, None, glue, term, seg if seg else None)
    return fm["out"], lines, fm
