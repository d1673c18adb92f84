"""The per-line context pass and the format pass on the device (acm_line_context_lines_async, acm_format_async,
Matcher.scan_format), through the C ABI, compared cell for cell and byte for byte with tests/format_model.py.  Every
output has guard cells or bytes on both sides and is pre-filled (tests/ops_guard.py), the workspace and the text's tail
are poisoned as tests/test_gpu_extract.py does; the name table lies between guards too, so a read that leaves it shows
in the output."""
import numpy as np
import pytest

import extract_model as xm
import format_model as fm
import line_model as lm
import ops_guard as og
from gpu_pattern_matching_amd import AcmError, DeviceArray, _lib
from gpu_pattern_matching_amd._lib import check
from streams import Rig
from test_gpu_extract import (PATS, Extract, compare, find_all, pieces, random_text, run_context, small_matcher, text_of_lines,
                              upload_text, word_lines)
from test_gpu_lines import Index, device_text

pytestmark = pytest.mark.gpu

TILE = 16384                 # output bytes a workgroup of the copy kernel owns
INT32_MAX = 0x7FFFFFFF
NAME, NUMBER, OFFSET = fm.NAME, fm.NUMBER, fm.OFFSET
ALL = NAME | NUMBER | OFFSET


def _ptr(x):
    return x if isinstance(x, int) or x is None else x.ptr


class Format:
    """one format call from poisoned outputs; read() checks the guard bands"""

    def __init__(self, lib, d_text, n, bp, ep, max_ranges, cap, origin=0, flags=0, kind=None, num=None, seg_num=None, nbase=0,
                 obase=0, sel=0x3A, ctx=0x2D, names=None, name_off=None, names_bytes=None, glue=b"", term=-1, at_cap=None,
                 seg=None, with_out=True, ws_fill=0xA5, stream=None):
        self.lib, self.stream, self.with_out = lib, stream, with_out
        self.out = og.Guarded(cap if with_out else 16, dtype=np.uint8)
        self.at = og.Guarded(at_cap) if at_cap is not None else None
        nseg = 0 if seg is None else len(seg)
        self.seg_in = og.Guarded(max(nseg, 1), host=np.asarray(seg, dtype=np.int32)) if nseg else None
        self.seg = og.Guarded(nseg) if nseg else None
        self.seg_num = og.Guarded(max(nseg, 1), host=np.asarray(seg_num, dtype=np.int32)) if seg_num is not None else None
        self.names = og.Guarded(max(len(names), 1), host=np.frombuffer(bytes(names), dtype=np.uint8), dtype=np.uint8) \
            if names is not None else None
        self.name_off = og.Guarded(nseg + 2, host=np.asarray(name_off, dtype=np.int32)) if name_off is not None else None
        self.info = og.Guarded(8)
        nb = lib.acm_format_workspace_bytes(max_ranges, nseg)
        self.ws = og.Workspace(nb, ws_fill)
        nbytes = (len(names) if names is not None else 0) if names_bytes is None else names_bytes
        self.go = lambda: check(lib.acm_format_async(
            d_text.ptr if d_text is not None else None, n, origin, _ptr(bp), _ptr(ep), max_ranges, flags, _ptr(kind), _ptr(num),
            _ptr(self.seg_num), nbase, obase, sel, ctx, _ptr(self.names), _ptr(self.name_off), nbytes, glue if glue else None,
            len(glue), term, self.out.ptr if with_out else None, cap if with_out else 0, self.at.ptr if self.at else None,
            at_cap or 0, self.seg_in.ptr if nseg else None, nseg, self.seg.ptr if nseg else None, self.info.ptr, self.ws.ptr, nb,
            stream), "acm_format_async")
        self.go()

    def read(self, what="", free=True):
        st = self.stream
        self.ws.check(st, what)
        res = dict(out=self.out.read(st, what), info=self.info.read(st, what),
                   at=self.at.read(st, what) if self.at else None, seg=self.seg.read(st, what) if self.seg else None)
        for x in (self.names, self.name_off, self.seg_num, self.seg_in):
            if x is not None:
                x.read(st, what)                  # (inputs: their guards stay too)
        if free:
            for x in (self.out, self.at, self.seg_in, self.seg, self.seg_num, self.names, self.name_off, self.info, self.ws):
                if x is not None:
                    x.free()
        return res


def run(lib, text, begins, ends, flags=0, kinds=None, nums=None, seg_num=None, nbase=0, obase=0, sel=0x3A, ctx=0x2D, names=None,
        name_off=None, names_bytes=None, origin=0, cap=None, glue=b"", term=-1, seg=None, max_ranges=None, count=None,
        at_cap="fit", with_out=True, what="", d_text=None, ws_fill=0xA5):
    """one call over host ranges, compared whole with the model; returns the model's dict"""
    begins, ends = np.asarray(begins, dtype=np.int64), np.asarray(ends, dtype=np.int64)
    mr = len(begins) if max_ranges is None else max_ranges
    bp, ep = fm.plane_of(begins, count), fm.plane_of(ends, count)
    kp = fm.plane_of(kinds, count) if kinds is not None else None
    nump = fm.plane_of(nums, count) if nums is not None else None
    if names is not None and name_off is None:
        names, name_off = fm.name_table(names, 0 if seg is None else len(seg))
    args = (text, origin, bp, ep, mr, flags, kp, nump, seg_num, nbase, obase, sel, ctx, names if names is not None else b"",
            name_off, names_bytes, glue, term, seg)
    full = fm.format(*args)
    cap = full["m"] + 37 if cap is None else cap
    exp = fm.format(*args, limit=cap) if with_out else full
    at_cap = len(full["at"]) + 5 if at_cap == "fit" else at_cap
    dt = d_text if d_text is not None else upload_text(text)
    dev = [DeviceArray.from_numpy(p, pad_to=0) if p is not None else None for p in (bp, ep, kp, nump)]
    got = Format(lib, dt, len(text), dev[0], dev[1], mr, cap, origin, flags, dev[2], dev[3], seg_num, nbase, obase, sel, ctx,
                 names, name_off, names_bytes, glue, term, at_cap, seg, with_out, ws_fill).read(what)
    compare(got, exp, cap, at_cap, with_out, "%s n=%d ranges=%d cap=%d origin=%d flags=%d" % (what, len(text), len(begins), cap,
                                                                                             origin, flags))
    for b in dev + ([dt] if d_text is None else []):
        if b is not None:
            b.free()
    return full


def line_ranges(t):
    """(begin, end, 0-based number) of every line of t"""
    _, info, st = lm.index(t)
    rel, b, e = lm.lines_of(st, info, 0, len(t))
    return b, e, rel


# ------------------------------------------------------------------ format

@pytest.mark.parametrize("m", (0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 3 * TILE + 5))
def test_output_lengths(gpu, lib, m):
    """ranges of 20 to 200 bytes, each behind name:number:offset:, that give exactly m bytes of output"""
    name = b"dir/a.txt"
    t = random_text(m + 600, m, newline=0)
    begins, ends, nums, at = [], [], [], 3
    for k in pieces(m, m + 1):
        if k <= len(name) + 1 + len(b"%d:%d:" % (len(begins) + 1, at)):       # no room for a prefix and a byte: the range in front grows
            if not begins:
                break
            ends[-1] += k
            at += k
            continue
        k -= len(name) + 1 + len(b"%d:%d:" % (len(begins) + 1, at))
        begins.append(at)
        ends.append(at + k)
        nums.append(len(begins) - 1)
        at += k + len(begins) % 3
    full = run(lib, t, begins, ends, ALL, nums=nums, nbase=1, names=[name], what="m = %d" % m)
    assert full["m"] == (m if begins else 0)
    run(lib, t, begins, ends, ALL, kinds=[1 + 2 * (i % 2) for i in range(len(begins))], nums=nums, nbase=1, names=[name],
        glue=b"--\n", term=0x0A, what="m = %d, glued" % m)


def test_a_prefix_across_a_tile_border(gpu, lib):
    t = random_text(2 * TILE, 1, newline=0)
    dt = upload_text(t)
    glue, name = b"--\n", b"some/file"
    for first in range(TILE - 36, TILE + 2):
        # the first range's output ends at first: the glue, the name, the two numbers and their separators of the
        # second lie at first, first + 1, ...: every split of them over the border between two tiles
        k = first - len(b"some/file:7:5:")
        full = run(lib, t, [5, TILE + 100], [5 + k, TILE + 140], ALL, kinds=[3, 2], nums=[6, 123456], nbase=1, names=[name],
                   glue=glue, d_text=dt, what="border %d" % first)
        assert full["at"][1] == first + len(b"--\nsome/file-123457-16484-")
    dt.free()


@pytest.mark.parametrize("k", range(1, 19))
def test_digit_counts(gpu, lib, k):
    """10^k - 1, 10^k and 10^k + 1 for both numbers, reached through the bases on a tiny text"""
    t = b"ab\ncd\nef\n"
    b, e, rel = line_ranges(t)
    base = 10 ** k - 1
    full = run(lib, t, b, e, NUMBER | OFFSET, nums=rel, nbase=base, obase=base, what="10^%d" % k)
    assert full["out"].startswith(b"%d:%d:ab\n%d:%d:cd\n" % (base, base, base + 1, base + 3))
    if k == 18:
        run(lib, t, b, e, NUMBER | OFFSET, nums=rel, nbase=10 ** 18, obase=10 ** 18, what="the largest bases")
        o = INT32_MAX - 20                      # the largest values there are: 10^18 + 2^32 - 1 and 10^18 + 2^32 - 15
        full = run(lib, t, b + o, e + o, NUMBER | OFFSET, nums=[INT32_MAX] * 3, nbase=10 ** 18, obase=10 ** 18, origin=o,
                   seg=[-(1 << 31)], seg_num=[-(1 << 31)], what="largest values")
        assert full["out"].startswith(b"%d:%d:ab\n" % (10 ** 18 + (1 << 32) - 1, 10 ** 18 + (1 << 32) - 21))
        # negative values print as 0
        full = run(lib, t, b, e, NUMBER | OFFSET, nums=[-5, 0, 3], nbase=2, seg=[3], seg_num=[4], what="negative values")
        assert full["out"] == b"0:0:ab\n0:0:cd\n1:3:ef\n"


def test_name_lengths(gpu, lib):
    lens = (0, 1, 15, 16, 17, 255, 4096)
    rng = np.random.default_rng(2)
    names = [b""] + [bytes(rng.integers(0x41, 0x5B, size=k).astype(np.uint8)) for k in lens]
    t = text_of_lines(5 * len(lens), 3)
    b, e, rel = line_ranges(t)
    seg = [int(x) for x in b[::5]]
    assert len(seg) == len(lens)
    full = run(lib, t, b, e, ALL, kinds=[1, 0, 2, 3, 0] * len(lens), nums=rel, nbase=1, names=names, seg=seg, glue=b"--\n",
               seg_num=[int(x) for x in rel[::5]], what="names")
    assert full["m"] > TILE + 4096          # the longest name lies across a tile border, and in a tile of its own
    full = run(lib, t, b, e, NAME, names=names, seg=seg, what="names only")
    for cut in (1, 4095, 4096, 4097, 5000):             # the last text's part begins with its name
        run(lib, t, b, e, NAME, names=names, seg=seg, cap=int(full["seg_out"][-1]) + cut, what="a cut name")


def test_a_garbage_name_table(gpu, lib):
    t = text_of_lines(40, 4)
    b, e, rel = line_ranges(t)
    seg = [int(x) for x in b[4::4]]
    names = bytes(range(0x61, 0x7B)) * 200                    # 5200 bytes
    P = og.FILL32
    for i, off in enumerate(([5, 4, 3, 2, 1, 0, -1, -2, 7, 7, 9],          # descending, negative, empty
                             [0, 4097, 5200, 5201, 5200, P, -P, INT32_MAX, 0, 26, 52],
                             [-(1 << 31), INT32_MAX] * 5 + [0],
                             [5199, 5200, 5201, 5200, 5199, 1103, 5199, 5200, 0, 4096, 4097])):
        full = run(lib, t, b, e, NAME | NUMBER, nums=rel, names=names, name_off=off, seg=seg, what="garbage table %d" % i)
        run(lib, t, b, e, NAME, names=names, name_off=off, names_bytes=100, seg=seg, what="garbage table %d, 100 bytes" % i)
    assert b"\n" + names[5199:5200] + b":" in full["out"]


def test_more_lines_in_a_tile_than_threads(gpu, lib):
    """5000 one-byte lines, each with a full prefix"""
    t = b"\n" * 5000
    b, e, rel = line_ranges(t)
    full = run(lib, t, b, e, ALL, nums=rel, nbase=1, names=[b"n"], what="5000 one-byte lines")
    assert full["info"][0] == 5000 and full["out"].endswith(b"n:5000:4999:\n")
    run(lib, t, b, e, ALL, kinds=np.arange(5000) % 4, nums=rel, nbase=1, names=[b"n"], glue=b"--\n", what="5000 lines, kinds")


def test_a_line_longer_than_a_tile(gpu, lib):
    n = 5 * TILE // 2
    t = random_text(n + 100, 7, newline=0)
    for b in (0, 3, 16):
        run(lib, t, [b], [b + n], ALL, nums=[0], names=[b"x/y"], what="2.5 tiles")
        run(lib, t, [50, b, 60], [53, b + n, 70], ALL, kinds=[1, 2, 3], nums=[4, 5, 6], names=[b"x/y"], glue=b"--\n", term=0x0A,
            what="2.5 tiles between two short ranges")


def test_every_source_and_destination_phase(gpu, lib):
    """a 40-byte range at each of the 16 x 16 (source phase, destination phase) pairs, behind a prefix of three bytes: a
    filler range (a prefix of three bytes too) brings the output to the wanted phase"""
    t = random_text(4096, 5)
    begins, ends, nums, pos, mine = [], [], [], 0, []
    for s in range(16):
        for d in range(16):
            fill = (d - pos - 6) % 16 or 16
            begins.append(1000)
            ends.append(1000 + fill)
            b = 64 + 48 * d + s + 16 * ((s * 16 + d) % 3)
            mine.append(len(begins))
            begins.append(b)
            ends.append(b + 40)
            pos += fill + 46
            nums += [10 + s, 20 + d]
    full = run(lib, t, begins, ends, NUMBER, nums=nums, what="phases")
    assert {(begins[i] % 16, full["at"][i] % 16) for i in mine} == {(s, d) for s in range(16) for d in range(16)}
    assert full["m"] == pos


def test_kind_planes(gpu, lib):
    t = text_of_lines(600, 8)
    b, e, rel = line_ranges(t)
    rng = np.random.default_rng(8)
    seg = [int(x) for x in b[::37]]
    for high in (0, 1):
        kinds = rng.integers(0, 4, size=b.size) | (rng.integers(-(1 << 29), 1 << 29, size=b.size) << 2) * high
        assert set((kinds & 3).tolist()) == {0, 1, 2, 3}
        run(lib, t, b, e, ALL, kinds=kinds, nums=rel, nbase=1, names=[b""] + [b"f%d" % i for i in range(len(seg))], seg=seg,
            glue=b"--\n", term=0x0A, sel=0x3D, ctx=0x00, what="kinds, high bits %d" % high)
        run(lib, t, b, e, 0, kinds=kinds, glue=b"0123456789abcdef", what="kinds, no prefix")
    # no kind plane: every range selected, none a head
    full = run(lib, t, b, e, NUMBER, nums=rel, glue=b"--\n", what="no kind plane")
    assert b"--" not in full["out"] and full["out"].startswith(b"0:")


def test_glue_across_skipped_cells(gpu, lib):
    t = random_text(1000, 9, newline=0)
    P = og.FILL32
    b = [10, P, -5, 40, 2000, 60, 900, 80]
    e = [20, P, 5, 50, 2001, 60, 1001, 90]
    k = [3, 2, 2, 3, 2, 3, 3, 3]
    full = run(lib, t, b, e, OFFSET, kinds=k, glue=b"--\n", seg=[70], what="skipped cells in between")
    # the glue in front of the second used range, none in front of the third: it is another text's
    assert full["out"] == b"10:" + t[10:20] + b"--\n40:" + t[40:50] + b"10:" + t[80:90] and full["info"][1] == 5
    # a block border between the two used ranges: 3000 skipped cells
    b2, e2 = [10] + [P] * 3000 + [40], [20] + [0] * 3000 + [50]
    full = run(lib, t, b2, e2, 0, kinds=[2] * 3002, glue=b"--\n", what="a block of skipped cells")
    assert full["out"] == t[10:20] + b"--\n" + t[40:50]


def test_seg_num_and_skipped_ranges(gpu, lib):
    t = random_text(1000, 12)
    P = og.FILL32
    for origin in (0, -300, 5000):
        o = origin
        b = [o - 1, o, o + 10, o + 990, o + 20, o + 30, P, o + 40, -P, o + 1000, o + 999]
        e = [o + 5, o + 5, o + 10, o + 1001, o + 19, o + 35, o + 50, P, o + 60, o + 1001, o + 1000]
        for seg_num in (None, [7]):
            full = run(lib, t, b, e, ALL, kinds=[3] * len(b), nums=list(range(10, 10 + len(b))), seg_num=seg_num, nbase=1,
                       names=[b"one", b"two"], origin=origin, glue=b"--\n", term=0x0A, seg=[o + 25],
                       what="skipped, origin %d" % origin)
            assert full["info"][0] == 3 and full["info"][1] == len(b) - 3
            assert full["out"].startswith(b"one:12:0:") and (b"two:%d:5:" % (16 - (7 if seg_num else 0))) in full["out"]
    full = run(lib, t, [-5, 2000], [3, 2001], ALL, nums=[1, 2], names=[b"x"], what="all skipped")
    assert full["m"] == 0 and full["info"][1] == 2
    for count, mr in ((-1, 30), (1000, 30), (INT32_MAX, 12), (7, 30), (0, 30), (30, 0)):
        bb = np.arange(0, 900, 30)
        run(lib, t, bb, bb + 20, NUMBER, kinds=[2] * 30, nums=bb, glue=b"-", count=count, max_ranges=mr, what="count %d" % count)
    run(lib, t, [0, 10], [9, 19], NUMBER | fm.END_INCLUSIVE, nums=[1, 2], what="inclusive ends")


def test_capacities(gpu, lib):
    t = random_text(40000, 16)
    name = bytes(range(0x41, 0x5B)) * 4
    b, e = [10, 20000, 100], [10 + 18000, 20000 + 17000, 150]
    kw = dict(flags=ALL, kinds=[3, 3, 2], nums=[5, 123456789, 7], nbase=1, names=[name], glue=b"0123456789abcdef", term=0x0A)
    full = run(lib, t, b, e, **kw)
    m = full["m"]
    bytes_at = full["at"][1]
    pre = len(name) + 1 + 10 + 6                # the second range's prefix: the name, 123456790:, 20000:
    glue_at = bytes_at - pre - 16
    caps = [0, 1, 15, 16, 17, 9000, TILE, m - 1, m, m + 1]
    caps += [glue_at + x for x in (0, 1, 7, 16)]                          # inside the glue
    caps += [glue_at + 16 + x for x in (1, 50, len(name), len(name) + 1)]     # inside the name, on its separator
    caps += [bytes_at - 17 + x for x in (0, 1, 5, 9, 10, 11, 16)]         # inside the numbers
    caps += [bytes_at + x for x in (0, 1, 15, 16, 17)]                    # inside the bytes
    for cap in caps:
        run(lib, t, b, e, cap=cap, what="capacity %d of %d" % (cap, m), **kw)
    run(lib, t, b, e, with_out=False, what="NULL output", **kw)
    for at_cap in (2, 3, 4, 5, None):
        run(lib, t, b, e, at_cap=at_cap, what="at_capacity %s" % at_cap, **kw)


def test_without_flags_it_is_the_extract(gpu, lib):
    """no flags and no kind plane: acm_extract_async with glue_len = 0, whatever glue is given"""
    t = random_text(50000, 18)
    lens = pieces(40000, 19)
    b = np.cumsum(np.r_[0, lens[:-1]]) + np.arange(len(lens))
    e = b + np.asarray(lens)
    seg = [0, 20000, 45000]
    for glue in (b"", b"--\n", b"0123456789abcdef"):
        full = run(lib, t, b, e, glue=glue, term=0x0A, seg=seg, what="no flags, glue %d" % len(glue))
        ex = xm.extract(t, 0, xm.plane_of(b), xm.plane_of(e), len(b), terminator=0x0A, seg_start=seg)
        assert full["out"] == ex["out"] and full["at"] == ex["at"] and full["info"].tolist() == ex["info"].tolist()
        assert full["seg_out"].tolist() == ex["seg_out"].tolist()
    # ... and the library's extract over the same planes
    dt, dbp, dep = upload_text(t), DeviceArray.from_numpy(xm.plane_of(b), pad_to=0), DeviceArray.from_numpy(xm.plane_of(e), pad_to=0)
    x = Extract(lib, dt, len(t), dbp, dep, len(b), ex["m"] + 3, term=0x0A, at_cap=len(b) + 2, seg=seg).read("extract")
    f = Format(lib, dt, len(t), dbp, dep, len(b), ex["m"] + 3, glue=b"--\n", term=0x0A, at_cap=len(b) + 2, seg=seg).read("format")
    for k in x:
        assert np.array_equal(x[k], f[k]), "the extract and the format pass differ in %s" % k
    for d in (dt, dbp, dep):
        d.free()


# ------------------------------------------------------------------ the per-line context pass

def run_context_lines(lib, ix, origin, end, off_plane, max_records, invert, before, after, seg, ocap, stream=None, ws_fill=0xA5,
                      keep=None):
    nseg = 0 if seg is None else len(seg)
    outs = keep["outs"] if keep else [og.Guarded(ocap) for _ in range(4)]
    cinfo = keep["cinfo"] if keep else og.Guarded(4)
    seg_in = og.Guarded(max(nseg, 1), host=np.asarray(seg, dtype=np.int32)) if nseg else None
    nb = lib.acm_line_context_lines_workspace_bytes(ix.cap, nseg)
    ws = og.Workspace(nb, ws_fill)
    check(lib.acm_line_context_lines_async(ix.start_ptr, ix.cap, ix.info_ptr, origin, end, off_plane, max_records, invert, before,
                                           after, seg_in.ptr if nseg else None, nseg, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                           outs[3].ptr, ocap, cinfo.ptr, ws.ptr, nb, stream), "acm_line_context_lines_async")
    ws.check(stream)
    got = [b.read(stream) for b in outs], cinfo.read(stream)
    for b in ([] if keep else outs + [cinfo]) + [ws] + ([seg_in] if seg_in else []):
        b.free()
    return got


def check_lines(lib, t, offs, origin=0, prev=-1, invert=False, before=0, after=0, seg=None, ocap=None, what="", ix=None,
                d_off=None, groups=False):
    own = ix is None
    if own:
        ix = Index(lib, t, 0x0A, origin, prev)
    _, e_info, e_st = lm.index(t, origin, 0x0A, prev)
    end = origin + len(t)
    exp, e_ctx = fm.context_lines(e_st, e_info, origin, end, offs, invert, before, after, () if seg is None else seg)
    ocap = len(exp[0]) + 5 if ocap is None else ocap
    plane = d_off if d_off is not None else DeviceArray.from_numpy(fm.plane_of(offs), pad_to=0)
    got, ctx = run_context_lines(lib, ix, origin, end, plane.ptr, len(offs), 1 if invert else 0, before, after, seg, ocap)
    what = "%s lines=%d before=%d after=%d invert=%d capacity=%d" % (what, e_st.size, before, after, invert, ocap)
    assert ctx.tolist() == e_ctx.tolist(), "%s: ctx_info %s, model %s" % (what, ctx.tolist(), e_ctx.tolist())
    for g, x, name in zip(got, lm.planes(exp, ocap, og.FILL32), ("rel", "begin", "next", "kind")):
        og.same(g, x, "%s: %s plane" % (what, name))
    if groups:
        # the groups of acm_line_context_async over the same input, rebuilt from the kind bits
        k = int(e_ctx[2])
        dev, dctx = run_context(lib, ix, origin, end, plane.ptr, len(offs), 1 if invert else 0, before, after, seg, k + 2)
        assert dctx.tolist() == ctx.tolist()
        mine = fm.groups_of([g[1:1 + len(exp[0])] for g in got])
        for d, x, name in zip(dev, mine, ("rel", "begin", "next", "lines")):
            og.same(d[1:1 + k], x.astype(np.int32), "%s: the group form's %s" % (what, name))
    if d_off is None:
        plane.free()
    if own:
        ix.free()
    return exp, e_ctx


WINDOWS = ((0, 0), (1, 0), (0, 2), (2, 1), (31, 33), (32, 31), (33, 32), (1000, 2), (INT32_MAX, 0), (1, INT32_MAX),
           (INT32_MAX, INT32_MAX))


@pytest.mark.parametrize("lines", (0, 1, 31, 32, 33, 10007))
def test_context_lines_line_counts(gpu, lib, lines):
    rng = np.random.default_rng(lines)
    for prev in (-1, 0x41):                      # with a lead line and without
        t = text_of_lines(lines, lines + 1, last_newline=prev < 0)
        n = len(t)
        ix = Index(lib, t, 0x0A, 100, prev)
        picks = []
        if n:
            picks = [np.sort(rng.integers(0, n, size=max(1, lines // 60))) + 100, np.array([100, 100 + n - 1])]
        picks += [np.zeros(0, dtype=np.int64)]
        for offs in picks:
            d_off = DeviceArray.from_numpy(fm.plane_of(offs), pad_to=0)
            for i, (before, after) in enumerate(WINDOWS if lines > 1000 else WINDOWS[::2]):
                for invert in (False, True):
                    check_lines(lib, t, offs, 100, prev, invert, before, after, what="prev %d" % prev, ix=ix, d_off=d_off,
                                groups=i % 4 == 3 or lines < 100)
            d_off.free()
        ix.free()


def test_context_lines_everything_and_nothing_selected(gpu, lib):
    t = text_of_lines(3000, 20)
    _, _, st = lm.index(t)
    ix = Index(lib, t, 0x0A)
    for offs in (st, np.zeros(0, dtype=np.int64)):
        for invert in (False, True):
            exp, ctx = check_lines(lib, t, offs, invert=invert, before=2, after=2, ix=ix, groups=True)
            assert ctx[2] == (1 if ctx[0] else 0) and ctx[1] == ctx[0] and set(exp[3].tolist()) <= {1, 3}
    for offs in ([0], [len(t) - 1], [0, len(t) - 1]):
        for w in ((0, 0), (3, 3), (INT32_MAX, INT32_MAX)):
            check_lines(lib, t, offs, before=w[0], after=w[1], ix=ix, groups=True)
    ix.free()


def test_context_lines_text_barriers(gpu, lib):
    t = text_of_lines(4000, 21)
    n = len(t)
    _, _, st = lm.index(t, 50)
    rng = np.random.default_rng(21)
    offs = np.sort(rng.integers(0, n, size=120)) + 50
    on_lines = [int(x) for x in st[::500]]
    inside = [int(x) + 1 for x in st[100::700] if x + 1 < 50 + n]
    segs = {
        "on line starts": on_lines,
        "inside lines": inside,
        "equal starts": sorted(on_lines[:3] * 3),
        "beyond the end": on_lines[:2] + [50 + n, 50 + n + 10, INT32_MAX],
        "in front of the origin": [0, 49] + on_lines[1:3],
        "every line its own text": [int(x) for x in st],
        "mixed": sorted(on_lines + inside),
    }
    ix = Index(lib, t, 0x0A, 50)
    d_off = DeviceArray.from_numpy(fm.plane_of(offs), pad_to=0)
    for name, seg in segs.items():
        for before, after in ((0, 0), (2, 2), (0, 40), (1000, 1), (INT32_MAX, INT32_MAX)):
            for invert in (False, True):
                check_lines(lib, t, offs, 50, invert=invert, before=before, after=after, seg=seg, what=name, ix=ix, d_off=d_off,
                            groups=before == 2)
    d_off.free()
    ix.free()


def test_context_lines_capacities(gpu, lib):
    t = text_of_lines(500, 22)
    offs = np.arange(3, len(t), 97)
    ix = Index(lib, t, 0x0A)
    _, e_info, e_st = lm.index(t)
    kept = len(fm.context_lines(e_st, e_info, 0, len(t), offs, False, 1, 1)[0][0])
    assert kept > 30
    for ocap in (2, 3, 4, kept + 1, kept + 2, kept + 3):
        check_lines(lib, t, offs, before=1, after=1, ocap=ocap, ix=ix)
    ix.free()


# ------------------------------------------------------------------ both passes

def test_lines_and_a_glue_give_the_groups_bytes(gpu, lib):
    """no flags, the per-line planes and a glue: the bytes of the extract over the group planes (every line keeps its
    delimiter here, so no terminator falls inside a group)"""
    t = word_lines(3000, 26) + b"\n"
    offs = find_all(t, PATS)
    _, e_info, e_st = lm.index(t)
    seg = [0, len(t) // 3 + 1, len(t) // 2]
    for before, after, invert in ((0, 0, False), (1, 2, False), (2, 0, True)):
        lines, _ = fm.context_lines(e_st, e_info, 0, len(t), offs, invert, before, after, seg)
        groups, _ = xm.context(e_st, e_info, 0, len(t), offs, invert, before, after, seg)
        ex = xm.extract(t, 0, xm.plane_of(groups[1]), xm.plane_of(groups[2]), len(groups[1]), glue=b"--\n", terminator=0x0A,
                        seg_start=seg)
        full = run(lib, t, lines[1], lines[2], 0, kinds=lines[3], glue=b"--\n", term=0x0A, seg=seg, what="lines and glue")
        assert full["out"] == ex["out"] and full["seg_out"].tolist() == ex["seg_out"].tolist() and len(groups[1]) > 50


def test_both_passes_on_one_stream_twice(gpu, lib):
    """behind the index and the scan on a created stream, no sync in between, then once more into the same buffers"""
    t = word_lines(20000, 25)
    n = len(t)
    m = small_matcher(PATS, n)
    offs = np.asarray(find_all(t, PATS), dtype=np.int64)
    rig = Rig()
    s = rig.stream()
    d = device_text(t, 0x0A)
    _, e_info, e_st = lm.index(t)
    lcap = int(e_st.size) + 7
    seg = [0, n // 2]
    lines, e_ctx = fm.context_lines(e_st, e_info, 0, n, offs, False, 1, 2, seg)
    k = len(lines[0])
    assert k > 1000
    names, name_off = fm.name_table([b"", b"first/file", b"second"], 2)
    seg_num = lm.number(e_st, e_info, seg)
    exp = fm.format(t, 0, fm.plane_of(lines[1]), fm.plane_of(lines[2]), k, ALL, fm.plane_of(lines[3]), fm.plane_of(lines[0]),
                    seg_num, 1, 0, 0x3A, 0x2D, names, name_off, None, b"--\n", 0x0A, seg)
    cap = m.plane_capacity
    starts, linfo, cinfo, xinfo = og.Guarded(lcap), og.Guarded(8), og.Guarded(4), og.Guarded(8)
    planes = [og.Guarded(k + 2) for _ in range(4)]
    out, at, seg_out = og.Guarded(exp["m"], dtype=np.uint8), og.Guarded(k + 2), og.Guarded(2)
    seg_in = og.Guarded(2, host=np.array(seg, dtype=np.int32))
    d_seg_num = og.Guarded(2, host=np.asarray(seg_num, dtype=np.int32))
    d_names = og.Guarded(len(names), host=np.frombuffer(names, dtype=np.uint8), dtype=np.uint8)
    d_off = og.Guarded(4, host=name_off)
    wss = [og.Workspace(lib.acm_line_index_workspace_bytes(n)), og.Workspace(lib.acm_line_context_lines_workspace_bytes(lcap, 2)),
           og.Workspace(lib.acm_format_workspace_bytes(k, 2))]
    lib.acm_rt_device_sync()
    runs = []
    for _ in range(2):
        m.line_index_async(d, n, starts.ptr, lcap, linfo.ptr, workspace=(wss[0].ptr, wss[0].nbytes), stream=s)
        m.scan_async(d, n, 0, stream=s)
        m.line_context_lines_async(starts.ptr, lcap, linfo.ptr, 0, n, m.off_plane, cap - 2, planes[0].ptr, planes[1].ptr,
                                   planes[2].ptr, planes[3].ptr, k + 2, cinfo.ptr, before=1, after=2, seg_start=seg_in.ptr,
                                   segments=2, workspace=(wss[1].ptr, wss[1].nbytes), stream=s)
        m.format_async(d, n, planes[1].ptr, planes[2].ptr, k, out.ptr, exp["m"], xinfo.ptr, kind_plane=planes[3].ptr,
                       num_plane=planes[0].ptr, seg_num=d_seg_num.ptr, number=True, offset=True, names=d_names.ptr,
                       name_off=d_off.ptr, names_bytes=len(names), glue=b"--\n", terminator=0x0A, at_out=at.ptr, at_capacity=k + 2,
                       seg_start=seg_in.ptr, segments=2, seg_out=seg_out.ptr, workspace=(wss[2].ptr, wss[2].nbytes), stream=s)
        runs.append([x.read(s) for x in planes + [cinfo, xinfo, out, at, seg_out]])
    for w in wss:
        w.check(s)
    first, second = runs
    for g, x in zip(first[:4], lm.planes(lines, k + 2, og.FILL32)):
        og.same(g, x, "lines")
    assert first[4].tolist() == e_ctx.tolist() and first[5].tolist() == exp["info"].tolist()
    assert first[6].tobytes() == exp["out"]
    og.same(first[7], xm.at_plane(exp["at"], k + 2, og.FILL32), "at plane")
    og.same(first[8], exp["seg_out"], "seg_out")
    for x, y in zip(first, second):
        assert np.array_equal(x, y), "the second run left other cells"
    for b in [starts, linfo, cinfo, xinfo, out, at, seg_out, seg_in, d_seg_num, d_names, d_off, d] + planes + wss:
        b.free()
    rig.close()
    m.close()


def test_scan_format(gpu, lib):
    t = word_lines(6000, 23, hit=0.15)
    m = small_matcher(PATS, len(t))
    offs = find_all(t, PATS)
    assert len(offs) > 1000
    modes = [dict(with_name=h, line_number=n, byte_offset=b) for h in (False, True) for n in (False, True) for b in (False, True)]
    for i, mode in enumerate(modes):
        before, after, invert = ((0, 0, False), (2, 2, False), (1, 3, True), (0, 0, True), (INT32_MAX, 0, False))[i % 5]
        data, lines, at, info, seg = m.scan_format(t, names=[b"the/file"], before=before, after=after, invert=invert, **mode)
        exp_out, exp_lines, ex = fm.grep_like(t, offs, before, after, invert, names=[b"the/file"], **mode)
        assert data == exp_out and seg is None and info.tolist() == ex["info"].tolist() and at.tolist() == ex["at"], mode
        assert np.array_equal(lines, np.stack([exp_lines[0] + 1] + list(exp_lines[1:]), axis=1))
        if not any(mode.values()):
            assert data == m.scan_extract(t, before=before, after=after, invert=invert)[0]
    full = dict(with_name=True, line_number=True, byte_offset=True)
    # a glue and a terminator of the caller's
    data = m.scan_format(t, names=[b"f"], before=1, after=1, glue=b"~", terminator=-1, **full)[0]
    assert data == fm.grep_like(t, offs, 1, 1, names=[b"f"], glue=b"~", terminator=-1, **full)[0]
    # texts: each with its own name, numbered and counted alone; context and glue stay inside a text
    texts = [b"a\nneedle\nb\nc\n", b"d\ne\nhay\n", b"", b"f\n", b"g\nne\nh\ni\nhay"]
    names = [b"t0", b"t1", b"t2", b"t3", b"t4"]
    data, lines, at, info, seg = m.scan_format(texts=texts, names=names, before=1, after=1, **full)
    assert data == (b"t0-1-0-a\nt0:2:2:needle\nt0-3-9-b\n" + b"t1-2-2-e\nt1:3:4:hay\n" +
                    b"t4-1-0-g\nt4:2:2:ne\nt4-3-5-h\nt4-4-7-i\nt4:5:9:hay\n")
    starts = np.cumsum([0] + [len(x) for x in texts[:-1]])
    whole = b"".join(texts)
    exp_out, _, ex = fm.grep_like(whole, find_all(whole, PATS), 1, 1, seg_start=starts, names=names, **full)
    assert data == exp_out and seg.tolist() == ex["seg_out"].tolist() and lines[:, 3].tolist() == [2, 1, 0, 2, 1, 2, 1, 0, 0, 1]
    with pytest.raises(ValueError):
        m.scan_format(texts=texts, names=names[:2], with_name=True)
    # only_matching: grep -o -n -b: the line and the offset of the match itself
    data, lines, at, info, seg = m.scan_format(texts=texts, names=names, only_matching=True, **full)
    assert data == b"t0:2:2:needle\nt1:3:4:hay\nt4:2:2:ne\nt4:5:9:hay\n" and lines[:, 0].tolist() == [2, 7, 10, 13]
    data = m.scan_format(t, only_matching=True, line_number=True)[0]
    sel = m.scan_select(t)
    assert data == b"".join(b"%d:" % (t.count(b"\n", 0, s) + 1) + t[s:o + 1] + b"\n" for s, o in zip(sel[2].tolist(), sel[0].tolist()))
    # an output that does not fit is an error
    with pytest.raises(AcmError) as e:
        m.scan_format(t, before=1, after=1, line_number=True, out_capacity=1000)
    assert e.value.code == _lib.ACM_ERR_CAPACITY
    m.close()
    w = small_matcher(PATS, 4096, wild=True)
    with pytest.raises(ValueError):
        w.scan_format(b"needle q.z\n", only_matching=True)
    assert w.scan_format(b"a\nneedle q.z\n", line_number=True)[0] == b"2:needle q.z\n"
    w.close()
