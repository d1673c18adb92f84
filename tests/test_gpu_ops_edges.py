"""The post-processing ops of csrc/post.hip through the C ABI (_lib), compared cell for cell with
tests/ops_model.py: exclusive scan, bucket compaction, bitonic sort, bucketize, chunk pack and offset remap.
Every device buffer is an ops_guard.Guarded one -- guard cells on both sides, poison where the op has not
written -- so a write one cell past the end, a defined cell left unwritten and a write into a cell the op
must leave alone all show.  tests/test_gpu_ops.py keeps the api.* wrapper tests, which zero and size their
outputs exactly."""
import numpy as np
import pytest

import fixtures
import ops_model as om
from gpu_pattern_matching_amd import Automaton, Matcher
from gpu_pattern_matching_amd._lib import check
from ops_guard import FILL32, WS_FILLS, Guarded, Workspace, same
from streams import Rig

pytestmark = pytest.mark.gpu

ACM_ERR_ARG = -1
TILE = 1024
FF, A5 = WS_FILLS          # poison.FILLS' bytes: 0xFF, 0xA5


# ------------------------------------------------------------------------------------------- 1 scan

SCAN_N = (1, 3, 1023, 1024, 1025, 2047, 2048, 2049, TILE * TILE - 1, TILE * TILE, TILE * TILE + 1, TILE * (TILE + 1) + 1)


def scan_inputs(n):
    """int32 in [-1000, 1000] (no sum leaves int32), and zeros with a 1 either side of a tile border"""
    a = np.random.default_rng(n).integers(-1000, 1001, size=n).astype(np.int32)
    b = np.zeros(n, dtype=np.int32)
    border = (n - 1) // TILE * TILE if n > TILE else 0      # the last border inside the array, if there is one
    for at in (border - 1, border):
        if 0 <= at < n:
            b[at] = 1
    return (("random", a), ("border", b))


def run_scan(lib, a, in_place, with_total, ws_fill, stream=None, ws_null=False, what=""):
    n = a.size
    exp, total = om.scan(a)
    d_in = Guarded(n, a)
    d_out = d_in if in_place else Guarded(n)
    d_tot = Guarded(1)
    wsb = lib.acm_exclusive_scan_workspace_bytes(n)
    ws = Workspace(wsb, ws_fill)
    check(lib.acm_exclusive_scan_i32(d_in.ptr, d_out.ptr, n, d_tot.ptr if with_total else None,
                                     None if ws_null else ws.ptr, 0 if ws_null else wsb, stream), "acm_exclusive_scan_i32")
    same(d_out.read(stream, what), exp, what)
    if not in_place:
        same(d_in.read(stream, what), a, what + " (input)")
    if with_total:
        assert int(d_tot.read(stream, what)[0]) == total, "%s: total" % what
    else:
        d_tot.untouched(stream, what + " (no total asked)")
    ws.check(stream, what)
    for b in {d_in, d_out, d_tot, ws}:
        b.free()


@pytest.mark.parametrize("n", SCAN_N)
def test_scan(gpu, lib, n):
    for name, a in scan_inputs(n):
        assert abs(om.scan(a)[0]).max(initial=0) < 2 ** 31 and abs(om.scan(a)[1]) < 2 ** 31
        for in_place, with_total, fill in ((False, True, FF), (True, True, A5), (False, False, A5), (True, False, FF)):
            run_scan(lib, a, in_place, with_total, fill,
                     what="n %d %s %s total %d workspace %#x" % (n, name, "in place" if in_place else "out of place", with_total, fill))
        if n <= TILE:
            run_scan(lib, a, False, True, FF, ws_null=True, what="n %d %s no workspace" % (n, name))


def test_scan_short_workspace_writes_nothing(gpu, lib):
    n = 1025
    a = scan_inputs(n)[0][1]
    d_in, d_out, d_tot = Guarded(n, a), Guarded(n), Guarded(1)
    wsb = lib.acm_exclusive_scan_workspace_bytes(n)
    ws = Workspace(wsb, 0xA5)
    assert lib.acm_exclusive_scan_i32(d_in.ptr, d_out.ptr, n, d_tot.ptr, ws.ptr, wsb - 1, None) == ACM_ERR_ARG
    assert lib.acm_exclusive_scan_i32(d_in.ptr, d_out.ptr, n, d_tot.ptr, None, 0, None) == ACM_ERR_ARG
    d_out.untouched(what="short workspace: d_out")
    d_tot.untouched(what="short workspace: d_total")
    assert np.all(ws.buf.to_numpy(np.uint8, wsb + Workspace.TAIL) == 0xA5), "short workspace: the workspace was written"
    for b in (d_in, d_out, d_tot, ws):
        b.free()


def test_scan_of_nothing(gpu, lib):
    d_out, d_tot = Guarded(4), Guarded(1)
    check(lib.acm_exclusive_scan_i32(d_out.ptr, d_out.ptr, 0, d_tot.ptr, None, 0, None), "acm_exclusive_scan_i32")
    assert int(d_tot.read()[0]) == 0
    d_out.untouched(what="n 0: d_out")
    check(lib.acm_exclusive_scan_i32(None, None, 0, None, None, 0, None), "acm_exclusive_scan_i32")
    d_out.free(), d_tot.free()


def test_scan_feeds_a_scan_on_a_created_stream(gpu, lib):
    """two multi-level scans back to back on one created stream, the second reading what the first writes
    (through one workspace): nothing but stream order between them"""
    n = TILE * TILE + 1
    v = np.random.default_rng(5).integers(-500, 501, size=n + 1)
    a = (v[1:] - v[:-1]).astype(np.int32)            # in [-1000, 1000]; its sums stay within +-1000
    first, t1 = om.scan(a)
    second, t2 = om.scan(first)
    assert abs(second).max() < 2 ** 31 and abs(t2) < 2 ** 31
    rig = Rig()
    s = rig.stream()
    d_in, d_mid, d_out, d_t1, d_t2 = Guarded(n, a), Guarded(n), Guarded(n), Guarded(1), Guarded(1)
    wsb = lib.acm_exclusive_scan_workspace_bytes(n)
    ws = Workspace(wsb, 0xA5)
    check(lib.acm_exclusive_scan_i32(d_in.ptr, d_mid.ptr, n, d_t1.ptr, ws.ptr, wsb, s), "acm_exclusive_scan_i32")
    check(lib.acm_exclusive_scan_i32(d_mid.ptr, d_out.ptr, n, d_t2.ptr, ws.ptr, wsb, s), "acm_exclusive_scan_i32")
    same(d_out.read(s, "second"), second, "second scan")
    same(d_mid.read(s, "first"), first, "first scan")
    assert int(d_t1.read(s)[0]) == t1 and int(d_t2.read(s)[0]) == t2
    ws.check(s, "chained scans")
    for b in (d_in, d_mid, d_out, d_t1, d_t2, ws):
        b.free()
    rig.close()


# ------------------------------------------------------------------------------------- 2 compaction

def bucket_planes(length, R, seed, overflow):
    """bucket planes [R][length] + trailer: counts below R, or up to R + 2 with overflow (Q14)"""
    rng = np.random.default_rng(seed)
    src = rng.integers(1000, 2000, size=R * length + 1).astype(np.int32)
    src[:length] = rng.integers(0, R + 3 if overflow else max(R, 1), size=length)
    if R == 1:
        src[:length] = rng.integers(0, 3, size=length)     # counted, but a plane of one row has no cell for them
    src[R * length] = 31337
    return src, om.scan(src[:length])[0].astype(np.int32)


def run_compact(lib, src, prefix, length, R, what, stream=None):
    total = int(src[:length].astype(np.int64).sum())
    room = total + 2 + 37
    d_src, d_pre, d_dst = Guarded(src.size, src), Guarded(length, prefix), Guarded(room)
    check(lib.acm_compact_buckets(d_dst.ptr, d_src.ptr, d_pre.ptr, length, R, stream), "acm_compact_buckets")
    got = d_dst.read(stream, what)
    exp = om.compact(src, prefix, length, R, room, FILL32)
    same(got, exp, what)
    assert got[0] == total and got[total + 1] == 31337 and np.all(got[total + 2:] == FILL32), what
    same(d_src.read(stream, what), src, what + " (src)")
    for b in (d_src, d_pre, d_dst):
        b.free()
    return got


@pytest.mark.parametrize("length,R", [(1, 1), (1, 2), (255, 3), (256, 3), (257, 3), (1000, 1)])
def test_compact_buckets(gpu, lib, length, R):
    for overflow in (False, True):
        src, prefix = bucket_planes(length, R, 7 * length + R, overflow)
        if length == 1 and R == 2:
            src[0] = 3 if overflow else 1
        got = run_compact(lib, src, prefix, length, R, "len %d max_results %d overflow %d" % (length, R, overflow))
        total = int(got[0])
        holes = int(np.maximum(src[:length] - (R - 1), 0).sum())
        assert int((got[1:total + 1] == FILL32).sum()) == holes      # Q14's holes still hold the poison
        if R == 1:
            assert holes == total          # only dst[0] and the trailer are written
        elif overflow:
            assert holes > 0
        else:
            assert holes == 0 and np.all(got[1:total + 1] >= 1000)


def test_compact_buckets_overflowing_chunk_leaves_poison(gpu, lib):
    """test_gpu_ops.test_compact_buckets_overflowing_chunk's planes, with a dst that is not zeroed"""
    chunks, R = 8, 4
    src = np.zeros(R * chunks + 1, dtype=np.int32)
    src[:chunks] = [1, 9, 0, 2, 3, 0, 7, 1]
    for i in range(chunks):
        for j in range(min(src[i], R - 1)):
            src[(j + 1) * chunks + i] = 100 * i + j
    src[R * chunks] = 31337
    rig = Rig()
    got = run_compact(lib, src, om.scan(src[:chunks])[0].astype(np.int32), chunks, R, "Q14", stream=rig.stream())
    rig.close()
    assert got[:8].tolist() == [23, 0, 100, 101, 102] + [FILL32] * 3 and int((got[1:24] == FILL32).sum()) == 6 + 4


# ------------------------------------------------------------------------------------------- 3 sort

SORT_SHAPES = ((2, 1), (2, 3), (8, 3), (64, 33), (64, 100), (512, 5), (1024, 3), (2048, 3), (4096, 2), (8192, 1))
PER_ARRAY = {(2, 1), (2, 3), (8, 3), (64, 33), (64, 100)}     # batch * len is no multiple of 512


def run_sort(lib, k, v, batch, length, direction, in_place, stream=None, what=""):
    ek, ev, which = om.sort(k, v, batch, length, direction)
    # PER_ARRAY shapes: the oracle has the ocl_ wrapper's batch * len % 512 rule, so it sorts them array by
    # array at a batch the rule allows (ops_model.sort); every other shape is one batched oracle call
    assert which == ("per-array" if (length, batch) in PER_ARRAY else "batched")
    n = k.size
    ks, vs = Guarded(n, k, dtype=np.uint32), Guarded(n, v, dtype=np.uint32)
    kd, vd = (ks, vs) if in_place else (Guarded(n, dtype=np.uint32), Guarded(n, dtype=np.uint32))
    assert lib.acm_bitonic_sort_u32(kd.ptr, vd.ptr, ks.ptr, vs.ptr, batch, length, direction, stream) == 0
    same(kd.read(stream, what), ek, what + " keys")
    same(vd.read(stream, what), ev, what + " values")
    if not in_place:
        same(ks.read(stream, what), k, what + " (key src)")
        same(vs.read(stream, what), v, what + " (value src)")
    for b in {ks, vs, kd, vd}:
        b.free()


@pytest.mark.parametrize("length,batch", SORT_SHAPES)
def test_bitonic_sort(gpu, lib, length, batch):
    k = om.sort_keys(batch * length, 31 * length + batch)
    if k.size >= 64:
        assert set(om.SPECIAL_KEYS) <= set(k.tolist())
    else:
        k[:] = np.resize(np.array(om.SPECIAL_KEYS, dtype=np.uint32), k.size)[::-1]
    v = np.arange(k.size, dtype=np.uint32)
    for direction in (0, 1):
        for in_place in (False, True):
            run_sort(lib, k, v, batch, length, direction, in_place,
                     what="len %d batch %d dir %d %s" % (length, batch, direction, "in place" if in_place else "out of place"))


def test_bitonic_sort_on_a_created_stream(gpu, lib):
    rig = Rig()
    s = rig.stream()
    k = om.sort_keys(2 * 4096, 3)
    v = np.arange(k.size, dtype=np.uint32)
    run_sort(lib, k, v, 2, 4096, 1, False, stream=s, what="len 4096 batch 2 on a stream")
    run_sort(lib, k, v, 2, 4096, 0, True, stream=s, what="len 4096 batch 2 on a stream, in place")
    rig.close()


def test_bitonic_sort_nothing_to_sort(gpu, lib):
    k = Guarded(8, np.arange(8), dtype=np.uint32)
    kd, vd = Guarded(8, dtype=np.uint32), Guarded(8, dtype=np.uint32)
    for batch, length in ((1, 1), (8, 1), (3, 0), (0, 8), (0, 2)):
        assert lib.acm_bitonic_sort_u32(kd.ptr, vd.ptr, k.ptr, k.ptr, batch, length, 1, None) == 0
    kd.untouched(what="nothing to sort: keys")
    vd.untouched(what="nothing to sort: values")
    for b in (k, kd, vd):
        b.free()


# -------------------------------------------------------------------------------------- 4 bucketize

LAST = 4242


def run_bucketize(lib, pats, offs, last, cap, ind, siz, R, what, stream=None):
    """planes of `cap` cells (in buffers of exactly that many) holding pats/offs and the trailer `last`"""
    chunks = ind.size
    pp, op = om.plane(pats, last, cap), om.plane(offs, last, cap)
    d_pp, d_op = Guarded(cap, pp), Guarded(cap, op)
    d_ind, d_siz = Guarded(chunks, ind), Guarded(chunks, siz)
    d_r, d_r2 = Guarded(R * chunks + 1 + 5), Guarded(R * chunks + 1 + 5)
    check(lib.acm_bucketize(d_pp.ptr, d_op.ptr, d_ind.ptr, d_siz.ptr, chunks, R, d_r.ptr, d_r2.ptr, cap, stream), "acm_bucketize")
    r, r2 = d_r.read(stream, what), d_r2.read(stream, what)
    er, er2 = om.bucketize(pp, op, cap, ind, siz, R, FILL32)
    assert np.all(r[R * chunks + 1:] == FILL32) and np.all(r2[R * chunks + 1:] == FILL32), "%s: a cell behind the trailer was written" % what
    same(r[:R * chunks + 1], er, what + " results")
    same(r2[:R * chunks + 1], er2, what + " results2")
    assert r[R * chunks] == last and r2[R * chunks] == last, "%s: trailer" % what
    for b in (d_pp, d_op, d_ind, d_siz, d_r, d_r2):
        b.free()
    return r


@pytest.mark.parametrize("chunks", [1, 255, 256, 257])
@pytest.mark.parametrize("R", [1, 4])
def test_bucketize(gpu, lib, chunks, R):
    ind, siz, _ = om.chunk_list(chunks, chunks + R, first=1000 if chunks == 1 else None)
    offs = om.edge_records(ind, siz, R, 5, always=chunks == 1)
    pats = (np.arange(offs.size) + 100).astype(np.int32)
    m = offs.size
    if chunks > 1:
        per = np.searchsorted(offs, ind + siz) - np.searchsorted(offs, ind)
        assert np.any(siz == 0) and np.any(np.diff(ind) > siz[:-1]) and 0 in per[siz > 0]
        if R == 4:
            assert (R - 1) in per and R in per and (R + 1) in per
    assert set(ind[siz > 0]) & set(offs.tolist()) and set((ind + siz - 1)[siz > 0]) & set(offs.tolist())
    # roomy; count = cap - 2; count = cap - 1; count far above cap.  The trailer of a capped plane is the
    # offset of the first record that found no cell: taken for a record, it lands in a chunk
    for cap in (m + 9, m + 2, m + 1, max(2, m // 4), 2):
        last = int(offs[cap - 2]) if cap - 2 < m else LAST
        r = run_bucketize(lib, pats, offs, last, cap, ind, siz, R, "chunks %d max_results %d count %d cap %d" % (chunks, R, m, cap))
        assert int(r[:chunks].sum()) == min(m, cap - 2)
    rig = Rig()
    for cap in (2, 9):
        r = run_bucketize(lib, pats[:0], offs[:0], LAST, cap, ind, siz, R, "chunks %d empty plane cap %d" % (chunks, cap), stream=rig.stream())
        assert np.all(r[:chunks] == 0) and np.all(r[chunks:R * chunks] == FILL32)
    rig.close()


# ---------------------------------------------------------------------------------- 5 pack and remap

def run_pack(lib, ind, siz, buf, what, stream=None):
    chunks, total = ind.size, int(siz.sum())
    st = om.starts(siz)
    d_src = Guarded(buf.size, buf, fill=om.GAP_BYTE, dtype=np.uint8)
    d_ind, d_siz, d_st = Guarded(chunks, ind), Guarded(chunks, siz), Guarded(chunks, st)
    d_dst = Guarded(total + 100, dtype=np.uint8)
    check(lib.acm_pack_chunks(d_dst.ptr, d_src.ptr, d_ind.ptr, d_siz.ptr, d_st.ptr, chunks, stream), "acm_pack_chunks")
    got = d_dst.read(stream, what)
    same(got[:total], om.pack(buf, ind, siz), what)
    assert np.all(got[total:] == 0x5A), "%s: a byte behind the packed stream was written" % what
    assert om.GAP_BYTE not in got
    for b in (d_src, d_ind, d_siz, d_st, d_dst):
        b.free()


@pytest.mark.parametrize("chunks", [1, 300])
def test_pack_chunks(gpu, lib, chunks):
    rig = Rig()
    for first in ((1000, 257, 1, 0) if chunks == 1 else (None,)):
        ind, siz, buf = om.chunk_list(chunks, chunks, first=first)
        assert ind[0] % 2 == 1 and (chunks == 1 or set(om.PACK_SIZES) == set(siz.tolist()))
        run_pack(lib, ind, siz, buf, "chunks %d first %s" % (chunks, first))
        run_pack(lib, ind, siz, buf, "chunks %d first %s on a stream" % (chunks, first), stream=rig.stream())
    rig.close()


def run_remap(lib, pl, room, ind, st, max_records, what, stream=None):
    d_pl = Guarded(room, pl)
    d_ind, d_st = Guarded(ind.size, ind), Guarded(st.size, st)
    check(lib.acm_remap_offsets(d_pl.ptr, max_records, d_ind.ptr, d_st.ptr, ind.size, stream), "acm_remap_offsets")
    exp = np.full(room, FILL32, dtype=np.int32)
    exp[:pl.size] = om.remap(pl, ind, st, max_records)
    same(d_pl.read(stream, what), exp, what)
    for b in (d_pl, d_ind, d_st):
        b.free()
    return exp


@pytest.mark.parametrize("chunks", [1, 300])
def test_remap_offsets(gpu, lib, chunks):
    ind, siz, buf = om.chunk_list(chunks, chunks, first=257 if chunks == 1 else None)
    st = om.starts(siz)
    full = siz > 0
    if chunks > 1:
        assert np.any((siz[1:-1] == 0) & (siz[:-2] > 0) & (siz[2:] > 0))      # empty chunks between non-empty ones
    # a record on the first and on the last byte of every non-empty chunk, as offsets of the packed stream
    offs = np.unique(np.concatenate([st[full], (st + siz - 1)[full]])).astype(np.int32)
    m = offs.size
    pl = om.plane(offs, LAST, m + 2)
    rig = Rig()
    for max_records, s in ((m, None), (m + 1000, rig.stream()), (m - 1, None), (m // 2, rig.stream()), (1, None), (0, None)):
        exp = run_remap(lib, pl, m + 2 + 9, ind, st, max_records, "chunks %d count %d max_records %d" % (chunks, m, max_records), stream=s)
        k = min(m, max_records)
        assert np.array_equal(exp[1 + k:m + 2], pl[1 + k:]) and exp[m + 1] == LAST
        if k == m:
            firsts, lasts = set(ind[full].tolist()), set((ind + siz - 1)[full].tolist())
            assert set(exp[1:1 + m].tolist()) == firsts | lasts
            assert np.all(buf[exp[1:1 + m]] != om.GAP_BYTE)
    run_remap(lib, om.plane([], LAST, 2), 2 + 9, ind, st, 1000, "chunks %d count 0" % chunks)
    # a capped plane: the count cell says more than the cells hold, max_records = cells - 2 keeps the trailer
    capped = om.plane(offs, LAST, m + 1) if m > 1 else None
    if capped is not None:
        run_remap(lib, capped, m + 1 + 9, ind, st, m - 1, "chunks %d capped plane" % chunks)
    rig.close()


def sentiment():
    path, hx, ml = fixtures.set_source("sentiment")
    a = Automaton()
    a.load_file(path, hx, ml)
    a.compile()
    m = Matcher(a, 0, max_text=16, plane_capacity=2)
    a.close()
    return m, fixtures.oracle_for("sentiment")


def test_pack_scan_remap_bucketize_on_one_stream(gpu, lib):
    """what ocl_aho_match enqueues for a padded chunk list, on a created stream with no host sync inside:
    64 KiB of text in 1000-byte chunks with 24-byte gaps (four trips of the copy loop per chunk), compared
    with the serial scan of the chunk stream walked into buckets (test_gpu_compat_api.expected_bucket_walk)"""
    m, o = sentiment()
    n, B, gap, R = 64 * 1024, 1000, 24, 8
    text = fixtures.text_for({"kind": "words", "n": n, "seed": 11}, None)
    chunks = (n + B - 1) // B
    siz = np.full(chunks, B, dtype=np.int32)
    siz[-1] = n - B * (chunks - 1)
    ind = (7 + np.arange(chunks) * (B + gap)).astype(np.int32)
    st = om.starts(siz)
    word = max(fixtures.patterns_of("sentiment")[:50], key=len)
    for end in (st[3], st[5] - 1):                 # a match on the first byte of chunk 3 and on the last of chunk 4
        text[end + 1 - len(word):end + 1] = np.frombuffer(word, dtype=np.uint8)
    buf = np.full(int(ind[-1] + siz[-1]) + gap, ord("a"), dtype=np.uint8)     # gaps of letters: scanned, they would show
    for i, s, p in zip(ind, siz, st):
        buf[i:i + s] = text[p:p + s]
    pos, pat, last = o.scan(text)
    which = np.searchsorted(st, pos.astype(np.int64), side="right") - 1
    buf_pos = (ind[which] + (pos.astype(np.int64) - st[which])).astype(np.int32)
    assert pos.size > 1000 and ind[3] in buf_pos and ind[4] + B - 1 in buf_pos and np.bincount(which).max() > R - 1
    cap = n + 2
    er, er2 = om.bucketize(om.plane(pat, last, cap), om.plane(buf_pos, last, cap), cap, ind, siz, R, FILL32)

    rig = Rig()
    s = rig.stream()
    d_src = Guarded(buf.size, buf, fill=ord("a"), dtype=np.uint8)
    d_ind, d_siz, d_st = Guarded(chunks, ind), Guarded(chunks, siz), Guarded(chunks, st)
    d_text = Guarded(n, dtype=np.uint8)             # (the scan may read the 16-byte pad behind n: guard bytes)
    d_pp, d_op = Guarded(cap), Guarded(cap)
    d_r, d_r2 = Guarded(R * chunks + 1), Guarded(R * chunks + 1)
    wsb = lib.acm_scan_workspace_bytes(m.dfa, n)
    ws = Workspace(wsb, 0xA5)
    check(lib.acm_pack_chunks(d_text.ptr, d_src.ptr, d_ind.ptr, d_siz.ptr, d_st.ptr, chunks, s), "acm_pack_chunks")
    m.scan_async(d_text.ptr, n, stream=s, pat_plane=d_pp.ptr, off_plane=d_op.ptr, plane_capacity=cap, workspace=(ws.ptr, wsb))
    check(lib.acm_remap_offsets(d_op.ptr, n, d_ind.ptr, d_st.ptr, chunks, s), "acm_remap_offsets")
    check(lib.acm_bucketize(d_pp.ptr, d_op.ptr, d_ind.ptr, d_siz.ptr, chunks, R, d_r.ptr, d_r2.ptr, cap, s), "acm_bucketize")
    same(d_r.read(s, "results"), er, "results")
    same(d_r2.read(s, "results2"), er2, "results2")
    same(d_text.read(s, "packed text"), text, "packed text")
    op = d_op.read(s, "offset plane")
    same(op[:pos.size + 2], om.plane(buf_pos, last, cap), "remapped offset plane")
    assert np.all(op[pos.size + 2:] == FILL32)
    ws.check(s, "scan workspace")
    for b in (d_src, d_ind, d_siz, d_st, d_text, d_pp, d_op, d_r, d_r2, ws):
        b.free()
    rig.close()
