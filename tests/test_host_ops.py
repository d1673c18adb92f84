"""tests/ops_model.py pinned on the host: each numpy model against a loop over single cells, and against
the oracle library where it has the op.  tests/test_gpu_ops_edges.py compares the device with the models."""
import numpy as np
import pytest

import ops_model as om
import orc
import poison

P = poison.cell(0x5A)


def test_scan_is_the_running_sum():
    rng = np.random.default_rng(1)
    for n in (1, 2, 1025, 5000):
        a = rng.integers(-1000, 1001, size=n).astype(np.int32)
        out, total = om.scan(a)
        acc, loop = 0, []
        for x in a.tolist():
            loop.append(acc)
            acc += x
        assert out.tolist() == loop and total == acc
        assert np.array_equal(out.astype(np.int32), orc.exclusive_scan(a))
    assert om.scan(np.zeros(0, np.int32))[1] == 0


def compact_loop(src, prefix, length, R, cells, fill):
    dst = [fill] * cells
    total = int(prefix[length - 1] + src[length - 1])
    dst[0] = total
    dst[total + 1] = int(src[R * length])
    for g in range(length):
        for i in range(min(int(src[g]), R - 1)):
            dst[int(prefix[g]) + 1 + i] = int(src[length * (i + 1) + g])
    return dst


def bucket_planes(length, R, seed, overflow):
    """bucket planes [R][length] + trailer: counts below R, or up to R + 2 with overflow (Q14)"""
    rng = np.random.default_rng(seed)
    src = rng.integers(1000, 2000, size=R * length + 1).astype(np.int32)
    src[:length] = rng.integers(0, R + 3 if overflow else max(R, 1), size=length)
    src[R * length] = 31337
    return src, om.scan(src[:length])[0].astype(np.int32)


@pytest.mark.parametrize("length,R", [(1, 1), (1, 2), (8, 4), (257, 3), (1000, 1)])
@pytest.mark.parametrize("overflow", [False, True])
def test_compact_model(length, R, overflow):
    src, prefix = bucket_planes(length, R, length + R, overflow)
    total = int(src[:length].sum())
    got = om.compact(src, prefix, length, R, total + 5, P)
    assert got.tolist() == compact_loop(src, prefix, length, R, total + 5, P)
    zero = om.compact(src, prefix, length, R, total + 5, 0)
    assert np.array_equal(zero, orc.compact_array(src, prefix, length, R, total + 5))
    assert got[0] == total and got[total + 1] == 31337 and np.all(got[total + 2:] == P)
    holes = int(np.maximum(src[:length] - (R - 1), 0).sum())
    assert int((got[1:total + 1] == P).sum()) == holes
    assert holes > 0 if overflow and length > 1 else holes == 0 or R == 1 or overflow


def test_sort_model_per_array_is_the_batched_network():
    """where the oracle takes the shape whole, the per-array form gives the same cells"""
    for length, batch in ((2, 256), (64, 16), (512, 3)):
        k = om.sort_keys(batch * length, length)
        v = np.arange(k.size, dtype=np.uint32)
        for d in (0, 1):
            ek, ev, which = om.sort(k, v, batch, length, d)
            assert which == "batched"
            for b in range(batch):
                sl = slice(b * length, (b + 1) * length)
                pk, pv, w = om.sort(k[sl], v[sl], 1, length, d)
                assert w == ("per-array" if length < 512 else "batched")
                assert np.array_equal(pk, ek[sl]) and np.array_equal(pv, ev[sl])
            seg = ek.reshape(batch, length).astype(np.int64)
            assert np.all(np.diff(seg, axis=1) >= 0) if d else np.all(np.diff(seg, axis=1) <= 0)
            assert np.array_equal(k[ev], ek)
    assert set(om.SPECIAL_KEYS) <= set(om.sort_keys(4096, 0).tolist())


def bucketize_loop(pat_plane, off_plane, cap, indices, sizes, R, fill):
    chunks = len(indices)
    res, res2 = [fill] * (R * chunks + 1), [fill] * (R * chunks + 1)
    full = int(pat_plane[0])
    stored = min(full, cap - 2)
    for i in range(chunks):
        cnt = 0
        for r in range(stored):
            if indices[i] <= off_plane[1 + r] < indices[i] + sizes[i]:
                cnt += 1
                if cnt < R:
                    res[cnt * chunks + i], res2[cnt * chunks + i] = int(pat_plane[1 + r]), int(off_plane[1 + r])
        res[i] = res2[i] = cnt
    res[R * chunks] = res2[R * chunks] = int(pat_plane[min(full + 1, cap - 1)])
    return res, res2


@pytest.mark.parametrize("chunks,R", [(1, 1), (1, 4), (40, 1), (40, 4), (257, 4)])
def test_bucketize_model(chunks, R):
    ind, siz, _ = om.chunk_list(chunks, chunks + R, first=1000 if chunks == 1 else None)
    offs = om.edge_records(ind, siz, R, 5, always=chunks == 1)
    pats = (np.arange(offs.size) + 100).astype(np.int32)
    m = offs.size
    assert m > 0
    if R >= 3 and chunks > 1:
        per = np.searchsorted(offs, ind + siz) - np.searchsorted(offs, ind)
        assert (R - 1) in per and R in per and 0 in per[siz > 0] and (R + 1) in per
    assert set(ind[siz > 0]) & set(offs.tolist()) and set((ind + siz - 1)[siz > 0]) & set(offs.tolist())
    for cap in (m + 9, m + 2, m + 1, max(2, m // 4), 2):
        pp, op = om.plane(pats, 4242, cap), om.plane(offs, 4242, cap)
        assert pp.size == min(m + 2, cap)
        r, r2 = om.bucketize(pp, op, cap, ind, siz, R, P)
        lr, lr2 = bucketize_loop(pp, op, cap, ind, siz, R, P)
        assert r.tolist() == lr and r2.tolist() == lr2
        assert r[R * chunks] == 4242 and r2[R * chunks] == 4242
        if cap >= m + 2:    # the oracle knows no capped plane; it leaves res2's trailer alone
            er, er2 = orc.bucketize(offs.astype(np.uint32), pats, ind, siz, R, 4242)
            defined = r != P
            assert np.array_equal(r[defined], er[defined]) and np.array_equal(r2[defined][:-1], er2[defined][:-1])
            assert np.all(er[~defined] == 0)
    empty = om.bucketize(om.plane([], 7, 5), om.plane([], 7, 5), 5, ind, siz, R, P)
    assert np.all(empty[0][:chunks] == 0) and empty[0][R * chunks] == 7 and np.all(empty[0][chunks:R * chunks] == P)


def test_pack_and_remap_models():
    for count in (1, 300):
        ind, siz, buf = om.chunk_list(count, count, first=257 if count == 1 else None)
        st = om.starts(siz)
        packed = om.pack(buf, ind, siz)
        assert packed.size == int(siz.sum()) and om.GAP_BYTE not in packed and ind[0] % 2 == 1
        loop = bytearray()
        for i, s in zip(ind.tolist(), siz.tolist()):
            for k in range(s):
                loop.append(buf[i + k])
        assert packed.tobytes() == bytes(loop)
        if count > 1:
            assert np.any(siz == 0) and np.any(np.diff(ind) > siz[:-1]) and np.any(ind % 16)
            empties_between = np.flatnonzero((siz[1:-1] == 0) & (siz[:-2] > 0) & (siz[2:] > 0))
            assert empties_between.size
        # a record on every byte of the packed stream maps back to the byte it was packed from
        every = np.arange(packed.size, dtype=np.int32)
        pl = om.plane(every, 99, packed.size + 2)
        back = om.remap(pl, ind, st, packed.size)
        assert back[0] == packed.size and back[-1] == 99
        assert np.array_equal(buf[back[1:-1]], packed)
        for r in (0, packed.size // 2, packed.size - 1):
            c = max(i for i in range(count) if st[i] <= r and siz[i] > 0)
            assert back[1 + r] == ind[c] + r - st[c]
        part = om.remap(pl, ind, st, 10)
        assert np.array_equal(part[1:11], back[1:11]) and np.array_equal(part[11:], pl[11:])
        assert np.array_equal(om.remap(pl, ind, st, 0), pl)
        assert np.array_equal(om.remap(om.plane([], 5, 4), ind, st, 100), [0, 5])
