"""The post-processing ops of csrc/post.hip in plain numpy (a test helper, not a conftest): what every cell
of an output holds after a call, the cells the op leaves alone included -- `fill` is the int32 the output
held before.  tests/test_host_ops.py pins each against a loop over single cells and, where the oracle
library has the op, against orc.*.

  scan        np.cumsum in int64: (exclusive sums, total)
  compact     compactarray.cl cell for cell: count, cells in order, holes where a chunk counted more matches
              than it has cells, trailer
  sort        orc.bitonic_sort; where it refuses a shape acm_bitonic_sort_u32 takes (the batch * len % 512
              rule of the ocl_ wrapper), one call per array at a batch the rule allows
  plane       a compact plane of `cap` cells as the scan kernels write it: count, the records that fit,
              trailer (in the last cell when the plane is capped)
  bucketize   np.searchsorted over the stored records of a (possibly capped) plane pair
  pack        slicing; starts() the packed start of each chunk
  remap       np.searchsorted over the packed starts
"""
import numpy as np

import orc


def scan(a):
    a = np.asarray(a, dtype=np.int64)
    inc = np.cumsum(a)
    return inc - a, int(inc[-1]) if a.size else 0


def compact(src, prefix, length, max_results, cells, fill):
    src = np.asarray(src, dtype=np.int64)
    prefix = np.asarray(prefix, dtype=np.int64)
    dst = np.full(cells, fill, dtype=np.int64)
    total = int(prefix[length - 1] + src[length - 1])
    dst[0] = total
    dst[total + 1] = src[max_results * length]
    for i in range(max_results - 1):
        has = np.flatnonzero(src[:length] > i)
        dst[prefix[has] + 1 + i] = src[length * (i + 1) + has]
    return dst.astype(np.int32)


def sort(key, val, batch, length, direction):
    """(keys, values, which): which = "batched" (one orc.bitonic_sort call) or "per-array" """
    key = np.asarray(key, dtype=np.uint32)
    val = np.asarray(val, dtype=np.uint32)
    rc, k, v = orc.bitonic_sort(key, val, batch, length, direction)
    if rc == 0:
        return k, v, "batched"
    assert length <= 512 and (batch * length) % 512, "the oracle refuses this shape for another reason"
    rep = 512 // length          # the array `rep` times over: the sorts of a batch do not see each other
    k, v = key.copy(), val.copy()
    for b in range(batch):
        sl = slice(b * length, (b + 1) * length)
        rc, kk, vv = orc.bitonic_sort(np.tile(key[sl], rep), np.tile(val[sl], rep), rep, length, direction)
        assert rc == 0
        k[sl], v[sl] = kk[:length], vv[:length]
    return k, v, "per-array"


def plane(records, last, cap):
    records = np.asarray(records, dtype=np.int32)
    m = records.size
    assert cap >= 2
    stored = min(m, cap - 2)
    return np.concatenate([[m], records[:stored], [last]]).astype(np.int32)


def bucketize(pat_plane, off_plane, cap, indices, sizes, max_results, fill):
    pat_plane = np.asarray(pat_plane, dtype=np.int64)
    off_plane = np.asarray(off_plane, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    sizes = np.asarray(sizes, dtype=np.int64)
    chunks = indices.size
    full = int(pat_plane[0])
    m, tail = min(full, cap - 2), min(full + 1, cap - 1)
    offs = off_plane[1:1 + m]
    r0 = np.searchsorted(offs, indices, side="left")
    r1 = np.searchsorted(offs, indices + sizes, side="left")
    res = np.full(max_results * chunks + 1, fill, dtype=np.int64)
    res2 = res.copy()
    res[:chunks] = res2[:chunks] = r1 - r0
    for k in range(max_results - 1):
        has = np.flatnonzero(r1 - r0 > k)
        res[(k + 1) * chunks + has] = pat_plane[1 + r0[has] + k]
        res2[(k + 1) * chunks + has] = off_plane[1 + r0[has] + k]
    res[max_results * chunks] = res2[max_results * chunks] = pat_plane[tail]
    return res.astype(np.int32), res2.astype(np.int32)


def starts(sizes):
    sizes = np.asarray(sizes, dtype=np.int64)
    return (np.cumsum(sizes) - sizes).astype(np.int32)


def pack(src, indices, sizes):
    parts = [src[i:i + s] for i, s in zip(indices, sizes)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def remap(off_plane, indices, packed_start, max_records):
    out = np.array(off_plane, dtype=np.int32)
    m = min(int(out[0]), max_records)
    off = out[1:1 + m].astype(np.int64)
    c = np.searchsorted(np.asarray(packed_start, dtype=np.int64), off, side="right") - 1
    out[1:1 + m] = np.asarray(indices, dtype=np.int64)[c] + off - np.asarray(packed_start, dtype=np.int64)[c]
    return out


# ---------------------------------------------------------------------------------------------- inputs

SPECIAL_KEYS = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)
PACK_SIZES = (0, 1, 15, 16, 17, 255, 256, 257, 1000)
GAP_BYTE = 0xEE


def sort_keys(n, seed):
    """ties and both halves of the unsigned range: mostly SPECIAL_KEYS, a few random keys"""
    rng = np.random.default_rng(seed)
    k = np.array(SPECIAL_KEYS, dtype=np.uint32)[rng.integers(0, len(SPECIAL_KEYS), size=n)]
    some = rng.random(n) < 0.25
    k[some] = rng.integers(0, 1 << 32, size=int(some.sum()), dtype=np.uint64).astype(np.uint32)
    return k


def chunk_list(count, seed, sizes=PACK_SIZES, first=None):
    """(indices, sizes, buffer bytes): chunks of the given sizes at unaligned indices, empty ones and gaps
    of 0..7 bytes between them; the buffer holds GAP_BYTE outside the chunks and never inside one"""
    rng = np.random.default_rng(seed)
    siz = np.array(sizes, dtype=np.int32)[rng.integers(0, len(sizes), size=count)]
    if first is not None:
        siz[0] = first
    gaps = rng.integers(0, 8, size=count).astype(np.int32)
    gaps[0] |= 1
    ind = (np.cumsum(gaps + siz) - siz).astype(np.int32)
    buf = np.full(int(ind[-1] + siz[-1]) + 5, GAP_BYTE, dtype=np.uint8)
    for i, s in zip(ind, siz):
        buf[i:i + s] = rng.integers(0, GAP_BYTE, size=s, dtype=np.uint8)
    return ind, siz, buf


def edge_records(indices, sizes, max_results, seed, always=False):
    """sorted buffer offsets of the records of a chunk list: 0 .. max_results + 1 per chunk, in three chunks
    of four (always: in every one) on the first and on the last byte; with max_results >= 3 the first chunk of 8 bytes or more
    holds exactly max_results - 1 records and the next such chunk max_results"""
    rng = np.random.default_rng(seed)
    out, want = [], [max_results - 1, max_results]
    for i, s in zip(indices, sizes):
        if s == 0:
            continue
        pick = {0, s - 1} if always or rng.random() < 0.75 else set()
        n = max(int(rng.integers(0, max_results + 2)), len(pick))
        if s >= 8 and want and want[0] >= 2:
            pick, n = {0, s - 1}, want.pop(0)
        n = min(n, s)
        while len(pick) < n:
            pick.add(int(rng.integers(0, s)))
        out.extend(int(i) + p for p in sorted(pick))
    return np.array(out, dtype=np.int32)
