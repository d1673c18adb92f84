"""Leftmost-longest non-overlapping selection in Python (test infrastructure only, not a conftest): the rule of
acm_select_matches_async, written from include/acmatch.h.

Entry (p, o) of pattern p (length L, wildcard context pre and post) spans [s, e] = [o - L + 1 - pre, o + post].  It
is eligible iff p is a pattern index, L >= 1 and s >= min_start.  Cursor c = min_start; among the eligible entries
with s >= c the smallest s, then the largest e, then the first in the input; emit it, c = e + 1, repeat.

  SelectModel   one serial sweep: every eligible entry is visited once, in (s, -e, input index) order, and taken
                iff it starts at or behind the cursor.  No successor function, no search, no doubling.
  brute_force   the rule word for word: every step looks at every entry again
  planes        the three planes a call must leave
"""
import numpy as np

import position_model as pm


class SelectModel:
    """pat_lens: the length of every pattern; pre, post: the wildcard context of every pattern (default: none)"""

    def __init__(self, pat_lens, pre=None, post=None):
        self.len = np.asarray(pat_lens, dtype=np.int64)
        self.pre = np.zeros_like(self.len) if pre is None else np.asarray(pre, dtype=np.int64)
        self.post = np.zeros_like(self.len) if post is None else np.asarray(post, dtype=np.int64)

    def spans(self, cells, offs, min_start=0):
        """(s, e, eligible, dropped) of every entry, whatever the cells hold"""
        cells = np.asarray(cells, dtype=np.int64)
        offs = np.asarray(offs, dtype=np.int64)
        valid = (cells >= 0) & (cells < self.len.size)
        p = np.where(valid, cells, 0)
        real = valid & (self.len[p] >= 1) if self.len.size else np.zeros(cells.size, dtype=bool)
        if not self.len.size:
            return offs, offs, real, real
        s = offs - self.len[p] + 1 - self.pre[p]
        e = offs + self.post[p]
        return s, e, real & (s >= min_start), real & (s < min_start)

    def run(self, cells, offs, min_start=0):
        """(patterns int32, offsets int64, starts int64, info[4]) the pass writes for the cells"""
        cells = np.asarray(cells, dtype=np.int64)
        offs = np.asarray(offs, dtype=np.int64)
        s, e, elig, dropped = self.spans(cells, offs, min_start)
        idx = np.flatnonzero(elig)
        order = idx[np.lexsort((idx, -e[idx], s[idx]))]
        cursor, chosen = int(min_start), []
        for i, si, ei in zip(order.tolist(), s[order].tolist(), e[order].tolist()):
            if si >= cursor:
                chosen.append(i)
                cursor = ei + 1
        chosen = np.asarray(chosen, dtype=np.int64)
        lo = cursor & 0xFFFFFFFF                                  # the cursor as the int32 pair (lo, hi)
        info = [int(elig.sum()), int(dropped.sum()), lo - (1 << 32) if lo >= 1 << 31 else lo, cursor >> 32]
        return cells[chosen].astype(np.int32), offs[chosen], s[chosen], info


def brute_force(cells, offs, lens, pre, post, min_start=0):
    """the indices of the selected entries: every step scans all entries for (smallest s, largest e, first)"""
    n, c, out = len(cells), min_start, []
    while True:
        pick = None
        for i in range(n):
            p = int(cells[i])
            if not (0 <= p < len(lens)) or lens[p] < 1:
                continue
            s = int(offs[i]) - lens[p] + 1 - pre[p]
            e = int(offs[i]) + post[p]
            if s < min_start or s < c:
                continue
            if pick is None or s < pick[0] or (s == pick[0] and e > pick[1]):
                pick = (s, e, i)
        if pick is None:
            return out
        out.append(pick[2])
        c = pick[1] + 1


def planes(pats, offs, starts, cap, poison, trailer):
    """the three planes of cap cells a call must leave: the pattern and offset planes as every pass leaves them,
    the start plane with trailer cell 0"""
    return pm.planes(pats, offs, cap, poison, trailer) + [pm.planes(starts, starts, cap, poison, 0)[0]]
