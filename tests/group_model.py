"""Groups of wildcard patterns in Python (test infrastructure only, not a conftest): the rule of
acm_automaton_add_wildcard_groups, the grammar of ACM_SIG_EXTENDED | ACM_SIG_GROUPS and a translation of a body
into Python's re, written from include/acmatch.h.  What groups do not change comes from wildcard_model.

A group is (at, strings, negated): the text bytes under positions [at, at + w) of the pattern equal one of the
strings of w bytes (negated: none).  The positions it covers carry the full set.

  Pattern            wildcard_model.Pattern with groups: holds() asks them too
  GroupModel         wildcard_model.WildcardModel whose verdict asks the groups where the context held
  parse_body_groups  the grammar with the groups bit: (parts, gaps, groups per part); BodyError names the column
  body_regex         the body as a regular expression, an independent statement of what it matches
  regex_ends         the offsets a body matches ending at, by re alone
"""
import re

import wildcard_model as wm
from sequence_model import BodyError, MAX_PARTS, UNB

MAX_WIDTH, MAX_ALTERNATIVES, MAX_GROUPS = 32, 256, 16
FULL = wm.FULL
DROP, KEEP, UNDECIDED = wm.DROP, wm.KEEP, wm.UNDECIDED


def group_holds(group, t, k):
    """does the group hold for a pattern whose first position is t[k]?"""
    at, strings, negated = group
    w = len(strings[0])
    return (bytes(t[k + at:k + at + w]) in [bytes(s) for s in strings]) != bool(negated)


class Pattern(wm.Pattern):
    def __init__(self, positions, groups=(), nocase=False):
        super().__init__(positions, nocase)
        self.groups = [(at, [bytes(s) for s in strings], bool(neg)) for at, strings, neg in groups]
        for at, strings, _ in self.groups:
            assert all(self.positions[at + i] == FULL for i in range(len(strings[0])))

    def holds(self, t, k):
        return super().holds(t, k) and all(group_holds(g, t, k) for g in self.groups)

    def context_holds(self, t, k):
        """the sets alone: what the pattern would be without its groups"""
        return super().holds(t, k)


class GroupModel(wm.WildcardModel):
    """pats: Patterns (of this module or of wildcard_model)"""

    def _verdict(self, p, o, t0, tend, known, full, lo):
        v = super()._verdict(p, o, t0, tend, known, full, lo)
        if v != KEEP:
            return v
        w = self.pats[p]
        first = o - w.L + 1 - w.pre
        return KEEP if all(group_holds(g, full, first - lo) for g in getattr(w, "groups", ())) else DROP

    def context_verdict(self, p, o, t0, tend, known, full, lo):
        return super()._verdict(p, o, t0, tend, known, full, lo)


# ---- the grammar with the groups bit

def parse_body_groups(body):
    """(parts, gaps, groups): parts and gaps as wildcard_model.parse_body_ex gives them (the positions a group
    covers are FULL), groups[j] the (at, strings, negated) of part j with the strings distinct, in order"""
    body = body.encode() if isinstance(body, str) else bytes(body)
    parts, gaps, groups, cur, cur_groups, cur_at, gap, k = [], [], [], [], [], 0, None, 0

    def close_part():
        if not any(len(s) == 1 for s in cur):
            raise BodyError(cur_at + 1)
        parts.append(list(cur))
        groups.append(list(cur_groups))

    while k < len(body):
        at, c = k, body[k:k + 1]
        new = None                       # the positions this token adds
        if body[k] in wm.HEX:
            if wm._hex2(body, k) is not None:
                new = [frozenset((wm._hex2(body, k),))]
            elif body[k + 1:k + 2] == b"?":
                new = [frozenset(int(c, 16) << 4 | x for x in range(16))]
            else:
                raise BodyError(at + 1)
            k += 2
        elif c == b"?":
            n = body[k + 1:k + 2]
            if n == b"?":
                new = [FULL]
            elif n and n in wm.HEX:
                new = [frozenset(x << 4 | int(n, 16) for x in range(16))]
            else:
                raise BodyError(at + 1)
            k += 2
        elif c in (b"(", b"!"):
            if c == b"!" and body[k + 1:k + 2] != b"(":
                raise BodyError(at + 1)
            k += 2 if c == b"!" else 1
            strings, width = [], None
            while True:
                alt_at, alt = k, bytearray()
                while wm._hex2(body, k) is not None:
                    alt.append(wm._hex2(body, k))
                    k += 2
                if not alt or (k < len(body) and body[k] in wm.HEX):
                    raise BodyError(k + 1)
                width = len(alt) if width is None else width
                if len(alt) != width:
                    raise BodyError(alt_at + 1)
                if bytes(alt) not in strings:
                    strings.append(bytes(alt))
                if body[k:k + 1] == b")":
                    break
                if body[k:k + 1] != b"|":
                    raise BodyError(k + 1)
                k += 1
            k += 1
            neg = c == b"!"
            if width == 1:
                listed = {s[0] for s in strings}
                new = [frozenset(listed) if not neg else FULL - listed]
                if not new[0]:
                    raise BodyError(at + 1)
            else:
                if width > MAX_WIDTH or len(strings) > MAX_ALTERNATIVES:
                    raise BodyError(at + 1)
                if not neg and len(strings) == 1:
                    new = [frozenset((b,)) for b in strings[0]]
                else:
                    if len(cur_groups) >= MAX_GROUPS:
                        raise BodyError(at + 1)
                    new = (len(cur), strings, neg)
        elif c == b"*":
            lo, hi, k = 0, None, k + 1
        elif c == b"{":
            r = wm._braces(body, k)
            if not r:
                raise BodyError(at + 1)
            lo, hi, k = r
        else:
            raise BodyError(at + 1)
        if new is not None:
            group = new if isinstance(new, tuple) else None
            added = [FULL] * len(group[1][0]) if group else new
            if not parts and not cur and not group and added[0] == FULL:
                raise BodyError(at + 1)
            if len(cur) + len(added) > wm.MAX_POSITIONS:
                raise BodyError(at + 1)
            if gap is not None:
                gaps.append(gap)
                gap = None
            if not cur:
                cur_at = at
            if group:
                cur_groups.append(group)
            cur += added
            last_any = not group and added[-1] == FULL
            continue
        if gap is None:
            if not cur:
                raise BodyError(at + 1)
            close_part()
            cur, cur_groups = [], []
            gap = (0, 0)
        gap = (gap[0] + lo, None if gap[1] is None or hi is None else gap[1] + hi)
        if max(gap[0], gap[1] or 0) >= UNB:
            raise BodyError(at + 1)
    if gap is not None or not cur or last_any:
        raise BodyError(len(body) + 1)
    close_part()
    if len(parts) > MAX_PARTS:
        raise BodyError(len(body) + 1)
    return parts, gaps, groups


def body_patterns(body, nocase=False):
    """(Patterns, gaps) of a body"""
    parts, gaps, groups = parse_body_groups(body)
    return [Pattern(p, g, nocase) for p, g in zip(parts, groups)], gaps


# ---- the body as a regular expression

ANY = b"[\\s\\S]"


def _x(b):
    return b"\\x%02x" % b


def body_regex(body):
    """the body for re (bytes): (aabb|ccdd) is (?:\\xaa\\xbb|\\xcc\\xdd), !(..) is (?!(?:..))[\\s\\S]{w}, a nibble
    wildcard a class, ?? [\\s\\S], * [\\s\\S]*, {n-m} [\\s\\S]{n,m}.  For bodies the grammar accepts."""
    body = body.encode() if isinstance(body, str) else bytes(body)
    out, k = [], 0
    while k < len(body):
        c = body[k:k + 1]
        if c in (b"(", b"!"):
            e = body.index(b")", k)
            alts = body[k + (2 if c == b"!" else 1):e].split(b"|")
            inner = b"(?:" + b"|".join(b"".join(_x(x) for x in bytes.fromhex(a.decode())) for a in alts) + b")"
            out.append(inner if c == b"(" else b"(?!" + inner + b")" + ANY + b"{%d}" % (len(alts[0]) // 2))
            k = e + 1
        elif c == b"*":
            out.append(ANY + b"*")
            k += 1
        elif c == b"{":
            lo, hi, k = wm._braces(body, k)
            out.append(ANY + b"{%d,%s}" % (lo, b"" if hi is None else b"%d" % hi))
        else:
            hi_, lo_ = body[k:k + 1], body[k + 1:k + 2]
            if hi_ == b"?" and lo_ == b"?":
                out.append(ANY)
            elif hi_ == b"?":
                out.append(b"[" + b"".join(_x(x << 4 | int(lo_, 16)) for x in range(16)) + b"]")
            elif lo_ == b"?":
                out.append(b"[" + b"".join(_x(int(hi_, 16) << 4 | x) for x in range(16)) + b"]")
            else:
                out.append(_x(int(body[k:k + 2], 16)))
            k += 2
    return b"".join(out)


def regex_ends(body, t):
    """the offsets of t at which a match of the body ends: some match of the expression ends there"""
    rx = re.compile(b"(?:" + body_regex(body) + b")\\Z")
    t = bytes(t)
    return [o for o in range(len(t)) if rx.search(t, 0, o + 1)]


def regex_starts(body, t):
    """the offsets at which a body without gaps matches (its span has one length)"""
    return [m.start() for m in re.finditer(b"(?=" + body_regex(body) + b")", bytes(t))]
