"""Thin Python front-end over the native boundary (acm_* in include/acmatch.h).

Used by tests/ and bench.py.  Everything that computes runs in libacmatch.so
on the GPU; this module only moves bytes and keeps handles alive.
"""
import contextlib
import ctypes as C

import numpy as np

from . import _lib
from ._lib import AcmError, check  # noqa: F401


def _ptr(x):
    """device pointer of a DeviceArray / int / torch tensor (has data_ptr)."""
    if x is None:
        return None
    if isinstance(x, DeviceArray):
        return x.ptr
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return int(x)


def class_map(values):
    """(labels, class_of) of one value per pattern: labels sorted and unique, class_of int32 with
    labels[class_of[i]] == values[i] -- what Matcher.scan_tally and acm_tally_matches_async take.
    class_map(np.sign(automaton.iids())) splits a categorical pattern file into negative / positive."""
    labels, inverse = np.unique(np.asarray(values), return_inverse=True)
    return labels, np.ascontiguousarray(inverse.reshape(-1), dtype=np.int32)


class DeviceArray:
    """A hipMalloc'ed block; numpy in, numpy out."""

    def __init__(self, nbytes, device=None):
        self.lib = _lib.load()
        if device is not None:
            check(self.lib.acm_rt_set_device(device), "acm_rt_set_device")
        p = C.c_void_p()
        check(self.lib.acm_rt_malloc(C.byref(p), nbytes), "acm_rt_malloc")
        self.ptr = p.value
        self.nbytes = nbytes

    @classmethod
    def from_numpy(cls, a, pad_to=16, stream=None):
        a = np.ascontiguousarray(a)
        nb = (a.nbytes + pad_to - 1) // pad_to * pad_to if pad_to else a.nbytes
        d = cls(max(nb, 16))
        if nb > a.nbytes:
            check(d.lib.acm_rt_memset(d.ptr + a.nbytes, 0, nb - a.nbytes, stream), "acm_rt_memset")
        if a.nbytes:
            check(d.lib.acm_rt_memcpy_h2d(d.ptr, a.ctypes.data, a.nbytes, stream), "acm_rt_memcpy_h2d")
        check(d.lib.acm_rt_stream_sync(stream), "acm_rt_stream_sync")
        return d

    def to_numpy(self, dtype, count, offset_bytes=0, stream=None):
        out = np.empty(count, dtype=dtype)
        if out.nbytes:
            check(self.lib.acm_rt_memcpy_d2h(out.ctypes.data, self.ptr + offset_bytes, out.nbytes,
                                             stream), "acm_rt_memcpy_d2h")
        check(self.lib.acm_rt_stream_sync(stream), "acm_rt_stream_sync")
        return out

    def fill(self, byte, stream=None):
        check(self.lib.acm_rt_memset(self.ptr, byte, self.nbytes, stream), "acm_rt_memset")

    def free(self):
        if self.ptr:
            self.lib.acm_rt_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Automaton:
    """Host automaton: patterns -> acsmx-compatible DFA (acm_automaton_*)."""

    def __init__(self, nocase=False):
        self.lib = _lib.load()
        self.h = self.lib.acm_automaton_new()
        if not self.h:
            raise MemoryError("acm_automaton_new")
        if nocase:
            self.set_nocase(True)

    def set_nocase(self, enable=True):
        """ASCII case-insensitive matching (acm_automaton_set_nocase); only before compile()."""
        check(self.lib.acm_automaton_set_nocase(self.h, int(bool(enable))), "acm_automaton_set_nocase")
        return self

    @property
    def nocase(self):
        return bool(self.lib.acm_automaton_nocase(self.h))

    def add(self, pattern: bytes, iid: int = 0, nocase: bool = False):
        """Append one pattern.  nocase: this pattern ignores ASCII case (acm_automaton_add_ex); an
        automaton with both kinds is mixed: its scans give candidates, Matcher.scan_case the matches."""
        if nocase:
            check(self.lib.acm_automaton_add_ex(self.h, pattern, len(pattern), iid, _lib.PATTERN_NOCASE),
                  "acm_automaton_add_ex")
        else:
            check(self.lib.acm_automaton_add(self.h, pattern, len(pattern), iid), "acm_automaton_add")

    def load_file(self, path, hex=False, max_len=-1, nocase=False):
        if nocase:
            n = self.lib.acm_automaton_load_file_ex(self.h, str(path).encode(), int(hex), int(max_len),
                                                    _lib.PATTERN_NOCASE)
        else:
            n = self.lib.acm_automaton_load_file(self.h, str(path).encode(), int(hex), int(max_len))
        if n < 0:
            check(n, "acm_automaton_load_file")
        return n

    def pattern_flags(self, i):
        """the flags pattern i was added with (acm_automaton_pattern_flags): _lib.PATTERN_NOCASE or 0"""
        f = self.lib.acm_automaton_pattern_flags(self.h, i)
        if f < 0:
            check(f, "acm_automaton_pattern_flags")
        return f

    @property
    def mixed_case(self):
        """compiled, and some patterns ignore case while others do not (acm_automaton_mixed_case)"""
        return bool(self.lib.acm_automaton_mixed_case(self.h))

    def set_position(self, i, lo=0, hi=None, from_end=False):
        """Where in its text pattern i may start (acm_automaton_set_position): lo <= start - text start <=
        hi, or with from_end lo <= text end - start <= hi; hi None: no upper bound.  Before or after
        compile(), but before the Matcher is made: the upload copies the windows."""
        check(self.lib.acm_automaton_set_position(self.h, i, lo, _lib.POS_UNBOUNDED if hi is None else hi,
                                                  _lib.POS_FROM_END if from_end else 0), "acm_automaton_set_position")

    def position(self, i):
        """(lo, hi or None, from_end) of pattern i (acm_automaton_pattern_position)"""
        lo, hi, fl = C.c_int32(), C.c_int32(), C.c_uint()
        check(self.lib.acm_automaton_pattern_position(self.h, i, C.byref(lo), C.byref(hi), C.byref(fl)),
              "acm_automaton_pattern_position")
        return lo.value, None if hi.value == _lib.POS_UNBOUNDED else hi.value, bool(fl.value & _lib.POS_FROM_END)

    @property
    def positioned(self):
        """some pattern has a position constraint (acm_automaton_positioned)"""
        return bool(self.lib.acm_automaton_positioned(self.h))

    def load_position_file(self, path):
        """constraints from a file of "<pattern index> <lo> <hi or *> [end]" lines; returns how many"""
        n = self.lib.acm_automaton_load_position_file(self.h, str(path).encode())
        if n < 0:
            check(n, "acm_automaton_load_position_file")
        return n

    def set_replacement(self, i, data=None, fill=None):
        """What a match of pattern i becomes in a rewrite (acm_automaton_set_replacement): data, bytes that take
        the place of the whole span (b"": the span is deleted), or fill, one byte (an int or bytes of length 1) that
        every byte of the span becomes.  Before or after compile(), but before the Matcher is made: the upload
        copies the replacements."""
        if (data is None) == (fill is None):
            raise ValueError("set_replacement takes data or fill")
        if fill is not None:
            b, flags = bytes([fill]) if isinstance(fill, int) else bytes(fill), _lib.REPL_FILL
        else:
            b, flags = bytes(data), 0
        check(self.lib.acm_automaton_set_replacement(self.h, i, b, len(b), flags), "acm_automaton_set_replacement")

    def clear_replacement(self, i):
        """back to the default: a match of pattern i is copied as it is (acm_automaton_clear_replacement)"""
        check(self.lib.acm_automaton_clear_replacement(self.h, i), "acm_automaton_clear_replacement")

    def replacement(self, i):
        """None when pattern i has no replacement, else (bytes, is_fill) as set (acm_automaton_pattern_replacement)"""
        p, n, fl = C.c_void_p(), C.c_int(), C.c_uint()
        rc = self.lib.acm_automaton_pattern_replacement(self.h, i, C.byref(p), C.byref(n), C.byref(fl))
        if rc < 0:
            check(rc, "acm_automaton_pattern_replacement")
        if rc == 0:
            return None
        return C.string_at(p.value, n.value) if n.value else b"", bool(fl.value & _lib.REPL_FILL)

    @property
    def has_replacements(self):
        """some pattern has a replacement (acm_automaton_has_replacements)"""
        return bool(self.lib.acm_automaton_has_replacements(self.h))

    def load_replacement_file(self, path):
        """replacements from a file of "<pattern index> <hex bytes or empty>" and "<pattern index> fill <hh>"
        lines; returns how many"""
        n = self.lib.acm_automaton_load_replacement_file(self.h, str(path).encode())
        if n < 0:
            check(n, "acm_automaton_load_replacement_file")
        return n

    def add_sequence(self, parts, gaps=(), iid=0):
        """An ordered multi-part signature (acm_automaton_add_sequence): parts are pattern indices, gaps one
        (lo, hi) per part but the first, the bytes between that part and the one in front; hi None: no upper
        bound.  Before or after compile(), but before the Matcher is made.  Returns the sequence index."""
        parts, gaps = list(parts), list(gaps)
        if len(gaps) != max(len(parts) - 1, 0):
            raise ValueError("%d parts need %d gaps, not %d" % (len(parts), max(len(parts) - 1, 0), len(gaps)))
        p = (C.c_int32 * max(len(parts), 1))(*parts)
        lo = (C.c_int32 * max(len(gaps), 1))(*[g[0] for g in gaps])
        hi = (C.c_int32 * max(len(gaps), 1))(*[_lib.GAP_UNBOUNDED if g[1] is None else g[1] for g in gaps])
        r = self.lib.acm_automaton_add_sequence(self.h, p, lo, hi, len(parts), iid)
        if r < 0:
            check(r, "acm_automaton_add_sequence")
        return r

    @staticmethod
    def _syntax(extended, groups):
        return _lib.SIG_EXTENDED | _lib.SIG_GROUPS if groups else _lib.SIG_EXTENDED if extended else 0

    def add_signature(self, body, iid=0, nocase=False, extended=False, groups=False):
        """A ClamAV-style hex body (acm_automaton_add_signature): hex byte pairs, ??, *, {n}, {n-m}, {-m}, {n-}.
        Adds its fixed parts as patterns and registers the sequence; only before compile().  extended
        (acm_automaton_add_signature_ex, ACM_SIG_EXTENDED): also a?, ?a, (aa|bb), !(aa|bb), ?? a position; the
        parts are wildcard patterns (add_wildcard).  groups (ACM_SIG_GROUPS, implies extended): also alternatives
        of more than one byte, (aabb|ccdd) and !(aabb|ccdd), all of one width.  Returns the sequence index."""
        body = body.encode() if isinstance(body, str) else bytes(body)
        fl = _lib.PATTERN_NOCASE if nocase else 0
        if extended or groups:
            r = self.lib.acm_automaton_add_signature_ex(self.h, body, iid, fl, self._syntax(extended, groups))
        else:
            r = self.lib.acm_automaton_add_signature(self.h, body, iid, fl)
        if r < 0:
            check(r, "acm_automaton_add_signature")
        return r

    def load_signature_file(self, path, nocase=False, extended=False, groups=False):
        """signatures from a file, one per line with an optional leading "<iid>:"; returns how many.  extended:
        the extended body syntax (acm_automaton_load_signature_file_ex); groups: with multi-byte alternatives"""
        fl = _lib.PATTERN_NOCASE if nocase else 0
        if extended or groups:
            n = self.lib.acm_automaton_load_signature_file_ex(self.h, str(path).encode(), fl,
                                                              self._syntax(extended, groups))
        else:
            n = self.lib.acm_automaton_load_signature_file(self.h, str(path).encode(), fl)
        if n < 0:
            check(n, "acm_automaton_load_signature_file")
        return n

    @staticmethod
    def byte_set(position):
        """the 32 bytes of set of one position: an int, bytes or an iterable of ints"""
        if isinstance(position, int):
            position = (position,)
        out = bytearray(32)
        for b in position:
            b = int(b)
            if not 0 <= b <= 255:
                raise ValueError("byte value %d" % b)
            out[b >> 3] |= 1 << (b & 7)
        return bytes(out)

    def add_wildcard(self, positions, iid=0, nocase=False, groups=()):
        """A wildcard pattern (acm_automaton_add_wildcard): every position a set of byte values, given as an int,
        bytes or an iterable of ints.  The longest run of one-byte positions, its anchor, enters the automaton
        (nocase applies to it alone); the positions around it are checked by Matcher.scan_wildcards.  Only before
        compile().  groups (acm_automaton_add_wildcard_groups): (at, strings, negated) triples, ascending and
        disjoint, strings of one width >= 2; the text under positions [at, at + width), which all carry the full
        set, must equal one of the strings (negated: none).  Returns the pattern index."""
        sets = b"".join(self.byte_set(p) for p in positions)
        fl = _lib.PATTERN_NOCASE if nocase else 0
        groups = list(groups)
        if not groups:
            r = self.lib.acm_automaton_add_wildcard(self.h, sets, len(sets) // 32, iid, fl)
        else:
            arr, raw = (_lib.WildGroup * len(groups))(), []
            for k, (at, strings, negated) in enumerate(groups):
                strings = [bytes(x) for x in strings]
                if not strings or any(len(x) != len(strings[0]) for x in strings):
                    raise ValueError("group %d: the strings must be of one width, and at least one" % k)
                raw.append(b"".join(strings))   # (alive until the call returns)
                arr[k] = _lib.WildGroup(at, len(strings[0]), len(strings), 1 if negated else 0, raw[-1])
            r =self.lib.acm_automaton_add_wildcard_groups(self.h, sets, len(sets) // 32, arr, len(groups), iid, fl)
        if r < 0:
            check(r, "acm_automaton_add_wildcard")
        return r

    def wildcard_groups(self, i):
        """the groups of pattern i: a list of (at, strings, negated), at counted from the pattern's first position"""
        n = self.lib.acm_automaton_pattern_groups(self.h, i)
        if n < 0:
            check(n, "acm_automaton_pattern_groups")
        out = []
        for j in range(n):
            at, w, cnt, neg, ptr = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_void_p()
            check(self.lib.acm_automaton_pattern_group(self.h, i, j, C.byref(at), C.byref(w), C.byref(cnt), C.byref(neg),
                                                       C.byref(ptr)), "acm_automaton_pattern_group")
            raw = C.string_at(ptr.value, w.value * cnt.value)
            out.append((at.value, [raw[k * w.value:(k + 1) * w.value] for k in range(cnt.value)], bool(neg.value)))
        return out

    @property
    def has_groups(self):
        """some pattern has a group (acm_automaton_groups)"""
        return bool(self.lib.acm_automaton_groups(self.h))

    def wildcard(self, i):
        """(pre, post) of pattern i (acm_automaton_pattern_wildcard): the context positions in front of and behind
        its anchor, each a frozenset of byte values; two empty lists for a plain pattern"""
        pre, post, ps, qs = C.c_int32(), C.c_int32(), C.c_void_p(), C.c_void_p()
        r = self.lib.acm_automaton_pattern_wildcard(self.h, i, C.byref(pre), C.byref(post), C.byref(ps), C.byref(qs))
        if r < 0:
            check(r, "acm_automaton_pattern_wildcard")

        def sets(ptr, n):
            raw = C.string_at(ptr.value, 32 * n) if n else b""
            return [frozenset(b for b in range(256) if raw[32 * k + (b >> 3)] >> (b & 7) & 1) for k in range(n)]
        return sets(ps, pre.value), sets(qs, post.value)

    def wildcard_lengths(self, i):
        """(pre, post) of pattern i as counts"""
        pre, post = C.c_int32(), C.c_int32()
        r = self.lib.acm_automaton_pattern_wildcard(self.h, i, C.byref(pre), C.byref(post), None, None)
        if r < 0:
            check(r, "acm_automaton_pattern_wildcard")
        return pre.value, post.value

    @property
    def has_wildcards(self):
        """some pattern has a context (acm_automaton_wildcards)"""
        return bool(self.lib.acm_automaton_wildcards(self.h))

    @property
    def wildcard_reach(self):
        """(back, ahead) over the patterns with a context: the largest pre + anchor length, the largest post"""
        b, f = C.c_int32(), C.c_int32()
        check(self.lib.acm_automaton_wildcard_reach(self.h, C.byref(b), C.byref(f)), "acm_automaton_wildcard_reach")
        return b.value, f.value

    def add_approx(self, pattern: bytes, k: int, iid: int = 0, nocase: bool = False):
        """An approximate pattern (acm_automaton_add_approx): matches where at most k bytes differ.  Its k + 1 pieces
        enter the automaton as consecutive patterns; returns the index of piece 0 (k == 0: a plain add, the index of
        the new pattern).  nocase: the whole comparison folds ASCII case.  Only before compile(); the mismatches
        are counted by Matcher.scan_approx."""
        r = self.lib.acm_automaton_add_approx(self.h, bytes(pattern), len(pattern), k, iid,
                                              _lib.PATTERN_NOCASE if nocase else 0)
        if r < 0:
            check(r, "acm_automaton_add_approx")
        return r

    @property
    def num_approx(self):
        return self.lib.acm_automaton_num_approx(self.h)

    def approx(self, x):
        """(first_piece, bytes, k, iid, flags) of approximate pattern x (acm_automaton_approx)"""
        f, n, k, iid, fl, b = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint(), C.c_void_p()
        check(self.lib.acm_automaton_approx(self.h, x, C.byref(f), C.byref(n), C.byref(k), C.byref(iid), C.byref(fl),
                                            C.byref(b)), "acm_automaton_approx")
        return f.value, C.string_at(b.value, n.value), k.value, iid.value, fl.value

    def pattern_approx(self, i):
        """(x, piece, pre, post) where pattern i is a piece of approximate pattern x (acm_automaton_pattern_approx):
        pre bytes of x lie in front of the piece and post behind it; None for a plain pattern"""
        x, j, pre, post = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        r = self.lib.acm_automaton_pattern_approx(self.h, i, C.byref(x), C.byref(j), C.byref(pre), C.byref(post))
        if r < 0:
            check(r, "acm_automaton_pattern_approx")
        return (x.value, j.value, pre.value, post.value) if r else None

    @property
    def approx_reach(self):
        """(back, ahead) over the approximate patterns: the largest length, the largest post"""
        b, f = C.c_int32(), C.c_int32()
        check(self.lib.acm_automaton_approx_reach(self.h, C.byref(b), C.byref(f)), "acm_automaton_approx_reach")
        return b.value, f.value

    def add_edit(self, pattern: bytes, k: int, iid: int = 0, nocase: bool = False):
        """An edit pattern (acm_automaton_add_edit): matches where at most k bytes are substituted, inserted or
        deleted, k <= 4.  Pieces, return value and errors as add_approx; k == 0 is a plain add.  The matches are
        verified by Matcher.scan_edit."""
        r = self.lib.acm_automaton_add_edit(self.h, bytes(pattern), len(pattern), k, iid,
                                            _lib.PATTERN_NOCASE if nocase else 0)
        if r < 0:
            check(r, "acm_automaton_add_edit")
        return r

    def approx_mode(self, x):
        """0 where approximate pattern x counts substitutions (add_approx), 1 where it is an edit pattern (add_edit)"""
        r = self.lib.acm_automaton_approx_mode(self.h, x)
        if r < 0:
            check(r, "acm_automaton_approx_mode")
        return r

    def add_rule(self, sequences, expr, iid=0):
        """A condition over the sequences that hit one text (acm_automaton_add_rule): sequences are the operands,
        sequence indices, expr e.g. "(0&1)|2>3" over their positions in that list.  Before or after compile(),
        but before the Matcher is made.  Returns the rule index."""
        sequences = list(sequences)
        q = (C.c_int32 * max(len(sequences), 1))(*sequences)
        expr = expr.encode() if isinstance(expr, str) else bytes(expr)
        r = self.lib.acm_automaton_add_rule(self.h, q, len(sequences), expr, iid)
        if r < 0:
            check(r, "acm_automaton_add_rule")
        return r

    def add_logical_signature(self, line, iid=0, nocase=False, extended=False, groups=False):
        """"expr;body0;body1;..." (acm_automaton_add_logical_signature): every body is added as add_signature
        adds it and the rule registered over the sequences; only before compile().  Returns the rule index."""
        line = line.encode() if isinstance(line, str) else bytes(line)
        r = self.lib.acm_automaton_add_logical_signature(self.h, line, iid, _lib.PATTERN_NOCASE if nocase else 0,
                                                         self._syntax(extended, groups))
        if r < 0:
            check(r, "acm_automaton_add_logical_signature")
        return r

    def load_logical_file(self, path, nocase=False, extended=False, groups=False):
        """logical signatures from a file, one per line with an optional leading "<iid>:"; returns how many"""
        n = self.lib.acm_automaton_load_logical_file(self.h, str(path).encode(), _lib.PATTERN_NOCASE if nocase else 0,
                                                     self._syntax(extended, groups))
        if n < 0:
            check(n, "acm_automaton_load_logical_file")
        return n

    @property
    def num_rules(self):
        return self.lib.acm_automaton_num_rules(self.h)

    def rule(self, i):
        """(sequences, expr, iid) of rule i (acm_automaton_rule)"""
        iid, n, seqs, expr = C.c_int32(), C.c_int32(), C.POINTER(C.c_int32)(), C.c_char_p()
        check(self.lib.acm_automaton_rule(self.h, i, C.byref(iid), C.byref(n), C.byref(seqs), C.byref(expr)),
              "acm_automaton_rule")
        return [seqs[j] for j in range(n.value)], expr.value.decode(), iid.value

    def sequence_rule(self, q):
        """(rule, operand) sequence q is an operand of, or None (acm_automaton_sequence_rule)"""
        r, op = C.c_int32(), C.c_int32()
        rc = self.lib.acm_automaton_sequence_rule(self.h, q, C.byref(r), C.byref(op))
        if rc < 0:
            check(rc, "acm_automaton_sequence_rule")
        return (r.value, op.value) if rc else None

    @property
    def num_sequences(self):
        return self.lib.acm_automaton_num_sequences(self.h)

    def sequence(self, i):
        """(parts, gaps, iid) of sequence i (acm_automaton_sequence): gaps a list of (lo, hi or None)"""
        iid, n = C.c_int32(), C.c_int32()
        parts, lo, hi = _lib._i32p(), _lib._i32p(), _lib._i32p()
        check(self.lib.acm_automaton_sequence(self.h, i, C.byref(iid), C.byref(n), C.byref(parts), C.byref(lo),
                                              C.byref(hi)), "acm_automaton_sequence")
        k = n.value
        gaps = [(lo[j], None if hi[j] == _lib.GAP_UNBOUNDED else hi[j]) for j in range(k - 1)]
        return [parts[j] for j in range(k)], gaps, iid.value

    def pattern_sequence(self, p):
        """(sequence, level) pattern p is a part of, or None (acm_automaton_pattern_sequence)"""
        s, lv = C.c_int32(), C.c_int32()
        r = self.lib.acm_automaton_pattern_sequence(self.h, p, C.byref(s), C.byref(lv))
        if r < 0:
            check(r, "acm_automaton_pattern_sequence")
        return (s.value, lv.value) if r else None

    def compile(self):
        check(self.lib.acm_automaton_compile(self.h), "acm_automaton_compile")
        return self

    @property
    def num_patterns(self):
        return self.lib.acm_automaton_num_patterns(self.h)

    @property
    def num_states(self):
        return self.lib.acm_automaton_num_states(self.h)

    @property
    def max_pattern_len(self):
        return self.lib.acm_automaton_max_pattern_len(self.h)

    def byte_classes(self):
        """(number of byte classes, byte -> class map as a 256-entry uint8 array); 256 classes: no compression"""
        m = np.zeros(256, dtype=np.uint8)
        return int(self.lib.acm_automaton_byte_classes(self.h, m.ctypes.data_as(C.c_void_p))), m

    def reference_table(self):
        """The reference-format table [states, 2, 256] int32 (acsmx.c:640-658)."""
        t = np.zeros((self.num_states, 2, 256), dtype=np.int32)
        check(self.lib.acm_automaton_export_reference_table(
            self.h, t.ctypes.data_as(C.POINTER(C.c_int32))), "export_reference_table")
        return t

    def pattern(self, i):
        iid, n, nxt = C.c_int32(), C.c_int32(), C.c_int32()
        p = C.c_void_p()
        check(self.lib.acm_automaton_pattern(self.h, i, C.byref(iid), C.byref(n), C.byref(p),
                                             C.byref(nxt)), "acm_automaton_pattern")
        data = C.string_at(p.value, n.value) if n.value else b""
        return data, iid.value, nxt.value

    def iids(self):
        """int32[num_patterns]: the id every pattern was added with (the 'ID pattern' form of a pattern file)"""
        return np.array([self.pattern(i)[1] for i in range(self.num_patterns)], dtype=np.int32)

    def state_matches(self, ref_state):
        """Every pattern index ending where the walk enters ref_state, list order."""
        buf = (C.c_int32 * 4096)()
        n = self.lib.acm_automaton_state_matches(self.h, ref_state, buf, 4096)
        if n < 0:
            raise ValueError("bad state %r" % (ref_state,))
        return list(buf[:n])

    def state_output(self, ref_state):
        return self.lib.acm_automaton_state_output(self.h, ref_state)

    def state_fail(self, ref_state):
        """fail link of a reference state (acm_automaton_state_fail)"""
        r = self.lib.acm_automaton_state_fail(self.h, ref_state)
        if r < 0:
            check(r, "acm_automaton_state_fail")
        return r

    def state_depth(self, ref_state):
        """trie depth of a reference state (acm_automaton_state_depth); 0 for the root"""
        r = self.lib.acm_automaton_state_depth(self.h, ref_state)
        if r < 0:
            check(r, "acm_automaton_state_depth")
        return r

    def close(self):
        if self.h:
            self.lib.acm_automaton_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _host_bytes(x):
    """contiguous uint8 array of host bytes: bytes, bytearray, memoryview or an array"""
    return np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) \
        else np.ascontiguousarray(x, dtype=np.uint8)


class _Pipeline:
    """One convenience call of a Matcher (scan_*), as a context manager.  It owns the text, `before` and starts
    on the device and every DeviceArray it hands out, and frees them all on the way out, raised or not.  It
    carries the current planes (pat, off: room cells, max_records of them to read, in report form); a stage
    enqueues one pass over them into planes of its own and makes those current.  Everything is on the matcher's
    stream.  A stage is sized by max_records: where the one in front left fewer, the caller reads the count
    (count(): the host waits there) and sets max_records from it."""

    def __init__(self, m, where, text=None, texts=None, segments=None, before=b""):
        self.m, self.where, self.stream, self.bufs = m, where, m.stream, []
        if texts is not None:
            self.t, self.starts = m.pack_segments(texts)
        else:
            self.t = _host_bytes(text)
            self.starts = np.ascontiguousarray(segments if segments is not None else [], dtype=np.int32)
        self.bf = np.frombuffer(bytes(before), dtype=np.uint8)
        self.n, self.nseg, self.before_len = int(self.t.size), int(self.starts.size), int(self.bf.size)

    def __enter__(self):
        m = self.m
        m.reserve(max(self.n, 1))
        self.cap = m.plane_capacity
        self._advance(m.pat_plane, m.off_plane, self.cap, _lib.REPORT_STATE)
        try:
            self.d = self.upload(self.t)
            self.d_bf = self.upload(self.bf) if self.before_len else None
            self.d_st = self.upload(self.starts, pad_to=0) if self.nseg else None
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()

    def _advance(self, pat, off, room, report):
        self.pat, self.off, self.room, self.max_records, self.report = pat, off, room, room - 2, report

    # ---- device memory, freed on the way out

    def alloc(self, nbytes):
        self.bufs.append(DeviceArray(nbytes))
        return self.bufs[-1]

    def upload(self, a, pad_to=16):
        self.bufs.append(DeviceArray.from_numpy(a, pad_to=pad_to, stream=self.stream))
        return self.bufs[-1]

    def planes(self, cells, k=2):
        return [self.alloc(cells * 4) for _ in range(k)]

    def workspace(self, query, *args):
        """(ptr, nbytes) of a block of query(*args) bytes, as the *_async calls take it"""
        nb = query(*args)
        return self.alloc(max(nb, 16)).ptr, nb

    # ---- stages: cells is the room of the planes the stage writes; ws a workspace() made earlier

    def scan(self, init_state=0, report=_lib.REPORT_STATE):
        self.m.scan_async(self.d, self.n, init_state, report=report)

    def segment(self, report=_lib.REPORT_STATE, seg_start=None, segments=None, seg_out=None, seg_counts=None, ws=None):
        """clamp every record to its own text: by default the call's starts, in STATE form for the next stage"""
        ws = ws or self.workspace(self.m.lib.acm_segment_workspace_bytes, self.max_records)
        pat, off = self.planes(self.cap)
        self.m.segment_async(self.pat, self.off, self.max_records, self.d_st if seg_start is None else seg_start,
                             self.nseg if segments is None else segments, self.n, pat, off, self.cap, seg_out=seg_out,
                             seg_counts=seg_counts, report=report, workspace=ws)
        self._advance(pat, off, self.cap, report)

    def expand(self, cells, ws=None):
        ws = ws or self.workspace(self.m.lib.acm_expand_workspace_bytes, self.max_records)
        pat, off = self.planes(cells)
        check(self.m.lib.acm_expand_matches_async(self.m.dfa, _ptr(self.pat), _ptr(self.off), self.max_records, pat.ptr,
                                                  off.ptr, cells, ws[0], ws[1], self.stream), "acm_expand_matches_async")
        self._advance(pat, off, cells, _lib.REPORT_HEAD)

    def every_pattern(self, cells):
        """every pattern of every record: the case pass when the matcher is mixed, else the expansion"""
        if self.m.mixed:
            self.case(cells, True)
        else:
            self.expand(cells)

    def word(self, cells, all_patterns, next_byte=-1, word_mask=None, ws=None):
        ws = ws or self.workspace(self.m.lib.acm_word_workspace_bytes, self.max_records)
        pat, off = self.planes(cells)
        self.m.word_async(self.pat, self.off, self.max_records, self.d, 0, self.n, pat, off, cells, before=self.d_bf,
                          before_len=self.before_len, next_byte=next_byte, seg_start=self.d_st, segments=self.nseg,
                          word_mask=word_mask, all_patterns=all_patterns, workspace=ws)
        self._advance(pat, off, cells, _lib.REPORT_HEAD)

    def case(self, cells, all_patterns, ws=None):
        ws = ws or self.workspace(self.m.lib.acm_case_workspace_bytes, self.max_records)
        pat, off = self.planes(cells)
        self.m.case_async(self.pat, self.off, self.max_records, self.d, 0, self.n, pat, off, cells, before=self.d_bf,
                          before_len=self.before_len, all_patterns=all_patterns, workspace=ws)
        self._advance(pat, off, cells, _lib.REPORT_HEAD)

    def wildcard(self, cells, info, all_patterns, lead_begin):
        ws = self.workspace(self.m.lib.acm_wildcard_workspace_bytes, self.max_records)
        pat, off = self.planes(cells)
        self.m.wildcard_async(self.pat, self.off, self.max_records, self.d, 0, self.n, pat, off, cells, info,
                              report=self.report, before=self.d_bf, before_len=self.before_len, seg_start=self.d_st,
                              segments=self.nseg, lead_begin=lead_begin, open_end=self.n, all_patterns=all_patterns,
                              workspace=ws)
        self._advance(pat, off, cells, _lib.REPORT_HEAD)

    def approx(self, cells, info, lead_begin, dist=True):
        """the approx pass over the current planes; returns the distance plane (None without dist)"""
        ws = self.workspace(self.m.lib.acm_approx_workspace_bytes, self.max_records)
        pat, off = self.planes(cells)
        d = self.alloc(cells * 4) if dist else None
        self.m.approx_async(self.pat, self.off, self.max_records, self.d, 0, self.n, pat, off, cells, info, dist_out=d,
                            report=self.report, before=self.d_bf, before_len=self.before_len, seg_start=self.d_st,
                            segments=self.nseg, lead_begin=lead_begin, open_end=self.n, workspace=ws)
        self._advance(pat, off, cells, _lib.REPORT_HEAD)
        return d

    def edit(self, cells, info, lead_begin):
        """the edit pass over the current planes; returns the distance and the length plane"""
        ws = self.workspace(self.m.lib.acm_edit_workspace_bytes, self.m.dfa, self.max_records)
        pat, off, d, ln = self.planes(cells, 4)
        self.m.edit_async(self.pat, self.off, self.max_records, self.d, 0, self.n, pat, off, cells, info, dist_out=d,
                          len_out=ln, report=self.report, before=self.d_bf, before_len=self.before_len,
                          seg_start=self.d_st, segments=self.nseg, lead_begin=lead_begin, open_end=self.n, workspace=ws)
        self._advance(pat, off, cells, _lib.REPORT_HEAD)
        return d, ln

    def position(self, cells, info, all_patterns, lead_begin, open_end, ws=None):
        ws = ws or self.workspace(self.m.lib.acm_position_workspace_bytes, self.max_records)
        pat, off = self.planes(cells)
        self.m.position_async(self.pat, self.off, self.max_records, pat, off, cells, info, report=self.report,
                              seg_start=self.d_st, segments=self.nseg, lead_begin=lead_begin, text_end=self.n,
                              open_end=open_end, all_patterns=all_patterns, workspace=ws)
        self._advance(pat, off, cells, _lib.REPORT_HEAD)

    def sequence(self, cells, info, lead_begin):
        ws = self.workspace(self.m.lib.acm_sequence_workspace_bytes, self.m.dfa, self.max_records)
        seq, off = self.planes(cells)
        self.m.sequence_async(self.pat, self.off, self.max_records, seq, off, cells, info, seg_start=self.d_st,
                              segments=self.nseg, lead_begin=lead_begin, text_end=self.n, workspace=ws)
        self._advance(seq, off, cells, _lib.REPORT_HEAD)

    def rule(self, cells, info):
        """the current planes become (rule, offset); returns the third, the text of every record"""
        ws = self.workspace(self.m.lib.acm_rule_workspace_bytes, self.m.dfa, self.max_records)
        rule, text, off = self.planes(cells, 3)
        self.m.rule_async(self.pat, self.off, self.max_records, rule, text, off, cells, info, seg_start=self.d_st,
                          segments=self.nseg, workspace=ws)
        self._advance(rule, off, cells, _lib.REPORT_HEAD)
        return text

    def select(self, cells, info, min_start=0):
        """the current planes become the selected (pattern, offset); returns the third, the start of every match"""
        ws = self.workspace(self.m.lib.acm_select_workspace_bytes, self.max_records)
        pat, off, start = self.planes(cells, 3)
        self.m.select_async(self.pat, self.off, self.max_records, pat, off, cells, info, start_out=start,
                            min_start=min_start, workspace=ws)
        self._advance(pat, off, cells, _lib.REPORT_HEAD)
        return start

    def rewrite(self, info, out_capacity, d_text=None, n=None, text_origin=0, at_cells=None):
        """the rewrite over the current planes (the select pass's); returns (out, at, seg_out): the output bytes, the
        plane of where every match's replacement begins, and where every text begins (None without texts)"""
        ws = self.workspace(self.m.lib.acm_rewrite_workspace_bytes, self.max_records, self.nseg)
        out = self.alloc(max((out_capacity + 15) // 16 * 16, 16))
        at = self.alloc((at_cells if at_cells is not None else self.max_records + 2) * 4)
        seg = self.alloc(self.nseg * 4) if self.nseg else None
        self.m.rewrite_async(self.d if d_text is None else d_text, self.n if n is None else n, self.pat, self.off,
                             self.max_records, out, out_capacity, info, text_origin=text_origin, at_out=at,
                             at_capacity=at.nbytes // 4, seg_start=self.d_st, segments=self.nseg, seg_out=seg,
                             workspace=ws)
        return out, at, seg

    def normalize(self, flags, blank_mask=None, blank_byte=0x20, out_capacity=None):
        """the normalise pass over the pipeline's text, which the normalised text then replaces (with texts, their
        starts in it replace the starts): every later stage runs on it.  What normalize_remap needs is kept.  The
        scan's length is a host argument, so the host waits here once and reads the figures; returns them, int32[8]"""
        cap = self.n if out_capacity is None else out_capacity
        ws = self.workspace(self.m.lib.acm_normalize_workspace_bytes, self.n, self.nseg)
        out = self.alloc((cap + 15) // 16 * 16 + 16)
        keep = self.alloc(max((self.n + 63) // 64 * 8, 16))
        block = self.alloc(((self.n + _lib.NORM_BLOCK - 1) // _lib.NORM_BLOCK + 1) * 4)
        seg = self.alloc(self.nseg * 4) if self.nseg else None
        info = self.alloc(32)
        self.m.normalize_async(self.d, self.n, flags, out, cap, keep, block, info, blank_mask=blank_mask,
                               blank_byte=blank_byte, seg_start=self.d_st, segments=self.nseg, seg_out=seg, workspace=ws)
        res = info.to_numpy(np.int32, 8, stream=self.stream)
        if res[4]:
            raise AcmError(_lib.ACM_ERR_CAPACITY, self.where, "the normalised text has %d bytes but the buffer holds %d" % (
                int(res[0]), cap))
        self.norm = (self.d, self.n, flags, keep, block)
        self.d, self.n, self.d_st = out, int(res[0]), seg
        return res

    def normalize_remap(self, info):
        """the current planes (pattern, offset in the normalised text) brought back to the text normalize() read: the
        offset plane in place becomes where every match ends; returns the plane of where it starts"""
        d, n, flags, keep, block = self.norm
        start = self.alloc(self.room * 4)
        self.m.normalize_remap_async(d, n, flags, keep, block, self.off, self.max_records, self.off, info,
                                     pat_plane=self.pat, start_out=start)
        return start

    def line_context(self, starts, lcap, linfo, cinfo, before, after, invert, ws):
        """the context pass over the current planes' offsets and the device-made starts; returns the planes (rel,
        begin, next, lines) of the groups, lcap + 2 cells each.  ws: (buffer, nbytes)"""
        rel, beg, nxt, cnt = self.planes(lcap + 2, 4)
        self.m.line_context_async(starts, lcap, linfo, 0, self.n, self.off, self.max_records, rel, beg, nxt, lcap + 2, cinfo,
                                  before=before, after=after, invert=invert, lines_out=cnt, seg_start=self.d_st,
                                  segments=self.nseg, workspace=ws)
        return rel, beg, nxt, cnt

    def extract(self, begin, end, ranges, info, out_capacity, glue, terminator, end_inclusive=False):
        """the extract over the text and two planes of ranges; returns (out, at, seg_out): the output bytes, the plane
        of where every range's bytes begin, and the output in front of every text (None without texts)"""
        ws = self.workspace(self.m.lib.acm_extract_workspace_bytes, ranges, self.nseg)
        out = self.alloc(max((out_capacity + 15) // 16 * 16, 16))
        at = self.alloc((ranges + 2) * 4)
        seg = self.alloc(self.nseg * 4) if self.nseg else None
        self.m.extract_async(self.d, self.n, begin, end, ranges, out, out_capacity, info, end_inclusive=end_inclusive,
                             glue=glue, terminator=terminator, at_out=at, at_capacity=ranges + 2, seg_start=self.d_st,
                             segments=self.nseg, seg_out=seg, workspace=ws)
        return out, at, seg

    def line_context_lines(self, starts, lcap, linfo, cinfo, before, after, invert, ws):
        """the per-line context pass over the current planes' offsets and the device-made starts; returns the planes
        (rel, begin, next, kind) of the kept lines, lcap + 2 cells each.  ws: (buffer, nbytes)"""
        rel, beg, nxt, kind = self.planes(lcap + 2, 4)
        self.m.line_context_lines_async(starts, lcap, linfo, 0, self.n, self.off, self.max_records, rel, beg, nxt, kind,
                                        lcap + 2, cinfo, before=before, after=after, invert=invert, seg_start=self.d_st,
                                        segments=self.nseg, workspace=ws)
        return rel, beg, nxt, kind

    def format(self, begin, end, ranges, info, out_capacity, glue, terminator, end_inclusive=False, **prefix):
        """the format pass over the text and two planes of ranges; prefix: format_async's kind_plane, num_plane,
        seg_num, names, name_off, names_bytes, number, offset, bases and separators.  Returns (out, at, seg_out) as
        extract does"""
        ws = self.workspace(self.m.lib.acm_format_workspace_bytes, ranges, self.nseg)
        out = self.alloc(max((out_capacity + 15) // 16 * 16, 16))
        at = self.alloc((ranges + 2) * 4)
        seg = self.alloc(self.nseg * 4) if self.nseg else None
        self.m.format_async(self.d, self.n, begin, end, ranges, out, out_capacity, info, end_inclusive=end_inclusive,
                            glue=glue, terminator=terminator, at_out=at, at_capacity=ranges + 2, seg_start=self.d_st,
                            segments=self.nseg, seg_out=seg, workspace=ws, **prefix)
        return out, at, seg

    # ---- results

    def count(self):
        """the records in the current planes, from the header cell: the host waits for the stream here"""
        n = int(self.pat.to_numpy(np.int32, 1, stream=self.stream)[0])
        if n > self.room - 2:
            raise AcmError(_lib.ACM_ERR_CAPACITY, self.where, "%d records but planes hold %d" % (n, self.room - 2))
        return n

    def download(self, n, *more):
        """(offsets uint32, cells int32, trailer) of the n records of the current planes, then the cells of
        every further plane given"""
        p, o = (x.to_numpy(np.int32, n + 2, stream=self.stream) for x in (self.pat, self.off))
        return (o[1:1 + n].astype(np.uint32), p[1:1 + n].copy(), int(p[n + 1])) + \
            tuple(x.to_numpy(np.int32, n + 2, stream=self.stream)[1:1 + n].copy() for x in more)


class Matcher:
    """Device DFA + scratch + result planes for texts up to max_text bytes."""

    def __init__(self, automaton, device=0, max_text=1 << 20, plane_capacity=None, stream=None):
        self.lib = _lib.load()
        self.device = device
        self.stream = stream
        h = C.c_void_p()
        check(self.lib.acm_dfa_upload(automaton.h, device, C.byref(h)), "acm_dfa_upload")
        self.dfa = h.value
        self.num_patterns = automaton.num_patterns
        self.mixed, self.positioned = automaton.mixed_case, automaton.positioned     # as uploaded (scan_sequences)
        self.wild = automaton.has_wildcards
        # the most bytes one match can add to a rewrite: the longest replacement against a span of one byte
        self.max_growth = max(self.lib.acm_automaton_max_replacement_len(automaton.h) - 1, 0)
        # post context of every sequence's last part: a match ends that far behind the offset the sequence pass reports
        self.seq_post = np.array([automaton.wildcard_lengths(automaton.sequence(q)[0][-1])[1]
                                  for q in range(automaton.num_sequences)] if self.wild else [], dtype=np.int64)
        # per pattern, for scan_approx: the first piece of the approximate pattern it is a piece of (else itself), and
        # how far behind a piece's end the match ends
        self.approx_first = np.arange(self.num_patterns, dtype=np.int32)
        self.approx_post = np.zeros(self.num_patterns, dtype=np.int64)
        for x in range(automaton.num_approx):
            first, b, k = automaton.approx(x)[:3]
            for j in range(k + 1):
                self.approx_first[first + j] = first
                self.approx_post[first + j] = automaton.pattern_approx(first + j)[3]
        self.max_text = 0
        self.ws = self.pat_plane = self.off_plane = None
        self.reserve(max_text, plane_capacity)

    def reserve(self, max_text, plane_capacity=None):
        cap = plane_capacity if plane_capacity is not None else max_text + 2
        if max_text <= self.max_text and cap <= getattr(self, "plane_capacity", 0):
            return
        for b in (self.ws, self.pat_plane, self.off_plane):
            if b is not None:
                b.free()
        self.max_text = max_text
        self.plane_capacity = max(cap, 2)
        self.ws_bytes = self.lib.acm_scan_workspace_bytes(self.dfa, max_text)
        self.ws = DeviceArray(self.ws_bytes, self.device)
        self.pat_plane = DeviceArray(self.plane_capacity * 4)
        self.off_plane = DeviceArray(self.plane_capacity * 4)

    @property
    def hot_rows(self):
        return self.lib.acm_dfa_hot_rows(self.dfa)

    @property
    def device_bytes(self):
        return self.lib.acm_dfa_device_bytes(self.dfa)

    def set_chain_bytes(self, s):
        return self.lib.acm_scan_set_chain_bytes(self.dfa, s)

    def set_chains_per_lane(self, c):
        return self.lib.acm_scan_set_chains_per_lane(self.dfa, c)

    MODES = {"auto": 0, "chain": 1, "sparse": 2}
    PATHS = {1: "chain", 2: "sparse", 0xDEAD: "failed"}

    def set_mode(self, mode):
        """'auto' | 'chain' | 'sparse' (acm_scan_set_mode); returns the mode in use."""
        got = self.lib.acm_scan_set_mode(self.dfa, self.MODES[mode])
        return [k for k, v in self.MODES.items() if v == got][0]

    def set_graphs(self, enable):
        """Replay repeating scans as HIP graphs (acm_scan_set_graphs); returns the setting in use."""
        return bool(self.lib.acm_scan_set_graphs(self.dfa, int(enable)))

    def graph_stats(self):
        """(graphs instantiated, hipGraphLaunch calls issued) since upload (acm_scan_graph_stats)."""
        cap, run = C.c_uint64(), C.c_uint64()
        check(self.lib.acm_scan_graph_stats(self.dfa, C.byref(cap), C.byref(run)), "acm_scan_graph_stats")
        return cap.value, run.value

    def sparse_eligible(self):
        return bool(self.lib.acm_scan_sparse_eligible(self.dfa))

    def lds_resident(self):
        """the chain pipeline walks this set with the whole automaton in LDS (lds_walk.hip)"""
        return bool(self.lib.acm_scan_lds_resident(self.dfa))

    def group_capable(self):
        """consecutive batches of one size share their launches in the current mode (acm_scan_batches_async)"""
        return bool(self.lib.acm_scan_group_capable(self.dfa))

    def path_taken(self, n, stream=None, workspace=None):
        """Which pipeline produced the planes of the last n-byte scan (synchronises)."""
        st = stream if stream is not None else self.stream
        ws_ptr = workspace[0] if workspace is not None else self.ws.ptr
        rc = self.lib.acm_scan_path_taken(self.dfa, _ptr(ws_ptr), n, st)
        if rc < 0:
            check(rc, "acm_scan_path_taken")
        return self.PATHS[rc]

    def scan_async(self, d_text, n, init_state=0, stream=None, pat_plane=None, off_plane=None,
                   plane_capacity=None, halo=0, offset_shift=0, workspace=None, wait_before_walk=None,
                   record_after_walk=None, report=0):
        """Enqueue one scan of device text; nothing is synchronised.

        halo/offset_shift: shard form (acm_scan_shard_async).  workspace: (ptr, nbytes) of a
        caller-owned scratch block instead of the matcher's own.  wait_before_walk /
        record_after_walk: hipEvent_t handles chaining the walk kernels of batches that are in
        flight on different streams (acm_scan_batch_async).
        """
        if workspace is None and n > self.max_text:
            raise ValueError("text of %d bytes exceeds reserved %d" % (n, self.max_text))
        st = stream if stream is not None else self.stream
        ws_ptr, ws_bytes = workspace if workspace is not None else (self.ws.ptr, self.ws_bytes)
        pat = _ptr(pat_plane) if pat_plane is not None else self.pat_plane.ptr
        off = _ptr(off_plane) if off_plane is not None else self.off_plane.ptr
        cap = plane_capacity if plane_capacity is not None else self.plane_capacity
        if wait_before_walk is not None or record_after_walk is not None or report:
            b = _lib.ScanBatch(_ptr(d_text), n, halo, offset_shift, init_state, _ptr(ws_ptr), ws_bytes, pat, off, cap,
                               st, wait_before_walk, record_after_walk, report)
            check(self.lib.acm_scan_batch_async(self.dfa, C.byref(b)), "acm_scan_batch_async")
            return
        check(self.lib.acm_scan_shard_async(self.dfa, _ptr(d_text), n, halo, offset_shift, init_state, _ptr(ws_ptr),
                                            ws_bytes, pat, off, cap, st), "acm_scan_async")

    def make_batch(self, d_text, n, stream, pat_plane, off_plane, plane_capacity, workspace, init_state=0, halo=0,
                   offset_shift=0, report=0, profile=False, init_plane=None, init_plane_capacity=0):
        """A reusable acm_scan_batch for enqueue(): a worker that scans with the same buffers over and
        over builds its batches once and pays one foreign call per scan."""
        return _lib.ScanBatch(_ptr(d_text), n, halo, offset_shift, init_state, _ptr(workspace[0]), workspace[1],
                              _ptr(pat_plane), _ptr(off_plane), plane_capacity, stream, None, None, report,
                              1 if profile else 0, _ptr(init_plane) if init_plane is not None else None,
                              init_plane_capacity)

    def enqueue(self, batch):
        rc = self.lib.acm_scan_batch_async(self.dfa, C.byref(batch))
        if rc:
            check(rc, "acm_scan_batch_async")

    def enqueue_many(self, batches):
        """acm_scan_batches_async: the batches in order with one foreign call; consecutive sparse
        batches of one size on one stream with their own workspaces and planes share their launches."""
        arr = (_lib.ScanBatch * len(batches))(*batches)
        rc = self.lib.acm_scan_batches_async(self.dfa, arr, len(batches))
        if rc:
            check(rc, "acm_scan_batches_async")

    def set_max_group(self, batches):
        return int(self.lib.acm_scan_set_max_group(self.dfa, int(batches)))

    def fetch(self, stream=None):
        """(offsets u32[], patterns i32[], last_state) of the last scan."""
        st = stream if stream is not None else self.stream
        head = self.pat_plane.to_numpy(np.int32, 1, stream=st)
        m = int(head[0])
        stored = min(m, self.plane_capacity - 2)
        pat = self.pat_plane.to_numpy(np.int32, stored + 2, stream=st)
        off = self.off_plane.to_numpy(np.int32, stored + 2, stream=st)
        if m > stored:
            raise AcmError(_lib.ACM_ERR_CAPACITY, "Matcher.fetch",
                           "%d matches but planes hold %d" % (m, stored))
        return off[1:1 + m].astype(np.uint32), pat[1:1 + m].copy(), int(pat[m + 1])

    def scan_all(self, text, init_state=0, out_capacity=None):
        """All-patterns reporting: scan with the final states in the pattern
        plane, expand every state's match list on the device (acm_expand_matches_async), download.
        Returns (offsets, patterns, last_state) with one record per pattern ending at each offset."""
        with _Pipeline(self, "Matcher.scan_all", text) as p:
            ws = p.workspace(self.lib.acm_expand_workspace_bytes, p.max_records)
            p.scan(init_state)
            p.expand(out_capacity if out_capacity is not None else 8 * p.cap, ws)
            return p.download(p.count())

    @contextlib.contextmanager
    def _workspace(self, workspace, stream, query, *args):
        """(ptr, nbytes) for one pass: the caller's, or with None a temporary block of query(*args) bytes that
        lives until the stream has passed it: on the way out, raised or not, the stream is synchronised"""
        if workspace is not None:
            yield workspace
            return
        nb = query(*args)
        tmp = DeviceArray(max(nb, 16))
        try:
            yield tmp.ptr, nb
        finally:
            check(self.lib.acm_rt_stream_sync(stream), "acm_rt_stream_sync")
            tmp.free()

    def segment_async(self, state_plane, off_plane, max_records, seg_start, segments, text_end, pat_out, off_out,
                      out_capacity, seg_out=None, seg_counts=None, report=0, workspace=None, stream=None):
        """Enqueue the segment pass (acm_segment_matches_async) over caller-owned device planes: the
        records of a REPORT_STATE scan, each clamped to its own segment.  seg_start: device int32
        [segments] (None when segments == 0).  workspace: (ptr, nbytes), or None for a temporary one
        that lives until the stream has passed it (the call then synchronises)."""
        st = stream if stream is not None else self.stream
        with self._workspace(workspace, st, self.lib.acm_segment_workspace_bytes, max_records) as (ws, nb):
            check(self.lib.acm_segment_matches_async(
                self.dfa, _ptr(state_plane), _ptr(off_plane), max_records, _ptr(seg_start), segments, text_end,
                report, _ptr(pat_out), _ptr(off_out), _ptr(seg_out), out_capacity, _ptr(seg_counts),
                _ptr(ws), nb, st), "acm_segment_matches_async")

    @staticmethod
    def pack_segments(texts):
        """(uint8 text, int32 starts) of a list of bytes-like texts, or of a (text, starts) pair."""
        if isinstance(texts, tuple):
            t, starts = texts
            return np.ascontiguousarray(t, dtype=np.uint8), np.ascontiguousarray(starts, dtype=np.int32)
        parts = [np.frombuffer(bytes(x), dtype=np.uint8) for x in texts]
        sizes = np.array([p.size for p in parts], dtype=np.int64)
        starts = np.zeros(len(parts), dtype=np.int64)
        if len(parts) > 1:
            starts[1:] = np.cumsum(sizes)[:-1]
        t = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
        return t, starts.astype(np.int32)

    def scan_segments(self, texts, init_state=0, all_patterns=False, counts=False, out_capacity=None):
        """Scan many independent texts in one batch: each text is matched as if scanned alone from the
        root (acm_segment_matches_async behind an ordinary scan).  texts: a list of bytes-like objects,
        or a (uint8 array, int32 starts) pair.  Returns (offsets, patterns, segment_ids, last_state),
        offsets in the coordinates of the concatenation; with counts=True also the records per text.
        Records before the first start continue a text that init_state was in (segment -1).
        all_patterns: every pattern of each record's clamped state (acm_expand_matches_async)."""
        with _Pipeline(self, "Matcher.scan_segments", texts=texts) as p:
            nseg = p.nseg
            ws = p.workspace(self.lib.acm_segment_workspace_bytes, p.max_records)
            seg, cnt = p.alloc(p.cap * 4), p.alloc(max(nseg, 1) * 4)
            p.scan(init_state)
            p.segment(_lib.REPORT_STATE if all_patterns else _lib.REPORT_HEAD, seg_out=seg,
                      seg_counts=cnt if nseg else None, ws=ws)
            m = p.count()
            if not all_patterns:
                offs, pats, last, sg = p.download(m, seg)
                res = (offs, pats, sg, last)
                if counts:
                    res += (cnt.to_numpy(np.int32, nseg, stream=self.stream),)
                return res
            p.max_records = max(m, 1)
            p.expand(out_capacity if out_capacity is not None else 8 * p.cap)
            offs, pats, last = p.download(p.count())
            sg = (np.searchsorted(p.starts, offs.astype(np.int64), side="right") - 1).astype(np.int32)
            res = (offs, pats, sg, last)
            if counts:
                res += (np.bincount(sg[sg >= 0], minlength=nseg).astype(np.int32)[:nseg],)
            return res

    @staticmethod
    def word_mask(word_set):
        """32-byte mask (bit b of byte b // 8: byte b is a word byte) of an iterable of byte values or a
        bytes-like object listing the word bytes; None stays None (the default set [0-9A-Za-z_])."""
        if word_set is None:
            return None
        m = np.zeros(256, dtype=np.uint8)
        vals = np.frombuffer(bytes(word_set), dtype=np.uint8) if isinstance(word_set, (bytes, bytearray, memoryview)) \
            else np.asarray(list(word_set), dtype=np.int64)
        if vals.size:
            m[vals] = 1
        return np.packbits(m, bitorder="little").tobytes()

    def word_async(self, state_plane, off_plane, max_records, d_text, text_origin, text_end, pat_out, off_out,
                   out_capacity, before=None, before_len=0, next_byte=-1, seg_start=None, segments=0,
                   word_mask=None, all_patterns=False, tail_out=None, workspace=None, stream=None):
        """Enqueue the word pass (acm_word_matches_async) over caller-owned device planes: the records of
        a REPORT_STATE scan (or of the segment pass in STATE form) kept where a pattern is a whole word.
        word_mask: 32 bytes (Matcher.word_mask) or None for [0-9A-Za-z_].  workspace: (ptr, nbytes), or
        None for a temporary one that lives until the stream has passed it (the call then synchronises)."""
        st = stream if stream is not None else self.stream
        mask = None
        if word_mask is not None:
            if len(word_mask) != 32:
                raise ValueError("word_mask must be 32 bytes")
            mask = C.create_string_buffer(bytes(word_mask), 32)
        with self._workspace(workspace, st, self.lib.acm_word_workspace_bytes, max_records) as (ws, nb):
            check(self.lib.acm_word_matches_async(
                self.dfa, _ptr(state_plane), _ptr(off_plane), max_records, _ptr(d_text), text_origin, text_end,
                _ptr(before), before_len, next_byte, _ptr(seg_start), segments, mask, 1 if all_patterns else 0,
                _ptr(pat_out), _ptr(off_out), out_capacity, _ptr(tail_out), _ptr(ws), nb, st),
                "acm_word_matches_async")

    def scan_words(self, text, all_patterns=False, word_set=None, segments=None, init_state=0, before=b"",
                   next_byte=-1, out_capacity=None):
        """Whole-word matching (grep -w): scan host bytes and keep a pattern only where the bytes around
        it are not word bytes (acm_word_matches_async behind a REPORT_STATE scan).  word_set: the word
        bytes (bytes-like or iterable of ints), None for [0-9A-Za-z_].  segments: int32 text starts;
        the records then go through the segment pass first.  before: the bytes in front of text (a
        stream's previous piece; further back is a text start); next_byte: the byte after text, or -1.
        all_patterns: every word-bounded pattern, else the first in list order.  Returns
        (offsets, patterns, last_state)."""
        with _Pipeline(self, "Matcher.scan_words", text, segments=segments, before=before) as p:
            ocap = out_capacity if out_capacity is not None else (8 * p.cap if all_patterns else p.cap)
            ws = p.workspace(self.lib.acm_word_workspace_bytes, p.max_records)
            p.scan(init_state)
            if p.nseg:
                p.segment()
            p.word(ocap, all_patterns, next_byte=next_byte, word_mask=self.word_mask(word_set), ws=ws)
            return p.download(p.count())

    def case_async(self, state_plane, off_plane, max_records, d_text, text_origin, text_end, pat_out, off_out,
                   out_capacity, before=None, before_len=0, all_patterns=False, tail_out=None, workspace=None,
                   stream=None):
        """Enqueue the case pass (acm_case_matches_async) over caller-owned device planes: the records of
        a REPORT_STATE scan (or of the segment pass in STATE form) of a mixed automaton, an exact pattern
        kept only where the text equals its bytes as added.  workspace: (ptr, nbytes), or None for a
        temporary one that lives until the stream has passed it (the call then synchronises)."""
        st = stream if stream is not None else self.stream
        with self._workspace(workspace, st, self.lib.acm_case_workspace_bytes, max_records) as (ws, nb):
            check(self.lib.acm_case_matches_async(
                self.dfa, _ptr(state_plane), _ptr(off_plane), max_records, _ptr(d_text), text_origin, text_end,
                _ptr(before), before_len, 1 if all_patterns else 0, _ptr(pat_out), _ptr(off_out), out_capacity,
                _ptr(tail_out), _ptr(ws), nb, st), "acm_case_matches_async")

    def scan_case(self, text, all_patterns=False, texts=None, init_state=0, before=b"", out_capacity=None):
        """Matches of an automaton with case sensitivity per pattern (Automaton.add(..., nocase=True)):
        a REPORT_STATE scan, the segment pass when texts is given, then the case pass
        (acm_case_matches_async).  text: host bytes; or None with texts: a list of bytes-like objects or
        a (uint8 array, int32 starts) pair, each matched as if scanned alone.  before: the bytes in
        front of text (a stream's previous piece).  all_patterns: every kept pattern, else the first
        in list order.  Returns (offsets, patterns, last_state) as scan_all does."""
        with _Pipeline(self, "Matcher.scan_case", text, texts, before=before) as p:
            ocap = out_capacity if out_capacity is not None else (8 * p.cap if all_patterns else p.cap)
            ws = p.workspace(self.lib.acm_case_workspace_bytes, p.max_records)
            p.scan(init_state)
            if p.nseg:
                p.segment()
            p.case(ocap, all_patterns, ws=ws)
            return p.download(p.count())

    def position_async(self, pat_plane, off_plane, max_records, pat_out, off_out, out_capacity, info, report=0,
                       seg_start=None, segments=0, lead_begin=0, text_end=0, open_end=-1, all_patterns=False,
                       workspace=None, stream=None):
        """Enqueue the position pass (acm_position_matches_async) over caller-owned device planes: states
        (report=REPORT_STATE) or pattern indices (REPORT_HEAD: a HEAD scan, or the all-patterns output of
        the word, case or expand pass), an entry kept where its pattern's window holds.  info: device
        int32[4].  workspace: (ptr, nbytes), or None for a temporary one that lives until the stream has
        passed it (the call then synchronises)."""
        st = stream if stream is not None else self.stream
        with self._workspace(workspace, st, self.lib.acm_position_workspace_bytes, max_records) as (ws, nb):
            check(self.lib.acm_position_matches_async(
                self.dfa, _ptr(pat_plane), _ptr(off_plane), max_records, report, _ptr(seg_start), segments, lead_begin,
                text_end, open_end, 1 if all_patterns else 0, _ptr(pat_out), _ptr(off_out), out_capacity, _ptr(info),
                _ptr(ws), nb, st), "acm_position_matches_async")

    def scan_positions(self, text=None, texts=None, all_patterns=False, then=None, lead_begin=0, open_end="end",
                       init_state=0, before=b"", out_capacity=None):
        """Matches that obey the patterns' position constraints (Automaton.set_position): a REPORT_STATE
        scan, the segment pass when texts is given (each text matched alone and its own [T0, Tend)), then
        the position pass (acm_position_matches_async).  then: None, "case" or "words": that pass runs in
        its all-patterns form in between and the position pass takes its pattern-form output, so a
        constraint composes with exact-case or whole-word matching.  lead_begin: where the text in front
        of the first start began (text given: where it began; may be negative).  open_end: where the last
        text ends: "end" (with the bytes given), an int >= the bytes given, or None: unknown, end-anchored
        entries of that text are dropped and counted.  before: the bytes in front of text, for then.
        Returns (offsets, patterns, last_state, undecided)."""
        if then not in (None, "case", "words"):
            raise ValueError("then must be None, 'case' or 'words'")
        with _Pipeline(self, "Matcher.scan_positions", text, texts, before=before) as p:
            end = -1 if open_end is None else p.n if isinstance(open_end, str) else int(open_end)
            ocap = out_capacity if out_capacity is not None else (8 * p.cap if all_patterns or then else p.cap)
            # one workspace, sized before the scan for either input: the scan's records, or the pass in between's
            ws = p.workspace(self.lib.acm_position_workspace_bytes, max(p.max_records, 8 * p.cap))
            info = p.alloc(16)
            p.scan(init_state)
            if p.nseg:
                p.segment()
            if then:
                (p.case if then == "case" else p.word)(8 * p.cap, True)
                p.count()                      # (checked only: the position pass takes the whole planes)
            p.position(ocap, info, all_patterns, int(lead_begin), end, ws=ws)
            return p.download(p.count()) + (int(info.to_numpy(np.int32, 4, stream=self.stream)[0]),)

    def wildcard_async(self, pat_plane, off_plane, max_records, d_text, text_origin, text_end, pat_out, off_out,
                       out_capacity, info, report=0, before=None, before_len=0, seg_start=None, segments=0, lead_begin=0,
                       open_end=-1, all_patterns=True, workspace=None, stream=None):
        """Enqueue the wildcard pass (acm_wildcard_matches_async) over caller-owned device planes: states
        (report=REPORT_STATE) or pattern indices (REPORT_HEAD, all_patterns only), an entry kept where the bytes
        around its anchor lie in its pattern's context sets (Automaton.add_wildcard).  info: device int32[4].
        workspace: (ptr, nbytes), or None for a temporary one that lives until the stream has passed it (the
        call then synchronises)."""
        st = stream if stream is not None else self.stream
        with self._workspace(workspace, st, self.lib.acm_wildcard_workspace_bytes, max_records) as (ws, nb):
            check(self.lib.acm_wildcard_matches_async(
                self.dfa, _ptr(pat_plane), _ptr(off_plane), max_records, report, _ptr(d_text), text_origin, text_end,
                _ptr(before), before_len, _ptr(seg_start), segments, lead_begin, open_end, 1 if all_patterns else 0,
                _ptr(pat_out), _ptr(off_out), out_capacity, _ptr(info), _ptr(ws), nb, st),
                "acm_wildcard_matches_async")

    def scan_wildcards(self, text=None, texts=None, all_patterns=False, before=b"", init_state=0, out_capacity=None):
        """Matches of an automaton with wildcard patterns (Automaton.add_wildcard): a REPORT_STATE scan, the
        segment pass when texts is given (each text matched alone), then the wildcard pass
        (acm_wildcard_matches_async).  A mixed automaton: the case pass in its all form runs in between and the
        wildcard pass takes its pattern-form output (then, without all_patterns, the position pass picks the
        first entry of every offset).  text: host bytes; or None with texts: a list of bytes-like objects or a
        (uint8 array, int32 starts) pair.  before: the bytes in front of text, part of the same text.  The
        text ends with the bytes given.  Returns (offsets, patterns, last_state, info): the offsets are the
        ANCHORS' ends (a match ends Automaton.wildcard_lengths(p)[1] bytes behind), info[0] the undecided
        entries."""
        with _Pipeline(self, "Matcher.scan_wildcards", text, texts, before=before) as p:
            ocap = out_capacity if out_capacity is not None else (8 * p.cap if all_patterns or self.mixed else p.cap)
            info = p.alloc(16)
            p.scan(init_state)
            if p.nseg:
                p.segment()
            if self.mixed:
                p.case(8 * p.cap, True)
                p.max_records = p.count()
            p.wildcard(ocap, info, all_patterns or self.mixed, -p.before_len)
            m = p.count()
            und = info.to_numpy(np.int32, 4, stream=self.stream)
            if self.mixed and not all_patterns:        # the first entry of every offset: the position pass in head form
                p.max_records = m
                p.position(m + 2, p.alloc(16), False, -p.before_len, p.n)
                m = p.count()
            return p.download(m) + (und,)

    def approx_async(self, pat_plane, off_plane, max_records, d_text, text_origin, text_end, pat_out, off_out,
                     out_capacity, info, dist_out=None, report=0, before=None, before_len=0, seg_start=None, segments=0,
                     lead_begin=0, open_end=-1, workspace=None, stream=None):
        """Enqueue the approx pass (acm_approx_matches_async) over caller-owned device planes: states
        (report=REPORT_STATE) or pattern indices (REPORT_HEAD).  An entry that is a piece of an approximate pattern
        (Automaton.add_approx) is kept where the whole pattern lies within its budget and no piece in front of this
        one is exact; every other entry is kept.  dist_out: None, or a third plane for the distances.  info: device
        int32[4].  workspace: (ptr, nbytes), or None for a temporary one that lives until the stream has passed it
        (the call then synchronises)."""
        st = stream if stream is not None else self.stream
        with self._workspace(workspace, st, self.lib.acm_approx_workspace_bytes, max_records) as (ws, nb):
            check(self.lib.acm_approx_matches_async(
                self.dfa, _ptr(pat_plane), _ptr(off_plane), max_records, report, _ptr(d_text), text_origin, text_end,
                _ptr(before), before_len, _ptr(seg_start), segments, lead_begin, open_end, _ptr(pat_out), _ptr(off_out),
                _ptr(dist_out), out_capacity, _ptr(info), _ptr(ws), nb, st), "acm_approx_matches_async")

    def scan_approx(self, text=None, texts=None, before=b"", init_state=0, out_capacity=None):
        """Matches of an automaton with approximate patterns (Automaton.add_approx): a REPORT_STATE scan, the
        segment pass when texts is given (each text matched alone), then the approx pass
        (acm_approx_matches_async).  text: host bytes; or None with texts: a list of bytes-like objects or a
        (uint8 array, int32 starts) pair.  before: the bytes in front of text, part of the same text.  The text
        ends with the bytes given.  Returns (pattern, end, dist, undecided) in record order: pattern is the index
        of an approximate pattern's FIRST piece, or a plain pattern's own; end the offset of the match's last
        byte (int64); dist the mismatches; undecided the candidates whose span left the bytes given."""
        with _Pipeline(self, "Matcher.scan_approx", text, texts, before=before) as p:
            ocap = out_capacity if out_capacity is not None else 8 * p.cap
            info = p.alloc(16)
            p.scan(init_state)
            if p.nseg:
                p.segment()
            d = p.approx(ocap, info, -p.before_len)
            off, pat, _, dist = p.download(p.count(), d)
            und = int(info.to_numpy(np.int32, 4, stream=self.stream)[0])
            return self.approx_first[pat], off.astype(np.int64) + self.approx_post[pat], dist, und

    def edit_async(self, pat_plane, off_plane, max_records, d_text, text_origin, text_end, pat_out, off_out,
                   out_capacity, info, dist_out=None, len_out=None, report=0, before=None, before_len=0, seg_start=None,
                   segments=0, lead_begin=0, open_end=-1, workspace=None, stream=None):
        """Enqueue the edit pass (acm_edit_matches_async) over caller-owned device planes: states
        (report=REPORT_STATE) or pattern indices (REPORT_HEAD).  A piece of an edit pattern (Automaton.add_edit)
        becomes the nearest end within edit distance k and the shortest span that has it; plain and Hamming
        entries become their normalised record.  The records are unique and ordered by (offset, pattern).
        dist_out, len_out: None, or planes for the distances and the span lengths.  info: device int32[4].  The
        pass orders max_records cells (times the longest match list for states): size it to the planes.
        workspace: (ptr, nbytes), or None for a temporary one that lives until the stream has passed it (the call
        then synchronises)."""
        st = stream if stream is not None else self.stream
        with self._workspace(workspace, st, self.lib.acm_edit_workspace_bytes, self.dfa, max_records) as (ws, nb):
            check(self.lib.acm_edit_matches_async(
                self.dfa, _ptr(pat_plane), _ptr(off_plane), max_records, report, _ptr(d_text), text_origin, text_end,
                _ptr(before), before_len, _ptr(seg_start), segments, lead_begin, open_end, _ptr(pat_out), _ptr(off_out),
                _ptr(dist_out), _ptr(len_out), out_capacity, _ptr(info), _ptr(ws), nb, st), "acm_edit_matches_async")

    def scan_edit(self, text=None, texts=None, before=b"", init_state=0, out_capacity=None):
        """Matches of an automaton with edit patterns (Automaton.add_edit): a REPORT_STATE scan, the segment pass
        when texts is given (each text matched alone), then the edit pass (acm_edit_matches_async) over the records
        the scan left.  Arguments as scan_approx.  Returns (pattern, end, dist, length, undecided), unique and
        ordered by (end, pattern): pattern is the index of an approximate pattern's FIRST piece, or a plain
        pattern's own; end the offset of the match's last byte (int64); dist the errors; length the bytes of the
        shortest span with that distance that ends there; undecided the candidates whose window left the bytes
        given."""
        with _Pipeline(self, "Matcher.scan_edit", text, texts, before=before) as p:
            info = p.alloc(16)
            p.scan(init_state)
            if p.nseg:
                p.segment()
            p.max_records = p.count()                  # the pass orders max_records cells: no more than there are
            ocap = out_capacity if out_capacity is not None else 8 * p.max_records + 2
            d, ln = p.edit(ocap, info, -p.before_len)
            off, pat, _, dist, length = p.download(p.count(), d, ln)
            und = int(info.to_numpy(np.int32, 4, stream=self.stream)[0])
            return pat, off.astype(np.int64), dist, length, und

    def sequence_async(self, pat_plane, off_plane, max_records, seq_out, off_out, out_capacity, info, seg_start=None,
                       segments=0, lead_begin=0, text_end=0, workspace=None, stream=None):
        """Enqueue the sequence pass (acm_sequence_matches_async) over caller-owned device planes of pattern
        indices, one record per occurrence (the all-patterns output of the expand, word, case or position
        pass): one record (sequence index, end offset) per match of a sequence (Automaton.add_sequence).
        info: device int32[4].  The pass orders max_records cells: size it to the planes.  workspace: (ptr,
        nbytes), or None for a temporary one that lives until the stream has passed it (the call then
        synchronises)."""
        st = stream if stream is not None else self.stream
        with self._workspace(workspace, st, self.lib.acm_sequence_workspace_bytes, self.dfa, max_records) as (ws, nb):
            check(self.lib.acm_sequence_matches_async(
                self.dfa, _ptr(pat_plane), _ptr(off_plane), max_records, _ptr(seg_start), segments, lead_begin, text_end,
                _ptr(seq_out), _ptr(off_out), out_capacity, _ptr(info), _ptr(ws), nb, st),
                "acm_sequence_matches_async")

    def scan_sequences(self, text=None, texts=None, lead_begin=0, init_state=0, before=b"", out_capacity=None):
        """Matches of the automaton's sequences (Automaton.add_sequence, add_signature): a REPORT_STATE scan,
        the segment pass when texts is given (each text matched alone), every pattern of every record (the
        case pass when the automaton is mixed, else acm_expand_matches_async), the wildcard pass when the
        automaton has wildcard contexts (the offsets returned are then the matches' ends: the last part's post
        context is added on the host), the position pass in its all
        form when the automaton is positioned (a window on the first part anchors the signature), then the
        sequence pass (acm_sequence_matches_async).  text: host bytes; or None with texts: a list of bytes-like
        objects or a (uint8 array, int32 starts) pair.  lead_begin: where the text in front of the first
        start began.  before: the bytes in front of text, for the case pass.  Returns (offsets, sequences,
        last_state, info): a record per match, the sequence index and the offset it ends at; info: [records
        that are a part, alive records over all levels, 0, 0].  A sequence whose parts lie in different calls
        is not joined: scan whole texts."""
        return self._sequences(text, texts, lead_begin, init_state, before, out_capacity, False)

    def _sequences(self, text, texts, lead_begin, init_state, before, out_capacity, rules):
        """scan_sequences, and with rules scan_rules: the rule pass over the sequence pass's planes"""
        lead_begin = int(lead_begin)
        with _Pipeline(self, "Matcher.scan_sequences", text, texts, before=before) as p:
            p.scan(init_state)
            if p.nseg:
                p.segment()
            p.every_pattern(8 * p.cap)
            p.max_records = n = p.count()          # from here on every stage is sized by the count in front of it
            info = p.alloc(16)
            if self.wild:
                p.wildcard(n + 2, info, True, lead_begin)
                p.max_records = n = p.count()
            if self.positioned:
                p.position(n + 2, info, True, lead_begin, p.n)
                p.max_records = n = p.count()
            p.sequence(out_capacity if out_capacity is not None and not rules else n + 2, info, lead_begin)
            p.max_records = m = p.count()
            if rules:
                text_plane = p.rule(out_capacity if out_capacity is not None else m + 2, info)
                offs, fired, _, of_text = p.download(p.count(), text_plane)
                return fired, of_text, offs, info.to_numpy(np.int32, 4, stream=self.stream)
            ends, seqs, last = p.download(m)
            if self.wild:   # the pass reports the end of the last part's anchor: the match ends post bytes behind it
                ends = (ends.astype(np.int64) + self.seq_post[seqs]).astype(np.uint32)
            return ends, seqs, last, info.to_numpy(np.int32, 4, stream=self.stream)

    def rule_async(self, seq_plane, off_plane, max_records, rule_out, text_out, off_out, out_capacity, info, seg_start=None,
                   segments=0, workspace=None, stream=None):
        """Enqueue the rule pass (acm_rule_matches_async) over caller-owned device planes of sequence indices
        and end offsets (the output of sequence_async): one record (rule index, text index or -1 for the lead
        text, offset of the trigger) per (rule, text) whose expression is true (Automaton.add_rule).  info: device
        int32[4].  The pass orders max_records cells: size it to the planes.  workspace: (ptr, nbytes), or None
        for a temporary one that lives until the stream has passed it (the call then synchronises)."""
        st = stream if stream is not None else self.stream
        with self._workspace(workspace, st, self.lib.acm_rule_workspace_bytes, self.dfa, max_records) as (ws, nb):
            check(self.lib.acm_rule_matches_async(
                self.dfa, _ptr(seq_plane), _ptr(off_plane), max_records, _ptr(seg_start), segments, _ptr(rule_out),
                _ptr(text_out), _ptr(off_out), out_capacity, _ptr(info), _ptr(ws), nb, st),
                "acm_rule_matches_async")

    def scan_rules(self, text=None, texts=None, lead_begin=0, init_state=0, before=b"", out_capacity=None):
        """The automaton's rules that hold (Automaton.add_rule, add_logical_signature): everything scan_sequences
        runs, then the rule pass (acm_rule_matches_async) over the sequence pass's planes.  text: host bytes, one
        text (index -1); or None with texts, as scan_sequences takes them: each text is matched and counted
        alone.  Returns (rules, texts, offsets, info): a record per (rule, text) whose expression is true, text
        by text: the rule index, the text index and the offset of the trigger record (with wildcard
        signatures: the end of its last part's anchor); info: [records that are an operand, (operand, text)
        pairs, (rule, text) pairs evaluated, 0].  Counts are not carried across calls: scan whole texts."""
        return self._sequences(text, texts, lead_begin, init_state, before, out_capacity, True)

    def select_async(self, pat_plane, off_plane, max_records, pat_out, off_out, out_capacity, info, start_out=None,
                     min_start=0, workspace=None, stream=None):
        """Enqueue the select pass (acm_select_matches_async) over caller-owned device planes of pattern indices,
        one record per occurrence (the all-patterns output of the expand, word, case, position or wildcard pass):
        the leftmost-longest non-overlapping matches, a record (pattern, offset of the anchor's end) each and in
        start_out, when given, where the match starts.  info: device int32[4]: eligible entries, entries that
        start in front of min_start, the cursor behind the last match (int64).  The pass orders max_records
        cells: size it to the planes.  workspace: (ptr, nbytes), or None for a temporary one that lives until
        the stream has passed it (the call then synchronises)."""
        st = stream if stream is not None else self.stream
        with self._workspace(workspace, st, self.lib.acm_select_workspace_bytes, max_records) as (ws, nb):
            check(self.lib.acm_select_matches_async(
                self.dfa, _ptr(pat_plane), _ptr(off_plane), max_records, min_start, 0, _ptr(pat_out), _ptr(off_out),
                _ptr(start_out), out_capacity, _ptr(info), _ptr(ws), nb, st), "acm_select_matches_async")

    def _select_stages(self, p, init_state, info, out_capacity):
        """the stages of scan_select on the pipeline p, up to and with the select pass into planes of out_capacity
        cells (None: what the entries in front of it need); returns the plane of the matches' starts"""
        lead = -p.before_len
        p.scan(init_state)
        if p.nseg:
            p.segment()
        p.every_pattern(8 * p.cap)
        p.max_records = n = p.count()          # from here on every stage is sized by the count in front of it
        if self.wild:
            p.wildcard(n + 2, info, True, lead)
            p.max_records = n = p.count()
        if self.positioned:
            p.position(n + 2, info, True, lead, p.n)
            p.max_records = n = p.count()
        return p.select(out_capacity if out_capacity is not None else n + 2, info, lead)

    def scan_select(self, text=None, texts=None, before=b"", init_state=0, out_capacity=None):
        """The leftmost-longest non-overlapping matches of the pattern set, what grep -o prints for a list of
        fixed strings: a REPORT_STATE scan, the segment pass when texts is given (each text matched alone), every
        pattern of every record (the case pass when the automaton is mixed, else acm_expand_matches_async), the
        wildcard pass when the automaton has wildcard contexts, the position pass in its all form when it is
        positioned, then the select pass (acm_select_matches_async).  text: host bytes; or None with texts: a
        list of bytes-like objects or a (uint8 array, int32 starts) pair.  before: the bytes in front of text,
        part of the same text: a match may start in them.  Returns (offsets, patterns, starts, info): a record
        per match, the offset its anchor ends at (a wildcard match ends Automaton.wildcard_lengths(p)[1] bytes
        behind), its pattern and where it starts (int32: negative inside before); info: [eligible entries,
        entries that start in front of before, cursor lo, cursor hi].  A selection is not continued across
        calls: scan whole texts."""
        with _Pipeline(self, "Matcher.scan_select", text, texts, before=before) as p:
            info = p.alloc(16)
            start = self._select_stages(p, init_state, info, out_capacity)
            offs, pats, _, starts = p.download(p.count(), start)
            return offs, pats, starts, info.to_numpy(np.int32, 4, stream=self.stream)

    def rewrite_async(self, d_text, n, pat_plane, off_plane, max_records, out, out_capacity, info, text_origin=0,
                      at_out=None, at_capacity=0, seg_start=None, segments=0, seg_out=None, workspace=None, stream=None):
        """Enqueue the rewrite pass (acm_rewrite_async): the device text d_text[0, n) (the byte at offset
        text_origin + i in d_text[i]) with the span of every record of the select pass's planes replaced by its
        pattern's replacement (Automaton.set_replacement), into out (16-byte aligned, out_capacity bytes; None
        with 0: only the figures).  info: device int32[8]: used and skipped records, the output's length (int64),
        the input bytes inside used spans (int64), 1 if the output was cut at out_capacity, 0.  at_out: a plane
        of at_capacity cells: where every used record's replacement begins in the output; seg_start and seg_out,
        int32[segments] each: where every start lies in the output.  workspace: (ptr, nbytes), or None for a
        temporary one that lives until the stream has passed it (the call then synchronises)."""
        st = stream if stream is not None else self.stream
        with self._workspace(workspace, st, self.lib.acm_rewrite_workspace_bytes, max_records, segments) as (ws, nb):
            check(self.lib.acm_rewrite_async(
                self.dfa, _ptr(d_text), n, text_origin, _ptr(pat_plane), _ptr(off_plane), max_records, _ptr(out),
                out_capacity, _ptr(at_out), at_capacity, _ptr(seg_start), segments, _ptr(seg_out), _ptr(info), _ptr(ws),
                nb, st), "acm_rewrite_async")

    def scan_rewrite(self, text=None, texts=None, before=b"", init_state=0, out_capacity=None):
        """The text with every leftmost-longest non-overlapping match replaced by its pattern's replacement
        (Automaton.set_replacement; a pattern without one: the match as it is): exactly the stages of scan_select,
        then the rewrite pass (acm_rewrite_async) over before + text.  Returns (out_bytes, info, at, seg_out): the
        rewritten before + text; info int32[8] as rewrite_async leaves it; at: per match, where its replacement
        begins in the output; seg_out: per text, where it begins in the output (None without texts).  out_capacity:
        the room for the output in bytes; by default the text's length plus the growth of the longest replacement
        for every selected match.  An output that does not fit is ACM_ERR_CAPACITY, never cut silently."""
        with _Pipeline(self, "Matcher.scan_rewrite", text, texts, before=before) as p:
            lead = -p.before_len
            info = p.alloc(32)
            self._select_stages(p, init_state, info, None)
            p.max_records = n = p.count()
            whole, total = p.d, p.n
            if p.before_len:                                   # the rewrite reads one text: before and text, joined
                total = p.before_len + p.n
                whole = p.upload(np.concatenate([p.bf, p.t]))
            cap = out_capacity if out_capacity is not None else min(total + n * self.max_growth, 2 ** 31 - 17)
            out, at, seg = p.rewrite(info, cap, whole, total, lead, n + 2)
            res = info.to_numpy(np.int32, 8, stream=self.stream)
            if res[6]:
                raise AcmError(_lib.ACM_ERR_CAPACITY, p.where, "the output has %d bytes but the buffer holds %d" % (
                    (int(res[3]) << 32) | (int(res[2]) & 0xFFFFFFFF), cap))
            m = min((int(res[3]) << 32) | (int(res[2]) & 0xFFFFFFFF), cap)
            data = out.to_numpy(np.uint8, m, stream=self.stream).tobytes()
            used = int(res[0])
            at_cells = at.to_numpy(np.int32, used + 2, stream=self.stream)[1:1 + used].copy()
            seg_cells = seg.to_numpy(np.int32, p.nseg, stream=self.stream) if seg is not None else None
            return data, res, at_cells, seg_cells

    @staticmethod
    def blank_mask(blank_set):
        """32-byte mask (bit b % 8 of byte b // 8: byte b is blank) of an iterable of byte values or a bytes-like
        object; None stays None (the default set: tab, LF, VT, FF, CR, space)."""
        if blank_set is None:
            return None
        m = bytearray(32)
        for b in bytes(blank_set) if isinstance(blank_set, (bytes, bytearray, memoryview)) else blank_set:
            m[int(b) >> 3] |= 1 << (int(b) & 7)
        return bytes(m)

    def normalize_async(self, d_text, n, flags, out, out_capacity, keep, block, info, blank_mask=None, blank_byte=0x20,
                        text_origin=0, seg_start=None, segments=0, seg_out=None, workspace=None, stream=None):
        """Enqueue the normalise pass (acm_normalize_async): the device text d_text[0, n) with percent triples decoded
        (NORM_PERCENT) and blank units squeezed to blank_byte (NORM_SQUEEZE) or dropped (NORM_STRIP), into out (16-byte
        aligned, out_capacity bytes; None with 0: only the figures).  keep: device uint64[ceil(n / 64)], a bit per
        byte that emits; block: device int32[ceil(n / 1024) + 1], the output in front of every 1024 input bytes: the
        offset map.  blank_mask: 32 host bytes (Matcher.blank_mask) or None for the default set.  info: device
        int32[8]: m, units dropped, triples, blank units emitted, 1 if the output was cut, 0s.  seg_start and
        seg_out, int32[segments] each: the text starts, and where every text begins in the output.  workspace: (ptr,
        nbytes), or None for a temporary one that lives until the stream has passed it (the call then synchronises)."""
        st = stream if stream is not None else self.stream
        with self._workspace(workspace, st, self.lib.acm_normalize_workspace_bytes, n, segments) as (ws, nb):
            check(self.lib.acm_normalize_async(
                _ptr(d_text), n, text_origin, flags, blank_mask, blank_byte, _ptr(out), out_capacity, _ptr(keep),
                _ptr(block), _ptr(seg_start), segments, _ptr(seg_out), _ptr(info), _ptr(ws), nb, st), "acm_normalize_async")

    def normalize_remap_async(self, d_text, n, flags, keep, block, off_plane, max_records, off_out, info, pat_plane=None,
                              start_out=None, text_origin=0, stream=None):
        """Enqueue the remap pass (acm_normalize_remap_async): records whose offsets lie in the normalised text become
        offsets into the text the normalise call read.  d_text, n, flags, text_origin, keep and block are that
        call's.  off_out (it may be off_plane): where every record's last emitting unit ends; with pat_plane and
        start_out: where the match starts.  Unmapped cells are -1; info: device int32[8]: records, records with an
        unmapped cell, 0s."""
        st = stream if stream is not None else self.stream
        check(self.lib.acm_normalize_remap_async(
            self.dfa, _ptr(d_text), n, text_origin, flags, _ptr(keep), _ptr(block), _ptr(pat_plane), _ptr(off_plane),
            max_records, _ptr(off_out), _ptr(start_out), _ptr(info), st), "acm_normalize_remap_async")

    def scan_normalized(self, text=None, texts=None, percent=False, squeeze=False, strip=False, blank_set=None,
                        blank_byte=0x20, all_patterns=False, out_capacity=None):
        """Matches against a normalised view of the input, reported on the input: the normalise pass
        (acm_normalize_async: percent triples decoded, blanks squeezed to blank_byte or stripped), an ordinary scan of
        the normalised text, the segment pass over the normalised texts when texts is given (no match spans two
        texts, normalised or not), the case pass for a mixed automaton or with all_patterns every pattern of every
        record, then the remap (acm_normalize_remap_async).  text: host bytes; or None with texts: a list of
        bytes-like objects or a (uint8 array, int32 starts) pair.  blank_set: the blank bytes (None: tab, LF, VT,
        FF, CR, space).  Returns (patterns, starts, ends, m): per match its pattern and the first and last byte of
        the input it covers (int32, in the coordinates of the input or of the concatenation), and the normalised
        length.  The scan's length is a host argument and m lives on the device: the host waits once between
        normalise and scan to read it.  out_capacity: the room for the normalised text (by default the input's
        length, which always suffices); a text that does not fit is ACM_ERR_CAPACITY."""
        flags = (_lib.NORM_PERCENT if percent else 0) | (_lib.NORM_SQUEEZE if squeeze else 0) | (_lib.NORM_STRIP if strip else 0)
        with _Pipeline(self, "Matcher.scan_normalized", text, texts) as p:
            m = int(p.normalize(flags, self.blank_mask(blank_set), blank_byte, out_capacity)[0])
            none = np.zeros(0, dtype=np.int32)
            if m == 0:
                return none, none, none, 0
            info = p.alloc(32)
            if all_patterns or self.mixed:
                p.scan()
                if p.nseg:
                    p.segment()
                if all_patterns:
                    p.every_pattern(8 * p.cap)
                else:
                    p.case(p.cap, False)
            elif p.nseg:
                p.scan()
                p.segment(_lib.REPORT_HEAD)
            else:
                p.scan(report=_lib.REPORT_HEAD)
            p.max_records = n = p.count()
            start = p.normalize_remap(info)
            ends, pats, _, starts = p.download(n, start)
            return pats, starts, ends.astype(np.int32), m

    def tally_async(self, pat_plane, off_plane, max_records, class_total, report=0, all_patterns=False,
                    accumulate=False, class_of=None, num_classes=None, seg_start=None, segments=0, seg_class=None,
                    lead=None, workspace=None, stream=None):
        """Enqueue the tally pass (acm_tally_matches_async) over caller-owned device planes: entries per
        class into class_total (uint64[num_classes]), per (segment, class) into seg_class
        (int32[segments, num_classes]) and of the records in front of the first start into lead
        (int32[num_classes]).  class_of: device int32[num_patterns] or None for the identity (num_classes
        then defaults to the number of patterns).  workspace: (ptr, nbytes), or None for a temporary one
        that lives until the stream has passed it (the call then synchronises)."""
        st = stream if stream is not None else self.stream
        if num_classes is None:
            if class_of is not None:
                raise ValueError("num_classes is needed with a class map")
            num_classes = self.num_patterns
        flags = (_lib.TALLY_ACCUMULATE if accumulate else 0) | (_lib.TALLY_ALL_PATTERNS if all_patterns else 0)
        with self._workspace(workspace, st, self.lib.acm_tally_workspace_bytes, max_records, num_classes) as (ws, nb):
            check(self.lib.acm_tally_matches_async(
                self.dfa, _ptr(pat_plane), _ptr(off_plane), max_records, report, flags, _ptr(class_of), num_classes,
                _ptr(seg_start), segments, _ptr(class_total), _ptr(seg_class), _ptr(lead), _ptr(ws), nb, st),
                "acm_tally_matches_async")

    def scan_tally(self, texts, class_of=None, num_classes=None, all_patterns=False, per_text=True, init_state=0):
        """Count instead of list: scan, clamp every record to its own text when there are several
        (acm_segment_matches_async), tally on the device (acm_tally_matches_async) and download only the
        tallies.  texts: a list of bytes-like objects or a (uint8 array, int32 starts) pair, as
        scan_segments takes them, or one bytes-like / uint8 array with no segments.  class_of: int32 class
        of every pattern (class_map), None for one class per pattern; num_classes defaults to
        max(class_of) + 1.  all_patterns: count every pattern that ends at an offset, else the one the
        scan reports.  Returns (class_total uint64[C], seg_class int32[S, C] or None, lead int32[C],
        last_state); seg_class is None without segments or with per_text=False."""
        cmap = None
        if class_of is not None:
            cmap = np.ascontiguousarray(class_of, dtype=np.int32)
            if cmap.size != self.num_patterns:
                raise ValueError("class_of has %d entries for %d patterns" % (cmap.size, self.num_patterns))
            if num_classes is None:
                num_classes = max(int(cmap.max()) + 1, 1) if cmap.size else 1
        elif num_classes is None:
            num_classes = self.num_patterns
        ncls = int(num_classes)
        several = isinstance(texts, (list, tuple))
        with _Pipeline(self, "Matcher.scan_tally", None if several else texts, texts if several else None) as p:
            nseg = p.nseg
            ws = p.workspace(self.lib.acm_tally_workspace_bytes, p.max_records, ncls)
            tot, lead = p.alloc(max(ncls * 8, 16)), p.alloc(max(ncls * 4, 16))
            d_map = rows = None
            if cmap is not None:
                d_map = p.upload(cmap, pad_to=0) if cmap.size else p.alloc(16)
            if per_text and nseg:
                rows = p.alloc(max(nseg * ncls * 4, 16))
            p.scan(init_state)
            if nseg:
                p.segment()
            self.tally_async(p.pat, p.off, p.max_records, tot, report=_lib.REPORT_STATE, all_patterns=all_patterns,
                             class_of=d_map, num_classes=ncls, seg_start=p.d_st, segments=nseg, seg_class=rows,
                             lead=lead, workspace=ws)
            m = p.count()
            last = int(p.pat.to_numpy(np.int32, 1, offset_bytes=4 * (m + 1), stream=self.stream)[0])
            seg_class = rows.to_numpy(np.int32, nseg * ncls, stream=self.stream).reshape(nseg, ncls) \
                if rows is not None else None
            return (tot.to_numpy(np.uint64, ncls, stream=self.stream), seg_class,
                    lead.to_numpy(np.int32, ncls, stream=self.stream), last)

    def line_index_async(self, d_text, n, line_start, capacity, info, text_origin=0, delimiter=b"\n", prev_byte=-1,
                         prev_info=None, workspace=None, stream=None):
        """Enqueue the line index (acm_line_index_async) over device text: the line starts into line_start
        (int32[capacity], INT32_MAX behind them: a valid seg_start for the segment, word and tally
        passes) and the counts into info (int32[8]).  prev_info: the info of the piece in front, on the
        device.  workspace: (ptr, nbytes), or None for a temporary one (the call then synchronises)."""
        st = stream if stream is not None else self.stream
        d = delimiter[0] if isinstance(delimiter, (bytes, bytearray)) else int(delimiter)
        with self._workspace(workspace, st, self.lib.acm_line_index_workspace_bytes, n) as (ws, nb):
            check(self.lib.acm_line_index_async(_ptr(d_text), n, text_origin, d, prev_byte, _ptr(prev_info),
                                                _ptr(line_start), capacity, _ptr(info), _ptr(ws), nb, st),
                  "acm_line_index_async")

    def line_number_async(self, line_start, capacity, info, offsets, count, line_out, d_count=None, stream=None):
        """Enqueue acm_line_number_async: delimiters in front of each of count device offsets (of at most
        *d_count of them when d_count is given: a plane's header cell) into line_out."""
        st = stream if stream is not None else self.stream
        check(self.lib.acm_line_number_async(_ptr(line_start), capacity, _ptr(info), _ptr(offsets), _ptr(d_count), count,
                                             _ptr(line_out), st), "acm_line_number_async")

    def line_select_async(self, line_start, capacity, info, text_origin, text_end, off_plane, max_records, rel_out,
                          begin_out, next_out, out_capacity, invert=False, workspace=None, stream=None):
        """Enqueue acm_line_select_async: the lines that hold a record of off_plane (invert: that hold
        none) as (delimiters in front, first byte, first byte behind) planes in the scan's cell layout.
        workspace: (ptr, nbytes), or None for a temporary one (the call then synchronises)."""
        st = stream if stream is not None else self.stream
        with self._workspace(workspace, st, self.lib.acm_line_select_workspace_bytes, capacity) as (ws, nb):
            check(self.lib.acm_line_select_async(_ptr(line_start), capacity, _ptr(info), text_origin, text_end,
                                                 _ptr(off_plane), max_records, 1 if invert else 0, _ptr(rel_out),
                                                 _ptr(begin_out), _ptr(next_out), out_capacity, _ptr(ws), nb, st),
                  "acm_line_select_async")

    def scan_lines(self, text, delimiter=b"\n", per_line=False, all_patterns=False, invert=False, init_state=0):
        """grep -n: scan host bytes, find the lines on the device (acm_line_index_async), number every
        record's line (acm_line_number_async) and list the lines that hold a record, or with invert the
        others (acm_line_select_async).  per_line: the device-made index goes to the segment pass first,
        so no match spans two lines.  all_patterns: every pattern that ends at an offset.  Nothing is
        split on the host.  A convenience call: a text of n bytes may have n lines, so the starts and the
        three select planes are sized for that (about 16 bytes of device memory per text byte besides the
        record planes, 0.6 GB for 32 MiB), allocated and freed on every call; a caller who knows a bound on
        its lines uses the three *_async calls with its own buffers.  Returns (patterns int32[], offsets
        uint32[], lines int64[] 1-based,
        selected int64[k, 3] of (1-based line, first byte, first byte behind), number of lines)."""
        with _Pipeline(self, "Matcher.scan_lines", text) as pl:
            n, lcap = pl.n, pl.n + 1
            idx_ws = self.lib.acm_line_index_workspace_bytes(n)
            sel_ws = self.lib.acm_line_select_workspace_bytes(lcap)
            starts, info, ws = pl.alloc(lcap * 4), pl.alloc(32), pl.alloc(max(idx_ws, sel_ws))
            pl.scan(init_state, _lib.REPORT_STATE if per_line or all_patterns else _lib.REPORT_HEAD)
            self.line_index_async(pl.d, n, starts, lcap, info, delimiter=delimiter, workspace=(ws.ptr, idx_ws))
            if per_line:
                pl.segment(_lib.REPORT_STATE if all_patterns else _lib.REPORT_HEAD, seg_start=starts, segments=lcap)
            if all_patterns:
                pl.expand(8 * pl.cap)
            pat, off, records = pl.pat, pl.off, pl.max_records
            num, rel, beg, nxt = [pl.alloc(pl.room * 4)] + pl.planes(lcap + 2, 3)
            self.line_number_async(starts, lcap, info, off.ptr + 4, records, num, d_count=off)
            self.line_select_async(starts, lcap, info, 0, n, off, records, rel, beg, nxt, lcap + 2, invert=invert,
                                   workspace=(ws.ptr, sel_ws))
            m = pl.count()
            h_info = info.to_numpy(np.int32, 8, stream=self.stream)
            first = 1 + (int(np.uint32(h_info[4])) | int(np.uint32(h_info[5])) << 32)
            p = pat.to_numpy(np.int32, m + 1, stream=self.stream)[1:]
            o = off.to_numpy(np.int32, m + 1, stream=self.stream)[1:].astype(np.uint32)
            ln = num.to_numpy(np.int32, m, stream=self.stream).astype(np.int64) + first
            k = int(rel.to_numpy(np.int32, 1, stream=self.stream)[0])
            sel = np.stack([rel.to_numpy(np.int32, k + 1, stream=self.stream)[1:].astype(np.int64) + first,
                            beg.to_numpy(np.int32, k + 1, stream=self.stream)[1:].astype(np.int64),
                            nxt.to_numpy(np.int32, k + 1, stream=self.stream)[1:].astype(np.int64)], axis=1)
            lines = int(h_info[0]) + (1 if n and not h_info[2] else 0)
            return p.copy(), o, ln, sel, lines

    def line_context_async(self, line_start, capacity, info, text_origin, text_end, off_plane, max_records, rel_out,
                           begin_out, next_out, out_capacity, ctx_info, before=0, after=0, invert=False, lines_out=None,
                           seg_start=None, segments=0, workspace=None, stream=None):
        """Enqueue acm_line_context_async: the lines that hold a record of off_plane (invert: that hold none)
        with before lines in front of and after lines behind each, merged into groups that never cross a start
        of seg_start: (delimiters in front, first byte, first byte behind, lines) planes in the scan's cell
        layout, and ctx_info (int32[4]: selected lines, kept lines, groups, 0).  workspace: (ptr, nbytes), or
        None for a temporary one (the call then synchronises)."""
        st = stream if stream is not None else self.stream
        with self._workspace(workspace, st, self.lib.acm_line_context_workspace_bytes, capacity, segments) as (ws, nb):
            check(self.lib.acm_line_context_async(
                _ptr(line_start), capacity, _ptr(info), text_origin, text_end, _ptr(off_plane), max_records,
                1 if invert else 0, before, after, _ptr(seg_start), segments, _ptr(rel_out), _ptr(begin_out),
                _ptr(next_out), _ptr(lines_out), out_capacity, _ptr(ctx_info), _ptr(ws), nb, st), "acm_line_context_async")

    def extract_async(self, d_text, n, begin_plane, end_plane, max_ranges, out, out_capacity, info, text_origin=0,
                      end_inclusive=False, glue=b"", terminator=-1, at_out=None, at_capacity=0, seg_start=None, segments=0,
                      seg_out=None, workspace=None, stream=None):
        """Enqueue the extract pass (acm_extract_async): the ranges [begin, end) of the two planes (end_inclusive:
        [begin, end]) of the device text d_text[0, n), gathered in input order into out (16-byte aligned,
        out_capacity bytes; None with 0: only the figures), glue (host bytes, at most 16) between ranges of one
        text and terminator (a byte value, -1: none) behind a range that does not end in it.  info: device
        int32[8]: used and skipped ranges, the output's length (int64), the text bytes copied (int64), 1 if the
        output was cut at out_capacity, terminators appended.  at_out: a plane of at_capacity cells: where every
        used range's bytes begin in the output; seg_start and seg_out, int32[segments] each: the output of the
        ranges in front of every start.  workspace: (ptr, nbytes), or None for a temporary one that lives until
        the stream has passed it (the call then synchronises)."""
        st = stream if stream is not None else self.stream
        glue = bytes(glue)
        term = terminator[0] if isinstance(terminator, (bytes, bytearray)) else int(terminator)
        with self._workspace(workspace, st, self.lib.acm_extract_workspace_bytes, max_ranges, segments) as (ws, nb):
            check(self.lib.acm_extract_async(
                _ptr(d_text), n, text_origin, _ptr(begin_plane), _ptr(end_plane), max_ranges,
                _lib.EXTRACT_END_INCLUSIVE if end_inclusive else 0, glue if glue else None, len(glue), term, _ptr(out),
                out_capacity, _ptr(at_out), at_capacity, _ptr(seg_start), segments, _ptr(seg_out), _ptr(info), _ptr(ws),
                nb, st), "acm_extract_async")

    def _packed_prologue(self, delimiter, terminator, before, after, only_matching):
        """What scan_extract and scan_format check first: (the delimiter's byte, the terminator's byte)."""
        d = delimiter[0] if isinstance(delimiter, (bytes, bytearray)) else int(delimiter)
        if only_matching and self.wild:
            raise ValueError("only_matching needs an automaton without wildcard contexts: a match there ends "
                             "behind its record's offset")
        if before < 0 or after < 0:
            raise ValueError("before and after are >= 0")
        term = d if terminator is None else (terminator[0] if isinstance(terminator, (bytes, bytearray)) else int(terminator))
        return d, term

    def _packed_results(self, pl, info, cap, out, at, seg):
        """What scan_extract and scan_format read back behind the packing pass: (the output's bytes, where every used
        range's bytes begin, info, seg_out or None); ACM_ERR_CAPACITY for an output of more than cap bytes."""
        res = info.to_numpy(np.int32, 8, stream=self.stream)
        m = (int(np.uint32(res[3])) << 32) | int(np.uint32(res[2]))
        if res[6]:
            raise AcmError(_lib.ACM_ERR_CAPACITY, pl.where, "the output has %d bytes but the buffer holds %d" % (m, cap))
        data = out.to_numpy(np.uint8, m, stream=self.stream).tobytes()
        used = int(res[0])
        at_cells = at.to_numpy(np.int32, used + 2, stream=self.stream)[1:1 + used].copy()
        seg_cells = seg.to_numpy(np.int32, pl.nseg, stream=self.stream) if seg is not None else None
        return data, at_cells, res, seg_cells

    def scan_extract(self, text=None, texts=None, delimiter=b"\n", before=0, after=0, invert=False, per_line=False,
                     only_matching=False, glue=None, terminator=None, init_state=0, out_capacity=None):
        """grep's output on the device: the lines that hold a match (invert: that hold none) with before lines in
        front of and after lines behind each, packed into one output.  The stages of scan_lines (per_line: the
        device-made line index goes to the segment pass first), then the context pass (acm_line_context_async) and
        the extract (acm_extract_async).  text: host bytes; or None with texts: a list of bytes-like objects or a
        (uint8 array, int32 starts) pair: each text matched alone, context and glue never cross into another
        text.  glue: the bytes between two groups of one text, by default b"--" + delimiter when before + after >
        0, else none; terminator: the byte appended to a group that does not end in it, by default the delimiter
        (-1: none).  only_matching: the stages of scan_select, then the extract over the matches themselves
        (grep -o's bytes: no glue, the terminator behind every match that does not end in it); ValueError for an
        automaton with wildcard contexts, whose matches end behind their offsets.
        Returns (out_bytes, groups, at, info, seg_out): groups int64[k, 4] of (1-based line, first byte, first byte
        behind, lines) per group (only_matching: (0, start, end, 0) per match); at: where every group's bytes
        begin in the output; info int32[8] as extract_async leaves it; seg_out: per text, where its part of the
        output begins (None without texts).  out_capacity: the room for the output in bytes; by default a bound
        that always fits: every kept line costs its bytes and at most one terminator, every group at most one
        glue, a text of n bytes has at most n + 1 lines: n + (n + 1) * (1 + len(glue)); for only_matching n + the
        records.  A convenience call, sized for the worst case as scan_lines is; a caller who knows better uses
        the *_async calls with its own buffers.  An output that does not fit is ACM_ERR_CAPACITY, never cut
        silently."""
        d, term = self._packed_prologue(delimiter, terminator, before, after, only_matching)
        with _Pipeline(self, "Matcher.scan_extract", text, texts) as pl:
            n, info = pl.n, pl.alloc(32)
            if only_matching:
                sel_info = pl.alloc(16)
                start = self._select_stages(pl, init_state, sel_info, None)
                pl.max_records = k = pl.count()
                g = b""
                cap = out_capacity if out_capacity is not None else min(n + k, 2 ** 31 - 17)
                begin, end, ranges, incl = start, pl.off, k, True
                grp = None
            else:
                g = (b"--" + bytes([d]) if before + after > 0 else b"") if glue is None else bytes(glue)
                lcap = n + 1
                idx_ws = self.lib.acm_line_index_workspace_bytes(n)
                ctx_ws = self.lib.acm_line_context_workspace_bytes(lcap, pl.nseg)
                starts, linfo, ws, cinfo = pl.alloc(lcap * 4), pl.alloc(32), pl.alloc(max(idx_ws, ctx_ws)), pl.alloc(16)
                pl.scan(init_state, _lib.REPORT_STATE if per_line or pl.nseg else _lib.REPORT_HEAD)
                self.line_index_async(pl.d, n, starts, lcap, linfo, delimiter=d, workspace=(ws.ptr, idx_ws))
                if pl.nseg:
                    pl.segment(_lib.REPORT_STATE if per_line else _lib.REPORT_HEAD)
                if per_line:
                    pl.segment(_lib.REPORT_HEAD, seg_start=starts, segments=lcap)
                rel, beg, nxt, cnt = pl.line_context(starts, lcap, linfo, cinfo, before, after, invert, (ws.ptr, ctx_ws))
                cap = out_capacity if out_capacity is not None else min(n + lcap * (1 + len(g)), 2 ** 31 - 17)
                begin, end, ranges, incl = beg, nxt, lcap, False
                grp = (rel, beg, nxt, cnt)
            packed = pl.extract(begin, end, ranges, info, cap, g, term, incl)
            data, at_cells, res, seg_cells = self._packed_results(pl, info, cap, *packed)
            if grp is None:
                k = ranges
                s = begin.to_numpy(np.int32, k + 1, stream=self.stream)[1:].astype(np.int64)
                e = end.to_numpy(np.int32, k + 1, stream=self.stream)[1:].astype(np.int64) + 1
                groups = np.stack([np.zeros(k, dtype=np.int64), s, e, np.zeros(k, dtype=np.int64)], axis=1)
            else:
                h = linfo.to_numpy(np.int32, 8, stream=self.stream)
                first = 1 + (int(np.uint32(h[4])) | int(np.uint32(h[5])) << 32)
                k = int(grp[0].to_numpy(np.int32, 1, stream=self.stream)[0])
                cols = [x.to_numpy(np.int32, k + 1, stream=self.stream)[1:].astype(np.int64) for x in grp]
                cols[0] = cols[0] + first
                groups = np.stack(cols, axis=1) if k else np.zeros((0, 4), dtype=np.int64)
            return data, groups, at_cells, res, seg_cells

    def line_context_lines_async(self, line_start, capacity, info, text_origin, text_end, off_plane, max_records, rel_out,
                                 begin_out, next_out, kind_out, out_capacity, ctx_info, before=0, after=0, invert=False,
                                 seg_start=None, segments=0, workspace=None, stream=None):
        """Enqueue acm_line_context_lines_async: line_context_async's lines, one entry per KEPT line instead of one per
        group: (delimiters in front, first byte, first byte behind, kind) planes in the scan's cell layout, kind
        being LINE_SELECTED | LINE_GROUP_HEAD, and ctx_info (int32[4]: selected lines, kept lines, groups, 0).
        workspace: (ptr, nbytes), or None for a temporary one (the call then synchronises)."""
        st = stream if stream is not None else self.stream
        with self._workspace(workspace, st, self.lib.acm_line_context_lines_workspace_bytes, capacity, segments) as (ws, nb):
            check(self.lib.acm_line_context_lines_async(
                _ptr(line_start), capacity, _ptr(info), text_origin, text_end, _ptr(off_plane), max_records,
                1 if invert else 0, before, after, _ptr(seg_start), segments, _ptr(rel_out), _ptr(begin_out),
                _ptr(next_out), _ptr(kind_out), out_capacity, _ptr(ctx_info), _ptr(ws), nb, st),
                "acm_line_context_lines_async")

    def format_async(self, d_text, n, begin_plane, end_plane, max_ranges, out, out_capacity, info, text_origin=0,
                     end_inclusive=False, kind_plane=None, num_plane=None, seg_num=None, number=False, offset=False,
                     number_base=1, offset_base=0, sel_sep=b":", ctx_sep=b"-", names=None, name_off=None, names_bytes=0,
                     glue=b"", terminator=-1, at_out=None, at_capacity=0, seg_start=None, segments=0, seg_out=None,
                     workspace=None, stream=None):
        """Enqueue the format pass (acm_format_async): extract_async with a prefix in front of every range's bytes.
        names and name_off (device uint8[names_bytes] and int32[segments + 2]): the name of every text id, printed
        when given; number: print number_base + num_plane's cell (less seg_num's cell of the range's text, device
        int32[segments]); offset: print offset_base + the range's first byte relative to its text; behind each of
        them sel_sep for a range whose kind_plane cell has LINE_SELECTED (no kind_plane: every range), else ctx_sep.
        glue goes in front of a range with LINE_GROUP_HEAD that follows a range of the same text.  Everything else
        is extract_async's."""
        st = stream if stream is not None else self.stream
        glue = bytes(glue)
        byte = lambda v: v[0] if isinstance(v, (bytes, bytearray)) else int(v)
        flags = (_lib.EXTRACT_END_INCLUSIVE if end_inclusive else 0) | (_lib.FORMAT_NAME if names is not None else 0) | \
            (_lib.FORMAT_NUMBER if number else 0) | (_lib.FORMAT_OFFSET if offset else 0)
        with self._workspace(workspace, st, self.lib.acm_format_workspace_bytes, max_ranges, segments) as (ws, nb):
            check(self.lib.acm_format_async(
                _ptr(d_text), n, text_origin, _ptr(begin_plane), _ptr(end_plane), max_ranges, flags, _ptr(kind_plane),
                _ptr(num_plane), _ptr(seg_num), number_base, offset_base, byte(sel_sep), byte(ctx_sep), _ptr(names),
                _ptr(name_off), names_bytes, glue if glue else None, len(glue), byte(terminator), _ptr(out), out_capacity,
                _ptr(at_out), at_capacity, _ptr(seg_start), segments, _ptr(seg_out), _ptr(info), _ptr(ws), nb, st),
                "acm_format_async")

    def scan_format(self, text=None, texts=None, names=None, with_name=False, line_number=False, byte_offset=False,
                    before=0, after=0, invert=False, per_line=False, only_matching=False, glue=None, terminator=None,
                    out_capacity=None, delimiter=b"\n", init_state=0):
        """grep -H -n -b on the device: scan_extract's output with `name:line:offset:` in front of every selected
        line and `name-line-offset-` in front of every context line.  The stages of scan_extract with the per-line
        context pass (acm_line_context_lines_async) and the format pass (acm_format_async) in the place of the
        group form and the extract.  names: one bytes per text (one for text), printed with with_name;
        line_number: the 1-based line in its text; byte_offset: the line's first byte in its text.  The glue goes
        between two groups of one text only.  only_matching: the stages of scan_select, acm_line_number_async
        over the matches' starts, then the format pass over the matches (grep -o -n -b: the line and the offset of
        the match itself); ValueError for an automaton with wildcard contexts, as scan_extract.
        Returns (out_bytes, lines, at, info, seg_out): lines int64[k, 4] of (1-based line in the call, first byte,
        first byte behind, kind) per kept line (only_matching: (line, start, end, LINE_SELECTED) per match); at:
        where every line's bytes begin in the output, behind its prefix; info and seg_out as extract_async leaves
        them.  out_capacity: by default a bound that always fits: scan_extract's, and for every line the longest
        prefix this text can have (the longest name, the digits of n + 1, a separator each).  An output that does
        not fit is ACM_ERR_CAPACITY, never cut silently."""
        d, term = self._packed_prologue(delimiter, terminator, before, after, only_matching)
        with _Pipeline(self, "Matcher.scan_format", text, texts) as pl:
            n, info, lcap = pl.n, pl.alloc(32), pl.n + 1
            table = None
            if with_name:
                given = [bytes(x) for x in (names if names is not None else [])]
                if len(given) != max(pl.nseg, 1) or any(len(x) > _lib.FORMAT_MAX_NAME for x in given):
                    raise ValueError("with_name needs one name per text, of at most %d bytes each" % _lib.FORMAT_MAX_NAME)
                table = ([b""] if pl.nseg else []) + given      # text id 0: what lies in front of the first start
            widest = (max(len(x) for x in table) + 1 if table else 0) + \
                ((len(str(n + 1)) + 1) if line_number else 0) + ((len(str(n)) + 1) if byte_offset else 0)
            prefix = dict(number=line_number, offset=byte_offset)
            if table:
                off = np.concatenate([[0], np.cumsum([len(x) for x in table])]).astype(np.int32)
                blob = np.frombuffer(b"".join(table), dtype=np.uint8)
                prefix.update(names=pl.upload(blob if blob.size else np.zeros(1, dtype=np.uint8)), name_off=pl.upload(off, pad_to=0),
                              names_bytes=int(blob.size))
            idx_ws = self.lib.acm_line_index_workspace_bytes(n)
            ctx_ws = self.lib.acm_line_context_lines_workspace_bytes(lcap, pl.nseg)
            starts, linfo, ws, cinfo = pl.alloc(lcap * 4), pl.alloc(32), pl.alloc(max(idx_ws, ctx_ws)), pl.alloc(16)
            self.line_index_async(pl.d, n, starts, lcap, linfo, delimiter=d, workspace=(ws.ptr, idx_ws))
            if line_number and pl.nseg:
                prefix["seg_num"] = pl.alloc(pl.nseg * 4)
                self.line_number_async(starts, lcap, linfo, pl.d_st, pl.nseg, prefix["seg_num"])
            if only_matching:
                sel_info = pl.alloc(16)
                start = self._select_stages(pl, init_state, sel_info, None)
                pl.max_records = k = pl.count()
                g = b""
                num = pl.alloc((k + 2) * 4)
                self.line_number_async(starts, lcap, linfo, start.ptr + 4, k, num.ptr + 4)
                cap = out_capacity if out_capacity is not None else min(n + k * (1 + widest), 2 ** 31 - 17)
                begin, end, ranges, incl = start, pl.off, k, True
                planes = (num, start, pl.off, None)
                prefix.update(num_plane=num)
            else:
                g = (b"--" + bytes([d]) if before + after > 0 else b"") if glue is None else bytes(glue)
                pl.scan(init_state, _lib.REPORT_STATE if per_line or pl.nseg else _lib.REPORT_HEAD)
                if pl.nseg:
                    pl.segment(_lib.REPORT_STATE if per_line else _lib.REPORT_HEAD)
                if per_line:
                    pl.segment(_lib.REPORT_HEAD, seg_start=starts, segments=lcap)
                rel, beg, nxt, kind = pl.line_context_lines(starts, lcap, linfo, cinfo, before, after, invert, (ws.ptr, ctx_ws))
                cap = out_capacity if out_capacity is not None else min(n + lcap * (1 + len(g) + widest), 2 ** 31 - 17)
                begin, end, ranges, incl = beg, nxt, lcap, False
                planes = (rel, beg, nxt, kind)
                prefix.update(kind_plane=kind, num_plane=rel)
            packed = pl.format(begin, end, ranges, info, cap, g, term, incl, **prefix)
            data, at_cells, res, seg_cells = self._packed_results(pl, info, cap, *packed)
            h = linfo.to_numpy(np.int32, 8, stream=self.stream)
            first = 1 + (int(np.uint32(h[4])) | int(np.uint32(h[5])) << 32)
            k = ranges if only_matching else int(planes[0].to_numpy(np.int32, 1, stream=self.stream)[0])
            cols = [x.to_numpy(np.int32, k + 1, stream=self.stream)[1:].astype(np.int64) if x is not None
                    else np.full(k, _lib.LINE_SELECTED, dtype=np.int64) for x in planes]
            cols[0] = cols[0] + first
            if only_matching:
                cols[2] = cols[2] + 1
            lines = np.stack(cols, axis=1) if k else np.zeros((0, 4), dtype=np.int64)
            return data, lines, at_cells, res, seg_cells

    def scan(self, text, init_state=0):
        """Scan host bytes: upload, scan, download."""
        with _Pipeline(self, "Matcher.scan", text) as p:
            p.scan(init_state, _lib.REPORT_HEAD)
            return self.fetch()

    def profile(self, enable):
        check(self.lib.acm_scan_profile_enable(self.dfa, int(enable)), "acm_scan_profile_enable")

    def profile_read(self):
        """(first kernel ms, second kernel ms, pipeline ms, launches) since the last read."""
        f, s2, p, n = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        check(self.lib.acm_scan_profile_read(self.dfa, C.byref(f), C.byref(s2), C.byref(p), C.byref(n)),
              "acm_scan_profile_read")
        return f.value, s2.value, p.value, n.value

    def close(self):
        for b in (self.ws, self.pat_plane, self.off_plane):
            if b is not None:
                b.free()
        self.ws = self.pat_plane = self.off_plane = None
        if self.dfa:
            self.lib.acm_dfa_release(self.dfa)
            self.dfa = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------- device ops

def exclusive_scan(values, stream=None):
    """int32 exclusive prefix sum on the device -> (scan, total)."""
    lib = _lib.load()
    a = np.ascontiguousarray(values, dtype=np.int32)
    d_in = DeviceArray.from_numpy(a, pad_to=0) if a.size else DeviceArray(16)
    d_out = DeviceArray(max(a.nbytes, 16))
    d_tot = DeviceArray(16)
    wsb = lib.acm_exclusive_scan_workspace_bytes(a.size)
    ws = DeviceArray(max(wsb, 16))
    check(lib.acm_exclusive_scan_i32(d_in.ptr, d_out.ptr, a.size, d_tot.ptr, ws.ptr, wsb, stream),
          "acm_exclusive_scan_i32")
    out = d_out.to_numpy(np.int32, a.size, stream=stream)
    tot = int(d_tot.to_numpy(np.int32, 1, stream=stream)[0])
    for d in (d_in, d_out, d_tot, ws):
        d.free()
    return out, tot


def compact_buckets(src, prefix, length, max_results, dst_cells, stream=None):
    lib = _lib.load()
    d_src = DeviceArray.from_numpy(np.ascontiguousarray(src, dtype=np.int32), pad_to=0)
    d_pre = DeviceArray.from_numpy(np.ascontiguousarray(prefix, dtype=np.int32), pad_to=0)
    d_dst = DeviceArray(dst_cells * 4)
    d_dst.fill(0)
    check(lib.acm_compact_buckets(d_dst.ptr, d_src.ptr, d_pre.ptr, length, max_results, stream),
          "acm_compact_buckets")
    out = d_dst.to_numpy(np.int32, dst_cells, stream=stream)
    for d in (d_src, d_pre, d_dst):
        d.free()
    return out


def bitonic_sort(keys, vals, batch, length, direction, stream=None):
    lib = _lib.load()
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    v = np.ascontiguousarray(vals, dtype=np.uint32)
    d_k = DeviceArray.from_numpy(k, pad_to=0)
    d_v = DeviceArray.from_numpy(v, pad_to=0)
    d_ko = DeviceArray(max(k.nbytes, 16))
    d_vo = DeviceArray(max(v.nbytes, 16))
    check(lib.acm_rt_memcpy_d2d(d_ko.ptr, d_k.ptr, k.nbytes, stream), "d2d")
    check(lib.acm_rt_memcpy_d2d(d_vo.ptr, d_v.ptr, v.nbytes, stream), "d2d")
    rc = lib.acm_bitonic_sort_u32(d_ko.ptr, d_vo.ptr, d_k.ptr, d_v.ptr, batch, length, direction,
                                  stream)
    ko = d_ko.to_numpy(np.uint32, k.size, stream=stream)
    vo = d_vo.to_numpy(np.uint32, v.size, stream=stream)
    for d in (d_k, d_v, d_ko, d_vo):
        d.free()
    return rc, ko, vo


def bucketize(pat_plane, off_plane, indices, sizes, max_results, stream=None):
    lib = _lib.load()
    ind = np.ascontiguousarray(indices, dtype=np.int32)
    siz = np.ascontiguousarray(sizes, dtype=np.int32)
    chunks = ind.size
    d_p = DeviceArray.from_numpy(np.ascontiguousarray(pat_plane, dtype=np.int32), pad_to=0)
    d_o = DeviceArray.from_numpy(np.ascontiguousarray(off_plane, dtype=np.int32), pad_to=0)
    d_i = DeviceArray.from_numpy(ind, pad_to=0)
    d_s = DeviceArray.from_numpy(siz, pad_to=0)
    cells = max_results * chunks + 1
    d_r = DeviceArray(cells * 4)
    d_r2 = DeviceArray(cells * 4)
    d_r.fill(0)
    d_r2.fill(0)
    check(lib.acm_bucketize(d_p.ptr, d_o.ptr, d_i.ptr, d_s.ptr, chunks, max_results, d_r.ptr,
                            d_r2.ptr, min(np.asarray(pat_plane).size, np.asarray(off_plane).size), stream),
          "acm_bucketize")
    r = d_r.to_numpy(np.int32, cells, stream=stream)
    r2 = d_r2.to_numpy(np.int32, cells, stream=stream)
    for d in (d_p, d_o, d_i, d_s, d_r, d_r2):
        d.free()
    return r, r2


def device_info(device=0):
    lib = _lib.load()
    name = C.create_string_buffer(256)
    cus, lds = C.c_int(), C.c_int()
    mem = C.c_size_t()
    check(lib.acm_rt_device_info(device, name, 256, C.byref(cus), C.byref(mem), C.byref(lds)),
          "acm_rt_device_info")
    return {"name": name.value.decode(), "cus": cus.value, "mem_bytes": mem.value,
            "lds_per_cu": lds.value}
