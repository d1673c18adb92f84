"""tests/signature_oracle.py against three other statements of the same thing, on small random cases (an alphabet
of five bytes, texts of at most 120 bytes, empty texts, texts that are exactly one match).  They are not all
independent of it: the oracle parses bodies with wildcard_model.parse_body_ex and evaluates rules with
rule_model.parse / evaluate, as 1 does; only 2 shares no body parser, and only the records of 3 no rule evaluator:
  1. wildcard_model.span_sequences (a Python loop per offset) combined with rule_model.RuleModel
  2. Python's re, for the signatures without a window and without nocase: the regex is built from the body text
     alone, and "a match ends at e" is fullmatch(text, 0, e + 1) of .*? + body
  3. the hand-derived expectations that test_gpu_rules.test_scan_rules and
     test_gpu_wildcards.test_scan_sequences_extended assert of the device
Bodies with groups, (aabb|ccdd) and !(aabb|ccdd), go the same three ways: the oracle shares only the grammar
(group_model.parse_body_groups) with 1, whose Patterns ask group_model.group_holds offset by offset; 2 is
group_model.body_regex, a translation of the body text; 3 are the texts of test_gpu_groups.test_span_rules_by_hand
and the body of test_the_issue_body.
No GPU: only the host library (the parsers of rule_model and wildcard_model are Python)."""
import hashlib
import re

import numpy as np
import pytest

import group_model as gm
import rule_model as rm
import signature_oracle as so
import wildcard_model as wm

CASES = 240


def random_case(seed, group_share=0.0):
    """(lines, nocase per signature, windows, texts); group_share > 0: a fifth value, the groups per signature and
    part, and some texts are near misses of a signature's groups"""
    rng = np.random.default_rng(seed)
    groups = []
    alphabet = so.LETTERS[:int(rng.integers(3, 6))]
    lines, nocase, windows, sigs = [], [], {}, []
    for _ in range(int(rng.integers(1, 4))):
        nops = int(rng.integers(1, 4))
        bodies = []
        for _ in range(nops):
            if group_share:
                groups.append([])
                body, sets, gaps = so.random_body(rng, parts=(1, 3), alphabet=alphabet, anchor=(1, 3), group_share=group_share,
                                                  groups_out=groups[-1])
            else:
                body, sets, gaps = so.random_body(rng, parts=(1, 3), alphabet=alphabet, anchor=(1, 3))
            q = len(sigs)
            nocase.append(bool(rng.random() < 0.3))
            sigs.append((sets, gaps))
            bodies.append(body)
            if rng.random() < 0.25:
                lo = int(rng.integers(0, 4))
                windows[q, 0] = [(0, 0, False), (lo, lo + int(rng.integers(0, 30)), False), (lo, None, False),
                                 (0, int(rng.integers(1, 40)), True), (len(sets[0]), len(sets[0]), True)][int(rng.integers(5))]
        lines.append(so.random_expr(rng, nops) + ";" + ";".join(bodies))
    texts = [b""]
    pool = np.frombuffer(alphabet, dtype=np.uint8)
    for _ in range(int(rng.integers(3, 8))):
        kind = rng.random()
        t = bytes(rng.choice(pool, size=int(rng.integers(0, 60))))
        if kind < 0.7:                                  # one or two planted matches; kind < 0.15: nothing around them
            for _ in range(int(rng.integers(1, 3))):
                q = int(rng.integers(len(sigs)))
                if group_share:
                    inst = so.materialise(rng, sigs[q][0], sigs[q][1], alphabet, nocase[q], groups[q],
                                          near_miss=any(groups[q]) and rng.random() < 0.4)
                else:
                    inst = so.materialise(rng, sigs[q][0], sigs[q][1], alphabet, nocase[q])
                t = inst if kind < 0.15 else t + inst + bytes(rng.choice(pool, size=int(rng.integers(0, 8))))
        texts.append(t[:120])
    texts.insert(int(rng.integers(len(texts))), b"")
    if group_share:
        return lines, nocase, windows, texts, groups
    return lines, nocase, windows, texts


def by_model(lines, nocase, windows, texts, groups=False):
    """(sorted (end, signature), sorted (rule, text, offset)) by span_sequences and RuleModel"""
    pats, seqs, rules, win = [], [], [], {}
    for line in lines:
        expr, bodies = so.split_line(line)
        ops = []
        for b in bodies:
            q = len(seqs)
            parts, gaps, grps = gm.parse_body_groups(b) if groups else wm.parse_body_ex(b) + (None,)
            for j in range(len(parts)):
                if (q, j) in windows:
                    win[len(pats) + j] = windows[q, j]
            seqs.append((list(range(len(pats), len(pats) + len(parts))), gaps))
            pats += [gm.Pattern(p, grps[j], nocase[q]) if groups else wm.Pattern(p, nocase[q]) for j, p in enumerate(parts)]
            ops.append(q)
        rules.append((ops, expr))
    found = sorted(wm.span_sequences(pats, seqs, texts, win))
    recs = sorted((e - pats[seqs[q][0][-1]].post, q) for e, q in found)      # the records of the sequence pass
    lens = [len(t) for t in texts]
    starts = (np.cumsum(lens) - lens).tolist()
    er, et, eo, _ = rm.RuleModel(len(seqs), rules).run([q for _, q in recs], [o for o, _ in recs], starts)
    return found, sorted(zip(er.tolist(), et.tolist(), eo.tolist()))


def by_oracle(lines, nocase, windows, texts, db_groups=False, **kw):
    db = so.Database(lines, nocase, windows, db_groups)
    m = so.sequences(db, texts, **kw)
    return sorted(zip(m[0].tolist(), m[2].tolist())), so.rules(db, texts, m)


_POSITION = re.compile(r"([0-9a-fA-F]{2})|(\?\?)|([0-9a-fA-F])\?|\?([0-9a-fA-F])|(!?)\(([0-9a-fA-F|]+)\)|(\*)|\{(\d*)(-?)(\d*)\}")


def regex_of(body):
    """the body as a regular expression over bytes, from its text alone"""
    out, at = b"", 0
    while at < len(body):
        m = _POSITION.match(body, at)
        g = m.groups()
        if g[0]:
            out += b"\\x" + g[0].encode()
        elif g[1]:
            out += b"."
        elif g[2]:
            out += b"[\\x%s0-\\x%sf]" % (g[2].encode(), g[2].encode())
        elif g[3]:
            out += b"[" + b"".join(b"\\x%x%s" % (h, g[3].encode()) for h in range(16)) + b"]"
        elif g[5]:
            out += (b"[^" if g[4] else b"[") + b"".join(b"\\x" + h.encode() for h in g[5].split("|")) + b"]"
        elif g[6]:
            out += b".*"
        else:
            lo, dash, hi = g[7], g[8], g[9]
            out += b".{%s,%s}" % ((lo or "0").encode(), (hi if dash else lo).encode())
        at = m.end()
    return re.compile(b".*?" + out, re.DOTALL)


def by_regex(lines, texts, keep):
    out, q = set(), 0
    for line in lines:
        for body in so.split_line(line)[1]:
            if keep(q):
                rx, base = regex_of(body), 0
                for t in texts:
                    out |= {(base + e, q) for e in range(len(t)) if rx.fullmatch(t, 0, e + 1)}
                    base += len(t)
            q += 1
    return out


def test_against_the_models_and_re():
    seen = dict(matches=0, rules=0, first=0, last=0, windows=0, nocase=0, cases_with_rules=0)
    for seed in range(CASES):
        lines, nocase, windows, texts = random_case(seed)
        found, fired = by_oracle(lines, nocase, windows, texts)
        xfound, xfired = by_model(lines, nocase, windows, texts)
        assert found == xfound, (seed, lines, sorted(set(found) ^ set(xfound))[:5])
        assert fired == xfired, (seed, lines, sorted(set(fired) ^ set(xfired))[:5])
        plain = lambda q: not nocase[q] and (q, 0) not in windows
        got = {x for x in found if plain(x[1])}
        assert got == by_regex(lines, texts, plain), (seed, lines)
        seen["matches"] += len(found)
        seen["rules"] += len(fired)
        seen["cases_with_rules"] += bool(fired)
        lens = [len(t) for t in texts]
        ends = set((np.cumsum(lens) - 1).tolist())
        seen["last"] += sum(e in ends for e, _ in found)
        seen["first"] += sum(bool(t) and any(e == b + len(t) - 1 for e, _ in found)
                             for t, b in zip(texts, np.cumsum(lens) - lens) if len(t) <= 20)
        seen["windows"] += found != by_oracle(lines, nocase, {}, texts)[0]
        seen["nocase"] += found != by_oracle(lines, None, windows, texts)[0]
    # the cases are worth their time: matches, rules, matches that end a text and that are a whole text, and cases
    # in which the windows and the case flags decide
    assert seen["matches"] > 10 * CASES and seen["cases_with_rules"] > CASES // 2 and seen["last"] > CASES // 2
    assert seen["first"] > 20 and seen["windows"] > 20 and seen["nocase"] > 20, seen


def digest(g):
    h = hashlib.sha256()
    for part in ("\n".join(g.lines).encode(), b"".join(len(t).to_bytes(4, "little") + t for t in g.texts),
                 repr(sorted(g.windows.items())).encode(), repr((g.nocase, g.rule_nocase)).encode()):
        h.update(hashlib.sha256(part).digest())
    return h.hexdigest()


def test_the_generator_without_groups_is_what_it_was():
    """make() with the share of groups at its default of 0 draws the random numbers it drew before it knew groups:
    the digest is that of the lines, texts, windows and case flags the module gave before (computed with it), the
    database of tests/test_gpu_signature_chain.py, whose seeded counts rest on it"""
    g = so.make(1, rules=70)
    assert digest(g) == "6287609dbe7ac9663aca6d420695450bb48b85f9260fe905e3ff0baaee35a496"
    assert not any(p.groups for parts, _ in g.db.sigs for p in parts)
    assert digest(so.make(1, rules=8, texts=300, total=20 * 1024, empties=100, long_text=2000, group_share=0.45)) != digest(
        so.make(1, rules=8, texts=300, total=20 * 1024, empties=100, long_text=2000))


GROUP_CASES = 200


def test_groups_against_the_models_and_re():
    """bodies of which half the parts carry a group: the oracle against span_sequences over group_model.Patterns with
    RuleModel, against re through group_model.body_regex, and against itself with the groups off"""
    seen = dict(matches=0, rules=0, dropped=0, rules_differ=0, negated=0, positive=0, exact=0, wide=0, many=0, adjacent=0,
                first=0, last=0, nocase=0, window_on_group=0)
    for seed in range(GROUP_CASES):
        lines, nocase, windows, texts, groups = random_case(1000 + seed, group_share=0.5)
        found, fired = by_oracle(lines, nocase, windows, texts, db_groups=True)
        xfound, xfired = by_model(lines, nocase, windows, texts, groups=True)
        assert found == xfound, (seed, lines, sorted(set(found) ^ set(xfound))[:5])
        assert fired == xfired, (seed, lines, sorted(set(fired) ^ set(xfired))[:5])
        plain = lambda q: not nocase[q] and (q, 0) not in windows
        base, want, bodies = 0, set(), [b for line in lines for b in so.split_line(line)[1]]
        for t in texts:
            for q, body in enumerate(bodies):
                if plain(q):
                    want |= {(base + e, q) for e in gm.regex_ends(body, t)}
            base += len(t)
        assert {x for x in found if plain(x[1])} == want, (seed, lines)
        # the groups off: what the same database matches with ?? in their place, a superset
        loose, lfired = by_oracle(lines, nocase, windows, texts, db_groups=True, groups=False)
        assert set(found) <= set(loose)
        db = so.Database(lines, nocase, windows, True)
        for q, (parts, _) in enumerate(db.sigs):           # the generator's record of the groups is the parser's
            assert [p.groups for p in parts] == [[(at, list(ss), neg) for at, ss, neg in gs] for gs in groups[q]], (seed, q)
            for j, p in enumerate(parts):
                for at, strings, neg in p.groups:
                    seen["negated" if neg else "positive"] += 1
                    seen["wide"] += len(strings[0]) >= 31
                    seen["many"] += len(strings) >= 255
                    seen["first"] += at == 0
                    seen["last"] += at + len(strings[0]) == p.n
                    seen["nocase"] += nocase[q]
                    seen["window_on_group"] += at == 0 and (q, j) in windows
                seen["adjacent"] += any(a[0] + len(a[1][0]) == b[0] for a, b in zip(p.groups, p.groups[1:]))
        seen["exact"] += sum(len(re.findall(r"(?<!!)\((?:[0-9a-f]{2}){2,}\)", b)) for b in bodies)      # one string: exact bytes
        seen["matches"] += len(found)
        seen["rules"] += len(fired)
        seen["dropped"] += len(loose) - len(found)
        seen["rules_differ"] += fired != lfired
    assert seen["matches"] > 5 * GROUP_CASES and seen["dropped"] > GROUP_CASES and seen["rules_differ"] > 20, seen
    assert min(seen["negated"], seen["positive"], seen["first"], seen["last"], seen["nocase"]) > 40, seen
    assert min(seen["wide"], seen["many"], seen["adjacent"], seen["window_on_group"], seen["exact"]) >= 5, seen
    print(seen)


def hits(bodies, texts, **kw):
    """sorted (offset at which the last part's ANCHOR ends, signature) of bodies with groups"""
    db = so.Database(["%s;%s" % ("|".join("%d" % j for j in range(len(bodies))), ";".join(bodies))], groups=True)
    _, aends, sigs = so.sequences(db, texts, **kw)
    return sorted(zip(aends.tolist(), sigs.tolist()))


def test_the_hand_derived_expectations_of_the_group_tests():
    # test_gpu_groups.test_span_rules_by_hand: its three patterns as bodies, its texts and what it derives by hand
    edge = ["(6378|7863)6262", "6262(6362|6262)", "!(637863)6262"]
    text = b"cxbbcbbbb"                                                   # bb ends at 3, 6, 7, 8
    assert hits(edge, [text]) == [(3, 0), (3, 1), (6, 1), (6, 2), (7, 2), (8, 2)]
    assert (7, 1) not in hits(edge, [text])                              # its group would need the byte at 9
    recs = hits(edge, [text[:1], text[1:]])                              # a text that starts at 1
    assert (3, 0) not in recs and (3, 1) in recs
    recs = hits(edge, [text[:5], text[5:]])                              # texts [0, 5) and [5, 9)
    assert (3, 1) not in recs and (3, 0) in recs and (6, 2) not in recs and (8, 2) not in recs
    for t, want in ((b"cxcbb", [(4, 0)]), (b"qxcbb", [(4, 0), (4, 2)]), (b"\x00xcbb", [(4, 0), (4, 2)]), (b"cqcbb", [(4, 2)]),
                    (b"c\x00cbb", [(4, 2)]), (b"zzcxcbb", [(6, 0)])):
        assert hits(edge, [t]) == want, t
    # with the groups off every bb with enough bytes around it is a hit
    assert hits(edge, [text], groups=False) == [(3, 0), (3, 1), (6, 0), (6, 1), (6, 2), (7, 0), (7, 2), (8, 0), (8, 2)]
    # the body of test_gpu_groups.test_the_issue_body, on its texts against re and on two texts by hand
    body = "aa(bbcc|ddee)ff*!(0102|0304)11"
    rng = np.random.default_rng(2)
    menu = [bytes.fromhex(x) for x in ("aabbccff", "aaddeeff", "aabbeeff", "010211", "030411", "010411", "ff11", "00", "aa")]
    texts = [b"".join(menu[int(k)] for k in rng.integers(0, len(menu), size=int(rng.integers(0, 14)))) for _ in range(30)]
    want, base = [], 0
    for t in texts:
        want += [(base + o, 0) for o in gm.regex_ends(body, t)]
        base += len(t)
    assert len(want) > 20 and hits([body], texts) == sorted(want)
    assert hits([body], [bytes.fromhex("aabbccff00010311")]) == [(7, 0)]
    assert hits([body], [bytes.fromhex("aaddeeff010211aabbccff03041111")]) == [(14, 0)]
    assert hits([body], [bytes.fromhex("aabbccff"), bytes.fromhex("010311")]) == []
    counts, loose = {}, {}
    so.sequences(so.Database(["0;" + body], groups=True), texts, counts=counts)
    so.sequences(so.Database(["0;" + body], groups=True), texts, counts=loose, groups=False)
    assert loose["anchors"] == counts["anchors"] and loose["parts"] > counts["parts"] > 0
    with pytest.raises(gm.BodyError):
        so.Database(["0;" + body])                       # the grammar without groups refuses it
    with pytest.raises(gm.BodyError):
        so.Database(["0;aa(bbcc|dd)"], groups=True)


def test_the_hand_derived_expectations_of_the_device_tests():
    # test_gpu_rules.test_scan_rules: its automaton as logical lines, its texts, the records it expects
    lines = ["0&1;6e6565646c65;6162{1-3}6364", "(0|1)>1;(31|32)7879;68656c6c6f", "0=2;7a7a"]
    nocase = [False, False, False, True, False]
    texts = [b"a needle, then ab.cd and abcd", b"needle ab....cd", b"ab..cd", b"needleneedle ab...cd abXcd",
             b"", b"1xy hello", b"1xy 2xy", b"HeLLo hello 3xy", b"hello", b"zz", b"zzz", b"z zz z zz", b"zz" * 150,
             b"1xyHELLOneedleab.cdzz.zz needle" + b"." * 300 + b"hello", b"", b"needle", b"ab.cd"]
    db = so.Database(lines, nocase)
    fired = so.rules(db, texts, so.sequences(db, texts))
    by_trigger = [(r, t) for r, t, o in sorted(fired, key=lambda x: (x[2], x[0]))]
    assert by_trigger == [(0, 0), (0, 3), (1, 5), (1, 6), (1, 7), (2, 10), (2, 11), (1, 13), (0, 13), (2, 13)]
    whole = [b"".join(texts)]
    assert [(r, t) for r, t, _ in so.rules(db, whole, so.sequences(db, whole))] == [(0, 0), (1, 0)]   # 150 + x "zz": "0=2" fails
    # test_gpu_wildcards.test_scan_sequences_extended: every signature matches somewhere, under every kind, and
    # the case flags and the windows matter; its windows are keyed by pattern: 3 is signature 1's only part, 5
    # the second part of signature 2
    sigs = ["61?2*(61|62)63{1-3}6?61", "6162??63", "!(61)6263{2}61!(62|63)", "63??????61{-4}62(61|63)", "6261"]
    lines = ["%s;%s" % ("|".join("%d" % j for j in range(len(sigs))), ";".join(sigs))]
    for kind in ("plain", "mixed", "window"):
        rng = np.random.default_rng(11)
        letters = (0x61, 0x62, 0x63, 0x41, 0x43) if kind == "mixed" else (0x61, 0x62, 0x63)
        texts = [bytes(rng.choice(np.array(letters, dtype=np.uint8), size=int(rng.integers(0, 90)))) for _ in range(20)] + [b""]
        nc = [q in (0, 3) and kind == "mixed" for q in range(5)]
        win = {(1, 0): (2, 30, False), (2, 1): (0, 12, True)} if kind == "window" else {}
        found, _ = by_oracle(lines, nc, win, texts)
        assert {q for _, q in found} == set(range(5)), kind
        assert found == by_model(lines, nc, win, texts)[0]
        if kind != "plain":
            assert found != by_oracle(lines, [False] * 5, {}, texts)[0]


def test_counts_and_switches():
    """the stage counts only shrink along the chain, and contexts=False is the anchors alone"""
    lines, nocase, windows, texts = random_case(5)
    db = so.Database(lines, nocase, windows)
    counts = {}
    so.sequences(db, texts, counts=counts)
    assert counts["anchors"] >= counts["parts"] >= counts["windowed"] and counts["matches"] >= 0
    loose = {}
    so.sequences(db, texts, contexts=False, counts=loose)
    assert loose["parts"] >= counts["parts"] and loose["anchors"] == counts["anchors"]
    # the parts behind one that never occurs are counted too: the device passes see their records
    dead = {}
    assert so.sequences(so.Database(["0;6161{2}6262(61|78)"]), [b"bbxbb", b"bba"], counts=dead)[0].size == 0
    assert dead == dict(anchors=3, parts=2, windowed=2, matches=0)
    with pytest.raises(rm.RuleError):
        so.Database(["0=0;6162"])
