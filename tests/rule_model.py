"""Rules in Python (test infrastructure only, not a conftest): the expression grammar of acm_automaton_add_rule,
its values, the trigger rule and the plane layout of acm_rule_matches_async, written from include/acmatch.h.
It shares no code with the C side.

  expr := term ( '&' term )*  |  term ( '|' term )*
  term := ( NUMBER | '(' expr ')' ) [ ( '=' | '>' | '<' ) NUMBER ]

Every node has a count and a truth: an operand its occurrences in the text and count > 0; '&' and '|' the sum of
their children's counts and all / any of their truths; a comparison keeps the count and tests it.

  parse        the expression as a tree; RuleError carries the error kind ("parse", "limit" or "arg") and,
               for a parse or limit error, the column (from 1)
  evaluate     (count, truth) of a tree over the operands' counts
  RuleModel    the pass over (sequence, offset) cells: per text the counts, per rule the trigger and the record
  planes       the three planes of cap cells a call must leave
"""
import numpy as np

MAX_OPERANDS = 64
MAX_NESTING = 8
INT32_MAX = 0x7FFFFFFF


class RuleError(ValueError):
    def __init__(self, kind, column=None, why=""):
        ValueError.__init__(self, "%s error%s: %s" % (kind, "" if column is None else " at column %d" % column, why))
        self.kind = kind
        self.column = column


class _Parser:
    def __init__(self, text, nops):
        self.t = text
        self.nops = nops
        self.pos = 0

    def peek(self):
        while self.pos < len(self.t) and self.t[self.pos] in " \t":
            self.pos += 1
        return self.t[self.pos] if self.pos < len(self.t) else ""

    def number(self):
        """the digits at pos (the caller has seen one)"""
        at = self.pos
        while self.pos < len(self.t) and self.t[self.pos] in "0123456789":
            self.pos += 1
        v = int(self.t[at:self.pos])
        if v > INT32_MAX:
            raise RuleError("parse", at + 1, "number too large")
        return v

    def term(self, depth):
        c = self.peek()
        at = self.pos
        if c and c in "0123456789":
            op = self.number()
            if op >= self.nops:
                raise RuleError("parse", at + 1, "operand out of range")
            node = ("op", op)
        elif c == "(":
            if depth + 1 > MAX_NESTING:
                raise RuleError("limit", at + 1, "nested too deep")
            self.pos += 1
            node = self.expr(depth + 1)
            if self.peek() != ")":
                raise RuleError("parse", self.pos + 1, "expected )")
            self.pos += 1
        else:
            raise RuleError("parse", at + 1, "expected an operand or (")
        c = self.peek()
        if c and c in "=><":
            self.pos += 1
            d = self.peek()
            if not d or d not in "0123456789":
                raise RuleError("parse", self.pos + 1, "expected a number")
            n = self.number()
            if self.pos < len(self.t) and self.t[self.pos] == ",":
                raise RuleError("parse", self.pos + 1, "=n,m is not provided")
            node = ("cmp", c, n, node)
        return node

    def expr(self, depth):
        kids = [self.term(depth)]
        op = self.peek()
        if op not in ("&", "|"):
            return kids[0]
        while self.peek() == op:
            self.pos += 1
            kids.append(self.term(depth))
        if self.peek() in ("&", "|"):
            raise RuleError("parse", self.pos + 1, "& and | mixed at one level")
        return (op, kids)


def evaluate(node, counts):
    """(count, truth) of the tree over counts[operand]"""
    if node[0] == "op":
        c = int(counts[node[1]])
        return c, c > 0
    if node[0] == "cmp":
        c, _ = evaluate(node[3], counts)
        return c, {"=": c == node[2], ">": c > node[2], "<": c < node[2]}[node[1]]
    vals = [evaluate(k, counts) for k in node[1]]
    truths = [t for _, t in vals]
    return sum(c for c, _ in vals), all(truths) if node[0] == "&" else any(truths)


def parse(text, nops):
    """the tree of an expression over nops operands; RuleError as acm_automaton_add_rule refuses it"""
    if nops < 1:
        raise RuleError("arg", None, "no operands")
    if nops > MAX_OPERANDS:
        raise RuleError("limit", None, "too many operands")
    p = _Parser(text, nops)
    tree = p.expr(0)
    if p.peek() != "":
        raise RuleError("parse", p.pos + 1, "unexpected character")
    if evaluate(tree, [0] * nops)[1]:
        raise RuleError("arg", None, "true for a text without a hit")
    return tree


class RuleModel:
    """num_sequences: the sequences of the set; rules: a list of (operand sequence indices, expression)"""

    def __init__(self, num_sequences, rules):
        self.nseq = num_sequences
        self.rules = [(list(ops), parse(e, len(ops))) for ops, e in rules]
        self.slot_of = {}
        for r, (ops, _) in enumerate(self.rules):
            for j, q in enumerate(ops):
                assert q not in self.slot_of and 0 <= q < num_sequences
                self.slot_of[q] = (r, j)

    def run(self, cells, offs, starts=()):
        """(rules int32, texts int32, offsets int64, info[4]) the pass writes for the cells, in offset order"""
        cells = [int(c) for c in cells]
        offs = np.asarray(offs, dtype=np.int64)
        text = np.searchsorted(np.asarray(starts, dtype=np.int64), offs, side="right") - 1 if len(starts) \
            else np.full(offs.size, -1, dtype=np.int64)
        count, first = {}, {}                       # (rule, operand, text) -> occurrences, first input index
        operands = 0
        for i, q in enumerate(cells):
            if q not in self.slot_of:
                continue
            operands += 1
            key = self.slot_of[q] + (int(text[i]),)
            count[key] = count.get(key, 0) + 1
            first.setdefault(key, i)
        pairs = {}                                  # (rule, text) -> the lowest operand that occurs
        for r, j, t in count:
            pairs[r, t] = min(pairs.get((r, t), j), j)
        out = []
        for (r, t), j in pairs.items():
            ops, tree = self.rules[r]
            if evaluate(tree, [count.get((r, k, t), 0) for k in range(len(ops))])[1]:
                out.append((first[r, j, t], r, t))
        out.sort()
        idx = [i for i, _, _ in out]
        return (np.array([r for _, r, _ in out], dtype=np.int32), np.array([t for _, _, t in out], dtype=np.int32),
                offs[idx], [operands, len(count), len(pairs), 0])


def planes(rules, texts, offs, cap, poison, trailer):
    """the three planes of cap cells a call must leave: [0] = count, the records that fit, the trailer at
    min(count + 1, cap - 1), the poison cell value everywhere else"""
    m = len(rules)
    stored = min(m, cap - 2)
    out = []
    for e in (rules, texts, offs):
        p = np.full(cap, poison, dtype=np.int32)
        p[0] = m
        p[1:1 + stored] = np.asarray(e[:stored], dtype=np.int64).astype(np.int32)
        p[min(m + 1, cap - 1)] = trailer
        out.append(p)
    return out
