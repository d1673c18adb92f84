"""What the rule pass costs: acm_rule_matches_async per 32 MiB batch beside the sequence pass whose records it
takes, in one process.  The set is that of tools/sequence_bench.py -- the 2000 ClamAV signatures three times: as
1-part sequences, and cut into 2 and into 4 parts joined by {0-64} gaps -- with every sequence an operand: the
first third of the sequences in rules of one operand ("0"), the second in rules of two ("0&1"), the last in rules
of four ("(0&1)|(2|3)>1").  512 texts of 64 KiB per batch.  Two workloads: random bytes with 200 planted
signatures (few records: the pass costs its launches) and a dense text with 200000 planted.  Both passes order
max_records cells, so each is given its input's record count rounded up to 4096, as a caller who sizes its planes
would.  Device events around each run, medians over repeated runs, one JSON line.

python tools/rule_bench.py [--seconds 0.5] [--planted 200 200000] >> profiles/rule_bench.jsonl
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import fixtures
import synth
from gpu_pattern_matching_amd import Automaton, DeviceArray, Matcher, _lib
from sequence_bench import N, PIECE, signature_file

SHAPES = [(1, "0"), (2, "0&1"), (4, "(0&1)|(2|3)>1")]


def add_rules(a, sequences):
    """every sequence an operand: thirds of the sequences in rules of 1, 2 and 4 operands; returns the rules added"""
    third = sequences // 3
    q = 0
    for k, (nops, expr) in enumerate(SHAPES):
        end = sequences if k == 2 else (k + 1) * third
        while q + nops <= end:
            a.add_rule(list(range(q, q + nops)), expr, iid=a.num_rules)
            q += nops
        q = end
    return a.num_rules


def measure(name, sig_path, text, seconds):
    a = Automaton()
    sequences = a.load_signature_file(sig_path)
    a.compile()
    rules = add_rules(a, sequences)
    m = Matcher(a, 0, max_text=N)
    patterns = a.num_patterns
    levels = max(len(a.sequence(i)[0]) for i in range(sequences))
    slots = sum(len(a.rule(r)[0]) for r in range(rules))
    a.close()
    cap = m.plane_capacity
    acap = 4 * cap
    d = DeviceArray.from_numpy(text)
    starts = np.arange(0, text.size, PIECE, dtype=np.int32)
    d_st = DeviceArray.from_numpy(starts, pad_to=0)
    xp, xo, sq, so, info = tuple(DeviceArray(acap * 4) for _ in range(4)) + (DeviceArray(16),)
    nb_ex = m.lib.acm_expand_workspace_bytes(cap - 2)
    ws_ex = DeviceArray(nb_ex)
    m.scan_async(d, text.size, report=_lib.REPORT_STATE)
    _lib.check(m.lib.acm_expand_matches_async(m.dfa, m.pat_plane.ptr, m.off_plane.ptr, cap - 2, xp.ptr, xo.ptr, acap,
                                              ws_ex.ptr, nb_ex, m.stream), "acm_expand_matches_async")
    entries = int(xp.to_numpy(np.int32, 1)[0])
    assert entries <= acap - 2
    mr = (entries + 4096) & ~4095
    nb_seq = m.lib.acm_sequence_workspace_bytes(m.dfa, mr)
    ws_seq = DeviceArray(nb_seq)

    def sequence():
        m.sequence_async(xp, xo, mr, sq, so, acap, info, seg_start=d_st, segments=starts.size, text_end=text.size,
                         workspace=(ws_seq.ptr, nb_seq))

    sequence()
    matches = int(sq.to_numpy(np.int32, 1)[0])
    rr = (matches + 4096) & ~4095
    nb_rule = m.lib.acm_rule_workspace_bytes(m.dfa, rr)
    ws_rule = DeviceArray(nb_rule)
    ro, rt, rf = (DeviceArray((rr + 2) * 4) for _ in range(3))

    def rule():
        m.rule_async(sq, so, rr, ro, rt, rf, rr + 2, info, seg_start=d_st, segments=starts.size, workspace=(ws_rule.ptr, nb_rule))

    runs = {"sequence_pass": sequence, "rule_pass": rule}
    for f in runs.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    rule()
    held = int(ro.to_numpy(np.int32, 1)[0])
    rule_info = info.to_numpy(np.int32, 4).tolist()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = {k: [] for k in runs}
    spent = 0.0
    while spent < len(runs) * seconds or len(t["rule_pass"]) < 20:
        for key, f in runs.items():   # (sq, so hold the sequence pass's records: it rewrites the same cells)
            ev[0].record()
            f()
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1])
            t[key].append(ms)
            spent += ms / 1e3
    med = {k: round(float(np.median(v)) * 1e3, 1) for k, v in t.items()}
    # the launches as csrc/sequence.hip and csrc/rule.hip enqueue them: one 8-bit pass per byte of the slot count
    passes = lambda n: 1 + (n >> 8 != 0) + (n >> 16 != 0) + (n >> 24 != 0)
    out = {"workload": name, "patterns": patterns, "sequences": sequences, "levels": levels, "rules": rules,
           "rule_slots": slots, "texts": int(starts.size), "list_entries": entries, "sequence_max_records": mr,
           "sequence_matches": matches, "rule_max_records": rr, "operand_records": rule_info[0],
           "operand_text_pairs": rule_info[1], "rule_text_pairs_evaluated": rule_info[2], "rules_held": held,
           "sequence_launches": 4 + 3 * passes(patterns) + 2 * levels, "rule_launches": 5 + 3 * passes(slots),
           "rule_workspace_bytes": int(nb_rule), "sequence_workspace_bytes": int(nb_seq), "runs": len(t["rule_pass"])}
    out.update({k + "_us": v for k, v in med.items()})
    out["rule_over_sequence"] = round(med["rule_pass"] / med["sequence_pass"], 2)
    for b in (d, d_st, xp, xo, sq, so, info, ws_ex, ws_seq, ws_rule, ro, rt, rf):
        b.free()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--planted", type=int, nargs="*", default=[200, 200000], help="planted signatures of each workload")
    args = ap.parse_args()
    path, hx, max_len = fixtures.set_source("clamav2000")
    bodies = [l.strip() for l in open(path) if l.strip()]
    sig_path = signature_file(bodies)
    clam = [bytes.fromhex(b) for b in bodies]
    rows = []
    for planted in args.planted:
        name = "clamav2000 x (1, 2, 4 parts) in rules of 1, 2, 4 operands, %d planted" % planted
        rows.append(measure(name, sig_path, synth.clamav_corpus(N, 11, clam, planted), args.seconds))
    os.unlink(sig_path)
    print(json.dumps({"tool": "rule_bench", "batch_bytes": N, "workloads": rows}), flush=True)


if __name__ == "__main__":
    main()
