"""What wildcard patterns cost and what they save: the 2000 ClamAV signatures with every 8th byte turned into a
wildcard, loaded two ways -- extended (acm_automaton_load_signature_file_ex: only each part's longest exact run
enters the automaton, the wildcard pass verifies the rest) and, where syntax 0 can say it (?? only), as
sequences of fragments joined by gaps of one.  Per 32 MiB batch: patterns and states of each automaton, whether
the sparse pipeline takes it, the records its scan leaves, the wildcard pass beside the case pass over the same
planes, and the sequence pass each way.  Device events around each run, medians over repeated runs.

python tools/wildcard_bench.py [--seconds 0.3] >> profiles/wildcard_bench.jsonl
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import fixtures
import synth
from gpu_pattern_matching_amd import Automaton, DeviceArray, Matcher, _lib
from gpu_pattern_matching_amd._lib import check

N = 32 << 20


def bodies(pats, kind):
    """the hex body of every pattern with every 8th byte (never the first or the last) a wildcard: kind "any": ??;
    "mixed": a?, ?a and ?? in turn"""
    out = []
    for p in pats:
        h = ["%02x" % b for b in p]
        for k, i in enumerate(range(7, len(p) - 1, 8)):
            form = 2 if kind == "any" else k % 3
            h[i] = (h[i][0] + "?", "?" + h[i][1], "??")[form]
        out.append("".join(h))
    return out


def timed(runs, seconds, least=20):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = {k: [] for k in runs}
    spent = 0.0
    while spent < len(runs) * seconds or len(next(iter(t.values()))) < least:
        for key, f in runs.items():
            ev[0].record()
            f()
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1])
            t[key].append(ms)
            spent += ms / 1e3
    return {k: round(float(np.median(v)) * 1e3, 1) for k, v in t.items()}, len(next(iter(t.values())))


def measure(name, sig_file, extended, text, seconds):
    a = Automaton()
    assert a.load_signature_file(sig_file, extended=extended) == 2000
    a.compile()
    out = {"workload": name, "syntax": "extended" if extended else "0", "patterns": a.num_patterns, "states": a.num_states,
           "contexts": a.has_wildcards, "reach": list(a.wildcard_reach),
           "shortest_pattern": min(len(a.pattern(i)[0]) for i in range(a.num_patterns))}
    m = Matcher(a, 0, max_text=N)
    a.close()
    out["sparse_eligible"] = bool(m.sparse_eligible())
    cap = m.plane_capacity
    d = DeviceArray.from_numpy(text)

    def scan_state():
        m.scan_async(d, text.size, report=_lib.REPORT_STATE)
    for _ in range(3):
        scan_state()
    out["pipeline"] = m.path_taken(text.size)
    out["records"] = int(m.pat_plane.to_numpy(np.int32, 1)[0])
    ex_bytes = m.lib.acm_expand_workspace_bytes(cap - 2)
    ex, two_p, two_o = DeviceArray(ex_bytes), DeviceArray(16), DeviceArray(16)

    def expand(pat, off, room):
        check(m.lib.acm_expand_matches_async(m.dfa, m.pat_plane.ptr, m.off_plane.ptr, cap - 2, pat.ptr, off.ptr, room, ex.ptr,
                                             ex_bytes, m.stream), "acm_expand_matches_async")
    expand(two_p, two_o, 2)                       # (the count cell holds the full count whatever the room)
    out["list_entries"] = entries = int(two_p.to_numpy(np.int32, 1)[0])
    room = entries + 2
    e_pat, e_off = DeviceArray(room * 4), DeviceArray(room * 4)       # the expansion: what the sequence pass takes in syntax 0
    w_pat, w_off = DeviceArray(room * 4), DeviceArray(room * 4)       # behind the wildcard or case pass
    q_pat, q_off = DeviceArray(room * 4), DeviceArray(room * 4)       # the sequence pass's
    info = DeviceArray(16)
    expand(e_pat, e_off, room)
    wl_bytes = m.lib.acm_wildcard_workspace_bytes(max(cap - 2, entries))
    cs_bytes = m.lib.acm_case_workspace_bytes(cap - 2)
    wl, cs = DeviceArray(wl_bytes), DeviceArray(cs_bytes)

    def wild(report):
        sp, so, n = (m.pat_plane, m.off_plane, cap - 2) if report == _lib.REPORT_STATE else (e_pat, e_off, entries)
        m.wildcard_async(sp, so, n, d, 0, text.size, w_pat, w_off, room, info, report=report, open_end=text.size,
                         all_patterns=True, workspace=(wl.ptr, wl_bytes))

    def case():
        m.case_async(m.pat_plane, m.off_plane, cap - 2, d, 0, text.size, w_pat, w_off, room, all_patterns=True,
                     workspace=(cs.ptr, cs_bytes))
    wild(_lib.REPORT_HEAD)
    out["kept_entries"] = kept = int(w_pat.to_numpy(np.int32, 1)[0])
    out["undecided"] = int(info.to_numpy(np.int32, 4)[0])
    sq_bytes = m.lib.acm_sequence_workspace_bytes(m.dfa, entries)
    sq = DeviceArray(sq_bytes)
    out["sequence_workspace_MiB"] = round(sq_bytes / 2 ** 20, 1)

    def sequence():
        sp, so, n = (w_pat, w_off, kept) if extended else (e_pat, e_off, entries)
        m.sequence_async(sp, so, n, q_pat, q_off, room, info, text_end=text.size, workspace=(sq.ptr, sq_bytes))
    sequence()
    out["matches"] = int(q_pat.to_numpy(np.int32, 1)[0])
    runs = {"scan_state": scan_state, "expand": lambda: expand(e_pat, e_off, room), "case_pass_all": case,
            "wildcard_pass_state_all": lambda: wild(_lib.REPORT_STATE), "wildcard_pass_head_all": lambda: wild(_lib.REPORT_HEAD)}
    for f in runs.values():
        f()
    wild(_lib.REPORT_HEAD)                        # (the sequence pass reads these planes)
    runs = dict(runs, wildcard_pass_head_all_again=lambda: wild(_lib.REPORT_HEAD), sequence_pass=sequence)
    torch.cuda.synchronize()
    med, n = timed(runs, seconds)
    med.pop("wildcard_pass_head_all_again")
    out["runs"] = n
    out.update({k + "_us": v for k, v in med.items()})
    out["wildcard_over_case"] = round(med["wildcard_pass_state_all"] / med["case_pass_all"], 2)
    for b in (d, ex, two_p, two_o, e_pat, e_off, w_pat, w_off, q_pat, q_off, info, wl, cs, sq):
        b.free()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3)
    args = ap.parse_args()
    path, _, _ = fixtures.set_source("clamav2000")
    pats = synth.load_hex_patterns(path, 2000)
    text = synth.clamav_corpus(N, 11, pats, 20000)
    with tempfile.TemporaryDirectory() as tmp:
        for kind, ways in (("mixed", (True,)), ("any", (True, False))):
            f = os.path.join(tmp, kind + ".sig")
            with open(f, "w") as fh:
                fh.write("\n".join(bodies(pats, kind)) + "\n")
            for extended in ways:
                name = "clamav2000, every 8th byte %s, 20000 planted" % ("a?, ?a or ??" if kind == "mixed" else "??")
                print(json.dumps(measure(name, f, extended, text, args.seconds)), flush=True)


if __name__ == "__main__":
    main()
