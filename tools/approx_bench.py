"""What approximate matching costs: the 2000 ClamAV signatures with a budget of k = 0, 1 and 2 mismatches each
(acm_automaton_add_approx; as acm_grep -k does, a pattern shorter than 3 * (k + 1) bytes stays exact, so that every
piece has three bytes and the sparse pipeline stays eligible).  Per 32 MiB batch: patterns and states of the
automaton, the pipeline its scan takes, the records the scan leaves and their list entries, the entries the
approx pass keeps, and the time of the scan, of the approx pass over states and over pattern cells, and of the
wildcard pass over the same planes (no contexts: it keeps every entry and reads no text -- the cost of the
record-pass skeleton alone).  Device events around each run, medians over repeated runs.

python tools/approx_bench.py [--seconds 0.3] >> profiles/approx_bench.jsonl
"""
import argparse
import json
import os
import sys

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
    med = {k: round(float(np.median(v)) * 1e3, 1) for k, v in t.items()}
    spread = {k: [round(float(min(v)) * 1e3, 1), round(float(max(v)) * 1e3, 1)] for k, v in t.items()}
    return med, spread, len(next(iter(t.values())))


def measure(pats, k, text, seconds):
    a = Automaton()
    tolerant = 0
    for i, p in enumerate(pats):
        ok = k > 0 and len(p) >= 3 * (k + 1)
        tolerant += ok
        a.add_approx(p, k if ok else 0, i)
    a.compile()
    out = {"workload": "clamav2000, 20000 planted", "k": k, "approximate": tolerant, "patterns": a.num_patterns,
           "states": a.num_states, "reach": list(a.approx_reach),
           "shortest_pattern": min(len(a.pattern(i)[0]) for i in range(a.num_patterns))}
    m = Matcher(a, 0, max_text=N)
    a.close()
    out["sparse_eligible"] = bool(m.sparse_eligible())
    out["device_MiB"] = round(m.device_bytes / 2 ** 20, 1)
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
    e_pat, e_off = DeviceArray(room * 4), DeviceArray(room * 4)                              # the expansion
    w_pat, w_off, w_dist = DeviceArray(room * 4), DeviceArray(room * 4), DeviceArray(room * 4)   # behind the pass
    info = DeviceArray(16)
    expand(e_pat, e_off, room)
    ax_bytes = m.lib.acm_approx_workspace_bytes(max(cap - 2, entries))
    wl_bytes = m.lib.acm_wildcard_workspace_bytes(max(cap - 2, entries))
    ax, wl = DeviceArray(ax_bytes), DeviceArray(wl_bytes)

    def planes(report):
        return (m.pat_plane, m.off_plane, cap - 2) if report == _lib.REPORT_STATE else (e_pat, e_off, entries)

    def approx(report, dist=True):
        sp, so, n = planes(report)
        m.approx_async(sp, so, n, d, 0, text.size, w_pat, w_off, room, info, dist_out=w_dist if dist else None, report=report,
                       open_end=text.size, workspace=(ax.ptr, ax_bytes))

    def wild(report):
        sp, so, n = planes(report)
        m.wildcard_async(sp, so, n, d, 0, text.size, w_pat, w_off, room, info, report=report, open_end=text.size,
                         all_patterns=True, workspace=(wl.ptr, wl_bytes))
    approx(_lib.REPORT_STATE)
    out["kept_entries"] = int(w_pat.to_numpy(np.int32, 1)[0])
    out["undecided"] = int(info.to_numpy(np.int32, 4)[0])
    dist = w_dist.to_numpy(np.int32, out["kept_entries"] + 2)[1:-1]
    out["kept_by_distance"] = np.bincount(dist, minlength=k + 1).tolist()
    runs = {"scan_state": scan_state, "expand": lambda: expand(e_pat, e_off, room),
            "approx_pass_state": lambda: approx(_lib.REPORT_STATE), "approx_pass_head": lambda: approx(_lib.REPORT_HEAD),
            "approx_pass_state_no_dist": lambda: approx(_lib.REPORT_STATE, False),
            "wildcard_pass_state_all": lambda: wild(_lib.REPORT_STATE), "wildcard_pass_head_all": lambda: wild(_lib.REPORT_HEAD)}
    for f in runs.values():
        f()
    torch.cuda.synchronize()
    med, spread, n = timed(runs, seconds)
    out["runs"] = n
    out.update({key + "_us": v for key, v in med.items()})
    out.update({key + "_us_min_max": v for key, v in spread.items()})
    out["approx_over_wildcard"] = round(med["approx_pass_state"] / med["wildcard_pass_state_all"], 2)
    for b in (d, ex, two_p, two_o, e_pat, e_off, w_pat, w_off, w_dist, info, ax, wl):
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
    for k in (0, 1, 2):
        print(json.dumps(measure(pats, k, text, args.seconds)), flush=True)


if __name__ == "__main__":
    main()
