"""What the group check of the wildcard pass costs: the 2000 ClamAV signatures with every 8th byte a wildcard, as
tools/wildcard_bench.py makes them, loaded three ways in one process.  In every signature of 12 bytes or more the
first wildcard byte and the three bytes behind it (positions 7 .. 10) are
  "any"   four ??: the yardstick, the same sets and the same anchors as the two loads below
  "A"     a group of 2 alternatives of 4 bytes: the signature's own bytes and one random string
  "B"     a group of 64 alternatives: the signature's own bytes LAST, behind 63 random strings
so the three automata are the same and the loads differ by the group check alone.  Text: 32 MiB of random bytes
with 20 000 signatures planted.  Device events around each run, medians over repeated runs.

python tools/group_bench.py [--seconds 0.3] >> profiles/group_bench.jsonl
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import fixtures
import synth
from gpu_pattern_matching_amd import Automaton, DeviceArray, Matcher, _lib
from gpu_pattern_matching_amd._lib import check
from wildcard_bench import N, timed

ALTERNATIVES = {"any": 0, "A": 2, "B": 64}


def bodies(pats, kind, seed=5):
    rng = np.random.default_rng(seed)
    out, groups = [], 0
    for p in pats:
        h = ["%02x" % b for b in p]
        for i in range(7, len(p) - 1, 8):
            h[i] = "??"
        if len(p) >= 12:
            groups += 1
            if kind == "any":
                h[7:11] = ["??"] * 4
            else:
                own = "".join("%02x" % b for b in p[7:11])
                others = ["".join("%02x" % int(b) for b in rng.integers(0, 256, size=4)) for _ in range(ALTERNATIVES[kind] - 1)]
                h[7:11] = ["(" + "|".join(others + [own]) + ")"]
        out.append("".join(h))
    return out, groups


def measure(kind, sig_file, text, seconds):
    a = Automaton()
    assert a.load_signature_file(sig_file, groups=True) == 2000
    a.compile()
    out = {"load": kind, "alternatives": ALTERNATIVES[kind], "patterns": a.num_patterns, "states": a.num_states,
           "groups": sum(len(a.wildcard_groups(i)) for i in range(a.num_patterns)), "reach": list(a.wildcard_reach)}
    m = Matcher(a, 0, max_text=N)
    a.close()
    out["device_bytes"] = m.device_bytes
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
    expand(two_p, two_o, 2)
    out["list_entries"] = entries = int(two_p.to_numpy(np.int32, 1)[0])
    room = entries + 2
    e_pat, e_off, w_pat, w_off = (DeviceArray(room * 4) for _ in range(4))
    info = DeviceArray(16)
    expand(e_pat, e_off, room)
    wl_bytes = m.lib.acm_wildcard_workspace_bytes(max(cap - 2, entries))
    wl = DeviceArray(wl_bytes)

    def wild(report):
        sp, so, n = (m.pat_plane, m.off_plane, cap - 2) if report == _lib.REPORT_STATE else (e_pat, e_off, entries)
        m.wildcard_async(sp, so, n, d, 0, text.size, w_pat, w_off, room, info, report=report, open_end=text.size,
                         all_patterns=True, workspace=(wl.ptr, wl_bytes))
    wild(_lib.REPORT_HEAD)
    out["kept_entries"] = int(w_pat.to_numpy(np.int32, 1)[0])
    out["undecided"] = int(info.to_numpy(np.int32, 4)[0])
    runs = {"scan_state": scan_state, "wildcard_pass_state_all": lambda: wild(_lib.REPORT_STATE),
            "wildcard_pass_head_all": lambda: wild(_lib.REPORT_HEAD)}
    for f in runs.values():
        f()
    torch.cuda.synchronize()
    med, n = timed(runs, seconds)
    out["runs"] = n
    out.update({k + "_us": v for k, v in med.items()})
    for b in (d, ex, two_p, two_o, e_pat, e_off, w_pat, w_off, info, wl):
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
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for kind in ALTERNATIVES:
            f = os.path.join(tmp, kind + ".sig")
            lines, groups = bodies(pats, kind)
            with open(f, "w") as fh:
                fh.write("\n".join(lines) + "\n")
            row = measure(kind, f, text, args.seconds)
            row["workload"] = "clamav2000, every 8th byte ??, positions 7..10 of %d signatures %s, 20000 planted" % (
                groups, "????????" if kind == "any" else "a group of %d" % ALTERNATIVES[kind])
            rows.append(row)
    for row in rows:                                    # the group check alone: against the ?? load of this process
        for k in ("wildcard_pass_state_all_us", "wildcard_pass_head_all_us"):
            row[k.replace("_us", "_over_any")] = round(row[k] / rows[0][k], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
