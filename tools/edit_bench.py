"""What edit-distance matching costs beside the Hamming pass: the 2000 ClamAV signatures with a budget of k = 1 and 2
each, once as Hamming patterns (acm_automaton_add_approx) and once as edit patterns (acm_automaton_add_edit); as
acm_grep -k does, a pattern shorter than 3 * (k + 1) bytes stays exact.  The pieces, the automaton, the text and the
records of the STATE scan are the same for both.  Per 32 MiB batch: the records and their list entries, what each
pass keeps, and the time of the Hamming pass, of the whole edit pass, and of the edit pass over the same planes with
the count cell set to 0 -- its order and unique step alone, whose cost is per cell ordered and not per candidate --
so that the difference is the candidates stage.  max_records is the record count, as Matcher.scan_edit sizes it.
Device events around each call, medians over repeated runs.

python tools/edit_bench.py [--seconds 0.3] >> profiles/edit_bench.jsonl
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
from approx_bench import N, timed
from gpu_pattern_matching_amd import Automaton, DeviceArray, Matcher, _lib


def build(pats, k, edit):
    a = Automaton()
    tolerant = 0
    for i, p in enumerate(pats):
        ok = len(p) >= 3 * (k + 1)
        tolerant += ok
        (a.add_edit if edit else a.add_approx)(p, k if ok else 0, i)
    a.compile()
    return a, tolerant


def measure(pats, k, text, seconds):
    out = {"workload": "clamav2000, 20000 planted", "k": k}
    runs, keep = {}, []
    d = DeviceArray.from_numpy(text)
    for name, edit in (("hamming", False), ("edit", True)):
        a, tolerant = build(pats, k, edit)
        out.update({"approximate": tolerant, "patterns": a.num_patterns, "states": a.num_states, name + "_reach": list(a.approx_reach)})
        m = Matcher(a, 0, max_text=N)
        a.close()
        for _ in range(3):
            m.scan_async(d, text.size, report=_lib.REPORT_STATE)
        out["pipeline"] = m.path_taken(text.size)
        out["records"] = records = int(m.pat_plane.to_numpy(np.int32, 1)[0])
        room = 8 * records + 2
        planes = [DeviceArray(room * 4) for _ in range(4)]
        info = DeviceArray(16)
        if not edit:
            nb = m.lib.acm_approx_workspace_bytes(records)
            ws = DeviceArray(nb)

            def hamming(m=m, planes=planes, info=info, ws=ws, nb=nb, records=records, room=room):
                m.approx_async(m.pat_plane, m.off_plane, records, d, 0, text.size, planes[0], planes[1], room, info,
                               dist_out=planes[2], report=_lib.REPORT_STATE, open_end=text.size, workspace=(ws.ptr, nb))
            hamming()
            out["hamming_kept"] = int(planes[0].to_numpy(np.int32, 1)[0])
            runs["hamming_pass"] = hamming
        else:
            nb = m.lib.acm_edit_workspace_bytes(m.dfa, records)
            ws = DeviceArray(nb)
            out["edit_workspace_MiB"] = round(nb / 2 ** 20, 1)
            # the same planes with no records: a copy whose count cell is 0
            e_pat, e_off = DeviceArray((records + 2) * 4), DeviceArray((records + 2) * 4)
            for src, dst in ((m.pat_plane, e_pat), (m.off_plane, e_off)):
                h = src.to_numpy(np.int32, records + 2).copy()
                h[0] = 0
                _lib.check(m.lib.acm_rt_memcpy_h2d(dst.ptr, h.ctypes.data, h.nbytes, None), "h2d")
            _lib.check(m.lib.acm_rt_stream_sync(None), "sync")

            def edit_pass(sp=m.pat_plane, so=m.off_plane, m=m, planes=planes, info=info, ws=ws, nb=nb, records=records, room=room):
                m.edit_async(sp, so, records, d, 0, text.size, planes[0], planes[1], room, info, dist_out=planes[2],
                             len_out=planes[3], report=_lib.REPORT_STATE, open_end=text.size, workspace=(ws.ptr, nb))
            edit_pass()
            n = int(planes[0].to_numpy(np.int32, 1)[0])
            i4 = info.to_numpy(np.int32, 4)
            out.update({"edit_records": n, "edit_candidates": int(i4[1]), "edit_undecided": int(i4[0])})
            dist = planes[2].to_numpy(np.int32, n + 2)[1:-1]
            out["edit_by_distance"] = np.bincount(dist, minlength=k + 1).tolist()
            runs["edit_pass"] = edit_pass
            runs["edit_order_unique"] = lambda f=edit_pass, a=e_pat, b=e_off: f(a, b)
            keep += [e_pat, e_off]
        keep += planes + [info, ws, m]
    for f in runs.values():
        f()
    torch.cuda.synchronize()
    med, spread, n = timed(runs, seconds)
    out["runs"] = n
    out.update({key + "_us": v for key, v in med.items()})
    out.update({key + "_us_min_max": v for key, v in spread.items()})
    out["edit_candidates_stage_us"] = round(med["edit_pass"] - med["edit_order_unique"], 1)
    out["edit_over_hamming"] = round(med["edit_pass"] / med["hamming_pass"], 2)
    for b in keep:
        (b.close if isinstance(b, Matcher) else b.free)()
    d.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3)
    args = ap.parse_args()
    path, _, _ = fixtures.set_source("clamav2000")
    pats = synth.load_hex_patterns(path, 2000)
    text = synth.clamav_corpus(N, 11, pats, 20000)
    for k in (1, 2):
        print(json.dumps(measure(pats, k, text, args.seconds)), flush=True)


if __name__ == "__main__":
    main()
