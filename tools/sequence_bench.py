"""What the sequence pass costs: acm_sequence_matches_async per 32 MiB batch beside the expansion and the
position pass over the same pattern-form planes, in one process.  The set is the 2000 ClamAV signatures three
times: as 1-part sequences, and cut into 2 and into 4 parts joined by {0-64} gaps (14000 patterns, 6000
sequences, 4 levels).  Two workloads: random bytes with 200 planted signatures (few records: the pass costs its
launches) and a dense text with 200000 planted (every plant is seven part records and three matches).  The
pass orders max_records cells, so it is given the planes' record count rounded up to 4096, as a caller who
sizes its planes would.  Device events around each run, medians over repeated runs, one JSON line.

python tools/sequence_bench.py [--seconds 0.5] [--planted 200 200000] >> profiles/sequence_bench.jsonl
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

N = 32 << 20
PIECE = 64 << 10


def cut(body, k):
    """the hex body cut into k parts of whole bytes, {0-64} between them; None when a part would have under 3 bytes"""
    n = len(body) // 2
    if n < 3 * k:
        return None
    at = [2 * (n * j // k) for j in range(k + 1)]
    return "{0-64}".join(body[at[j]:at[j + 1]] for j in range(k))


def signature_file(bodies):
    lines = []
    for k in (1, 2, 4):
        lines += [s for s in (cut(b, k) for b in bodies) if s]
    f = tempfile.NamedTemporaryFile("w", suffix=".sig", delete=False)
    f.write("\n".join(lines) + "\n")
    f.close()
    return f.name


def measure(name, sig_path, text, seconds):
    a = Automaton()
    sequences = a.load_signature_file(sig_path)
    a.compile()
    for i in range(0, a.num_patterns, 10):                 # every tenth pattern has a window: the yardstick's work
        a.set_position(i, 0, 1 << 20)
    m = Matcher(a, 0, max_text=N)
    patterns = a.num_patterns
    levels = max(len(a.sequence(i)[0]) for i in range(sequences))
    a.close()
    cap = m.plane_capacity
    acap = 4 * cap
    d = DeviceArray.from_numpy(text)
    starts = np.arange(0, text.size, PIECE, dtype=np.int32)
    d_st = DeviceArray.from_numpy(starts, pad_to=0)
    xp, xo, pat, off, info = (DeviceArray(acap * 4), DeviceArray(acap * 4), DeviceArray(acap * 4), DeviceArray(acap * 4),
                              DeviceArray(16))
    nb_ex = m.lib.acm_expand_workspace_bytes(cap - 2)
    ws_ex = DeviceArray(nb_ex)

    def scan_state():
        m.scan_async(d, text.size, report=_lib.REPORT_STATE)

    def expand():
        _lib.check(m.lib.acm_expand_matches_async(m.dfa, m.pat_plane.ptr, m.off_plane.ptr, cap - 2, xp.ptr, xo.ptr, acap,
                                                  ws_ex.ptr, nb_ex, m.stream), "acm_expand_matches_async")

    scan_state()
    expand()
    entries = int(xp.to_numpy(np.int32, 1)[0])
    assert entries <= acap - 2
    mr = (entries + 4096) & ~4095
    nb_pos, nb_seq = m.lib.acm_position_workspace_bytes(mr), m.lib.acm_sequence_workspace_bytes(m.dfa, mr)
    ws_pos, ws_seq = DeviceArray(nb_pos), DeviceArray(nb_seq)

    def position():
        m.position_async(xp, xo, mr, pat, off, acap, info, report=_lib.REPORT_HEAD, seg_start=d_st, segments=starts.size,
                         text_end=text.size, open_end=text.size, all_patterns=True, workspace=(ws_pos.ptr, nb_pos))

    def sequence():
        m.sequence_async(xp, xo, mr, pat, off, acap, info, seg_start=d_st, segments=starts.size, text_end=text.size,
                         workspace=(ws_seq.ptr, nb_seq))

    runs = {"scan_state": scan_state, "expand": expand, "position_pass_heads_all": position, "sequence_pass": sequence}
    for f in runs.values():   # warm-up (AUTO settles on its pipeline)
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    pipeline = m.path_taken(text.size)
    sequence()
    matches = int(pat.to_numpy(np.int32, 1)[0])
    seq_info = info.to_numpy(np.int32, 4).tolist()
    position()
    kept = int(pat.to_numpy(np.int32, 1)[0])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = {k: [] for k in runs}
    spent = 0.0
    while spent < len(runs) * seconds or len(t["scan_state"]) < 20:
        for key, f in runs.items():   # (xp, xo hold the last expansion: the passes only read them)
            ev[0].record()
            f()
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1])
            t[key].append(ms)
            spent += ms / 1e3
    med = {k: round(float(np.median(v)) * 1e3, 1) for k, v in t.items()}
    # the launches as csrc/sequence.hip enqueues them (radix_passes() and the launch list in its header comment):
    # one 8-bit pass per byte of the slot count, a slot per part; every pattern of this set is a part
    slots = patterns
    passes = 1 + (slots >> 8 != 0) + (slots >> 16 != 0) + (slots >> 24 != 0)
    out = {"workload": name, "pipeline": pipeline, "patterns": patterns, "sequences": sequences, "levels": levels,
           "starts": int(starts.size), "list_entries": entries, "max_records": mr, "part_records": seq_info[0],
           "alive_records": seq_info[1], "sequence_matches": matches, "position_kept": kept,
           "sequence_launches": 4 + 3 * passes + 2 * levels, "radix_passes": passes, "position_launches": 2,
           "sequence_workspace_bytes": int(nb_seq), "runs": len(t["scan_state"])}
    out.update({k + "_us": v for k, v in med.items()})
    out["sequence_over_position"] = round(med["sequence_pass"] / med["position_pass_heads_all"], 2)
    for b in (d, d_st, xp, xo, pat, off, info, ws_ex, ws_pos, ws_seq):
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
        name = "clamav2000 x (1, 2, 4 parts), %d planted" % planted
        rows.append(measure(name, sig_path, synth.clamav_corpus(N, 11, clam, planted), args.seconds))
    os.unlink(sig_path)
    print(json.dumps({"tool": "sequence_bench", "batch_bytes": N, "workloads": rows}), flush=True)


if __name__ == "__main__":
    main()
