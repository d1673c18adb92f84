"""Which scan-path kernel instantiations a rocprofv3 kernel-stats CSV never saw.

    python tools/variant_coverage.py profiles/variant_kernel_stats.csv

Lists the instantiations of the scan-path kernel families in the built library (every __global__
instantiation in its gfx950 code object has a host-side handle; `nm -C` names them the way rocprofv3
does) and prints each one that has no row in the CSV.  The debugging-only instantiations below are
reported as excluded, with the reason; the exit status is 1 when anything else is missing.
"""
import csv
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gpu_pattern_matching_amd", "libacmatch.so")

# the kernels a scan can launch: both pipelines, the chain scatter's block-total scans, all-patterns
# expansion and the segment pass
FAMILIES = ("k_sieve", "k_sieve_check", "k_sieve_emit", "k_spec_walk", "k_halo_walk", "k_probe", "k_resolve",
            "k_scan_top", "k_scatter_all", "k_scan_block", "k_scan_add", "k_lds_walk", "k_lds_scatter",
            "k_lds_scatter_wide", "k_expand_count", "k_expand_scatter", "k_segment")

EXCLUDED = [   # (pattern over the short name, reason)
    (r"^k_sieve<\d+, true, ", "clock stamps: only with ACM_SIEVE_STAMPS, a debugging aid"),
    (r"^k_lds_walk<2, false, 6>$", "the compiler's version of the LDS step: only with ACM_LDS_NOASM, a debugging aid"),
    (r"^k_lds_scatter<2, 1024>$", "the plain LDS scatter: only with ACM_LDS_SCATTER_BLOCK=1024, a debugging aid"),
]


def short(name):
    """'void (anonymous namespace)::k_sieve<8, false, 3, false>((anonymous namespace)::SieveGroup)' ->
    'k_sieve<8, false, 3, false>'"""
    name = name.replace("(anonymous namespace)::", "")
    name = re.sub(r"^void ", "", name)
    return re.sub(r"\(.*\)$", "", name).strip()


def family(s):
    return s.split("<", 1)[0]


def built(lib=LIB):
    out = subprocess.run(["nm", "-C", lib], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ [dD] (.*\(.*\))$", line)
        if m:
            s = short(m.group(1))
            if family(s) in FAMILIES:
                names.add(s)
    return sorted(names)


def seen(csv_path):
    with open(csv_path, newline="") as f:
        return {short(r["Name"]) for r in csv.DictReader(f) if int(r.get("Calls", "1") or 0) > 0}


def main(argv):
    if len(argv) < 2:
        print(__doc__.strip())
        return 2
    have = built(argv[2] if len(argv) > 2 else LIB)
    got = seen(argv[1])
    missing, excluded = [], []
    for k in have:
        if k in got:
            continue
        why = next((r for p, r in EXCLUDED if re.search(p, k)), None)
        (excluded if why else missing).append((k, why))
    print("%d scan-path instantiations built, %d run" % (len(have), len(have) - len(missing) - len(excluded)))
    for k, why in excluded:
        print("excluded  %-44s %s" % (k, why))
    for k, _ in missing:
        print("NOT RUN   %s" % k)
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
