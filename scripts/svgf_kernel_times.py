#!/usr/bin/env python3
"""svgf_kernel_times.py DB -- per-kernel times of a `rocprofv3 --kernel-trace --stats -- python3 scripts/svgf_time.py [--five]` run, from
its results database: every svgf_prep_kernel launch opens a chain whose svgf_iter_kernel launches are iterations 0, 1, ...; the chains
are grouped by frame, by where the taps came from (the kernels' template arguments), by whether a variance was given and by their
length, and each kernel's median and minimum over the group are printed in microseconds, beside the a-trous denoiser's iterations and
the feature pass of the same run.  DESIGN.md 4.11 quotes the medians."""
import re
import sqlite3
import statistics
import sys
from collections import defaultdict


def main(path):
    db = sqlite3.connect(path)
    rows = [(n.replace("void ", "").split("(")[0], gx, gy, d) for n, gx, gy, d in
            db.execute("select name, grid_x, grid_y, end - start from kernels order by start")]
    groups = defaultdict(list)
    i = 0
    while i < len(rows):
        name, gx, gy, dur = rows[i]
        frame = f"{gx}x{gy} threads"
        if name.startswith("svgf_prep_kernel"):
            have_var, tile = re.match(r"svgf_prep_kernel<(\w+), (\w+)>", name).groups()
            j = i + 1
            while j < len(rows) and rows[j][0].startswith("svgf_iter_kernel"):
                j += 1
            chain = rows[i + 1:j]
            tiles = "".join(re.match(r"svgf_iter_kernel<\w+, (\d)>", c[0]).group(1) for c in chain[:2])
            key = (frame, f"prep tile {tile}, iteration tiles {tiles}", "variance" if have_var == "true" else "no variance", len(chain))
            groups[key + ("prepare", name)].append(dur)
            for k, c in enumerate(chain):
                groups[key + (f"iteration {k}", c[0])].append(c[3])
            i = j
            continue
        if name.startswith("atrous_kernel"):
            j = i
            while j < len(rows) and rows[j][0].startswith("atrous_kernel"):
                j += 1
                if rows[j - 1][0].endswith(", true>"):
                    break
            for k, c in enumerate(rows[i:j]):
                groups[(frame, "a-trous denoiser", "", j - i, f"iteration {k}", c[0])].append(c[3])
            i = j
            continue
        if name.startswith(("feat_kernel", "tacc_kernel")):
            groups[(frame, name, "", 0, "", name)].append(dur)
        i += 1
    for k, v in sorted(groups.items()):
        print(f"{k[0]:<20} {k[1]:<38} {k[2]:<12} n={k[3]} {k[4]:<12} {k[5]:<32} runs {len(v):3d}  median {statistics.median(v) / 1e3:8.1f} us  "
              f"min {min(v) / 1e3:8.1f} us")


if __name__ == "__main__":
    main(sys.argv[1])
