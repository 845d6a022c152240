#!/usr/bin/env python3
"""Per-kernel summary of a `rocprofv3 --kernel-trace --output-format csv` run: dispatches, total and mean time, workgroups,
LDS, VGPRs and scratch as dispatched, one line per kernel and workgroup count, sorted by total time.

    python tools/kernel_trace_summary.py <directory rocprofv3 wrote to> [substring ...]
"""
import collections
import csv
import glob
import os
import re
import sys


def pick(row, *names, default=0):
    for n in names:
        if n in row and row[n] != "":
            return row[n]
    return default


def main():
    root, subs = sys.argv[1], sys.argv[2:]
    files = glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {root}")
    groups = collections.defaultdict(lambda: [0, 0.0])
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = pick(row, "Kernel_Name", default="?").replace("(anonymous namespace)::", "").replace(" [clone .kd]", "")
                name = re.sub(r"\(.*", "", name).replace("void ", "").replace("pfhe::", "")
                if subs and not any(s in name for s in subs):
                    continue
                wg = int(pick(row, "Workgroup_Size_X", "Workgroup_Size", default=1)) or 1
                grid = int(pick(row, "Grid_Size_X", "Grid_Size", default=0))
                grid_y = int(pick(row, "Grid_Size_Y", default=1)) or 1
                wgy = int(pick(row, "Workgroup_Size_Y", default=1)) or 1
                key = (name, (grid // wg) * (grid_y // wgy), int(pick(row, "LDS_Block_Size", "LDS_Block_Size_v", default=0)),
                       int(pick(row, "VGPR_Count", "Arch_VGPR_Count", default=0)), int(pick(row, "Scratch_Size", default=0)))
                g = groups[key]
                g[0] += 1
                g[1] += (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
    print("# dispatches   total_us    mean_us  workgroups      lds  vgpr scratch  kernel")
    for (name, wgs, lds, vgpr, scratch), (count, total) in sorted(groups.items(), key=lambda kv: -kv[1][1]):
        print(f"{count:12d} {total:10.1f} {total / count:10.2f} {wgs:11d} {lds:8d} {vgpr:5d} {scratch:7d}  {name}")


if __name__ == "__main__":
    main()
