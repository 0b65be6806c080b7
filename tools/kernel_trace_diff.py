"""Do two `rocprofv3 --kernel-trace` runs of one program launch the same kernels?  (profiles/r13/README.md (b).)

    python tools/kernel_trace_diff.py DIR_A DIR_B [--out FILE.json]

Reads every `*kernel_trace.csv` below each directory (one per traced process), orders each by dispatch id and compares the lists of
(kernel name, grid x / y / z, workgroup x / y / z, LDS bytes) position by position, process files paired by size.  Prints the counts and
the first differences, and how often each kernel of csrc/unwarp.hip ran; exit status 1 if a dispatch differs."""
import argparse
import collections
import csv
import glob
import json
import os
import sys


# csrc/unwarp.hip's kernels, counted apart in the summary (torch's own kernels also live in unnamed namespaces: names, not namespaces)
UNWARP_KERNELS = ("inverse_index_kernel", "inverse_owner_kernel", "inverse_grid_kernel", "fill_row_nearest_kernel", "fill_col_nearest_kernel",
                  "fill_copy_kernel", "unwarp_decide_kernel", "unwarp_label_kernel", "unwarp_count_kernel", "class_area_sampled_kernel",
                  "unwarp_area_finalize_kernel", "unwarp_trim_finalize_kernel", "unwarp_count_finalize_kernel", "unwarp_accuracy_kernel",
                  "trimap_row_kernel", "trimap_col_kernel")


def short(name):
    return name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]


def dispatches(path):
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"], r["Workgroup_Size_Y"],
             r["Workgroup_Size_Z"], r.get("LDS_Block_Size", "")) for r in rows]


def load(directory):
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    return sorted((dispatches(f) for f in files), key=len, reverse=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    A, B = load(args.a), load(args.b)
    res = {"processes": [len(A), len(B)], "dispatches": [sum(map(len, A)), sum(map(len, B))], "differ": 0, "first_differences": []}
    if len(A) != len(B) or not A:
        res["differ"] = -1
    else:
        for pa, pb in zip(A, B):
            for i in range(max(len(pa), len(pb))):
                da, db = (pa[i] if i < len(pa) else None), (pb[i] if i < len(pb) else None)
                if da != db:
                    res["differ"] += 1
                    if len(res["first_differences"]) < 10:
                        res["first_differences"].append({"index": i, "a": da, "b": db})
    names = collections.Counter(short(d[0]) for p in A for d in p)
    res["unwarp_kernels"] = {k: v for k, v in sorted(names.items()) if k.split("<")[0] in UNWARP_KERNELS}
    res["unwarp_dispatches"] = sum(res["unwarp_kernels"].values())
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if res["differ"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
