"""HBM bytes of the fused gradient-tracking round on the agent-major CSR bank
from rocprofv3 counter runs, one run per counter with nothing traced beside it
(no tracing option in the same run; the program after `--`):
  rocprofv3 --pmc FETCH_SIZE -d DIR/FETCH_SIZE -o run --output-format csv -- python tools/gt_csr_ab.py --legs a ...
  rocprofv3 --pmc WRITE_SIZE -d DIR/WRITE_SIZE -o run --output-format csv -- python tools/gt_csr_ab.py --legs a ...
  python tools/gt_csr_counters.py DIR --agents N [--params P] [--out profiles/gt_csr_counters.json]
Medians per launch of gt_csr_xcd_kernel (the pinned tiles: every f4 column at
P = 2^20), in KiB, per objective (the kernel's third template argument),
against the algorithmic 3 N P 4 read and 2 N P 4 written.  FETCH_SIZE counts
half the bytes of a wide streaming read on gfx950, so `read_over_algorithmic`
doubles it."""
import argparse
import csv
import glob
import json
import re
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--agents", type=int, required=True)
    ap.add_argument("--params", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    vals = {}
    for f in glob.glob(f"{a.dir}/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(r"gt_csr_xcd_kernel<(\d+), (\d+), (\d+)", r["Kernel_Name"])
            if m:
                obj = ("least_squares", "logistic")[int(m.group(3))]
                vals.setdefault(obj, {}).setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    read_kib, write_kib = 3 * a.agents * a.params * 4 // 1024, 2 * a.agents * a.params * 4 // 1024
    res = {"agents": a.agents, "params": a.params, "algorithmic_read_KiB": read_kib, "algorithmic_write_KiB": write_kib,
           "note": "medians per launch, KiB; FETCH_SIZE counts half the bytes of a wide streaming read on gfx950"}
    for obj, c in vals.items():
        res[obj] = {k: {"median": statistics.median(v), "n": len(v)} for k, v in c.items()}
        if "FETCH_SIZE" in c:
            res[obj]["read_over_algorithmic"] = 2 * statistics.median(c["FETCH_SIZE"]) / read_kib
        if "WRITE_SIZE" in c:
            res[obj]["write_over_algorithmic"] = statistics.median(c["WRITE_SIZE"]) / write_kib
        if "FETCH_SIZE" in c and "WRITE_SIZE" in c:
            res[obj]["bytes_over_algorithmic"] = (2 * statistics.median(c["FETCH_SIZE"]) +
                                                  statistics.median(c["WRITE_SIZE"])) / (read_kib + write_kib)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
