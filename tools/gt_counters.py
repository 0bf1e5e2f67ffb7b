"""HBM bytes of the fused gradient-tracking round on an agent-major bank from
rocprofv3 counter runs, one run per counter with nothing traced beside it (no
tracing option in the same run; the program after `--`):
  rocprofv3 --pmc FETCH_SIZE -d DIR/FETCH_SIZE -o run --output-format csv -- python tools/gt_ab.py --layout L --legs a ...
  rocprofv3 --pmc WRITE_SIZE -d DIR/WRITE_SIZE -o run --output-format csv -- python tools/gt_ab.py --layout L --legs a ...
  python tools/gt_counters.py DIR --layout L --agents N [--params P] [--out profiles/gt_L_counters.json]
Medians per launch, in KiB, per objective, of the layout's f4 kernel: L = ring
gt_ring_dma_kernel (the objective is its second template argument), L = csr
gt_csr_xcd_kernel<GtPlain, ...> (the pinned tiles: every f4 column at P = 2^20;
its fourth), L = csr-push gt_csr_xcd_kernel<GtPushSum, ...>, the same template's
push-sum instantiations (the same tiles; the program after `--` is
then `python tools/gt_push_ab.py --legs a ...`; the n-float v' kernel and the
2 n floats of v the main kernel reads are not counted), L = extra-csr /
extra-ring the EXTRA round's instantiations of the mixing kernels themselves,
csr_xcd_kernel<32, 2, ExtraEpi<OBJ, SELF>> and ring_mix_dma_kernel<4,
ExtraEpi<OBJ, SELF>, ...> (the program after `--` is then `python
tools/extra_ab.py --legs a ...` or `--legs e ...`; the same five streams), L =
extra-pm csr_pm_extra_kernel on the parameter-major bank (the objective is its
fourth template argument; `python tools/extra_ab.py --layout pm --legs a ...`),
against the algorithmic 3 N P 4 read and 2 N P 4 written.  FETCH_SIZE counts
half the bytes of a wide streaming read on gfx950, so `read_over_algorithmic`
doubles it."""
import argparse
import csv
import glob
import json
import re
import statistics


# the measured kernel's demangled name up to its objective, the one group
KERNELS = {"ring": r"gt_ring_dma_kernel<\d+, (\d+)",
           "csr": r"gt_csr_xcd_kernel<[^,<]*\bGtPlain, \d+, \d+, (\d+)",
           "csr-push": r"gt_csr_xcd_kernel<[^,<]*\bGtPushSum, \d+, \d+, (\d+)",
           "extra-csr": r"csr_xcd_kernel<\d+, \d+, [^<]*ExtraEpi<(\d+)",
           "extra-ring": r"ring_mix_dma_kernel<\d+, [^<]*ExtraEpi<(\d+)",
           "extra-pm": r"csr_pm_extra_kernel<\d+, \d+, \d+, (\d+)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--layout", required=True, choices=sorted(KERNELS))
    ap.add_argument("--agents", type=int, required=True)
    ap.add_argument("--params", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    kernel = KERNELS[a.layout]
    vals = {}
    for f in glob.glob(f"{a.dir}/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(kernel, r["Kernel_Name"])
            if m:
                obj = ("least_squares", "logistic")[int(m.group(1))]
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
