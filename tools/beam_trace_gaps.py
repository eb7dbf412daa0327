"""Per-frame timeline of rnnt_beam_decode from a rocprofv3 --kernel-trace CSV (<prefix>_kernel_trace.csv): durations of the
beam_chain and beam_merge_dev launches of the device path and the idle gaps chain -> merge and merge -> next chain (medians and
sums).
usage: python tools/beam_trace_gaps.py <kernel_trace.csv>  -> one JSON line"""
import csv
import json
import statistics
import sys


def main(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    short = lambda n: n.split("(")[0].split("<")[0].strip()
    k = [(a, b, short(n)) for a, b, n in rows]
    out = {}

    def summ(v):
        return {"n": len(v), "median_us": round(statistics.median(v) / 1e3, 2) if v else None, "sum_ms": round(sum(v) / 1e6, 3)}
    # device path: beam_chain immediately followed by beam_merge_dev
    dur_c, dur_m, gap_cm, gap_mc = [], [], [], []
    for i in range(len(k) - 1):
        a0, b0, n0 = k[i]
        a1, b1, n1 = k[i + 1]
        if n0 == "beam_chain" and n1 == "beam_merge_dev":
            dur_c.append(b0 - a0)
            dur_m.append(b1 - a1)
            gap_cm.append(a1 - b0)
            if i + 2 < len(k) and k[i + 2][2] == "beam_chain":
                gap_mc.append(k[i + 2][0] - b1)
    out["device_path"] = {"beam_chain": summ(dur_c), "beam_merge_dev": summ(dur_m), "gap_chain_to_merge": summ(gap_cm),
                          "gap_merge_to_next_chain": summ(gap_mc)}
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1])
