"""Counters of pb_wire_kernel: for each row one
`rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES --output-format csv` run, with no
tracing flag beside --pmc, of `scripts/wire_bench.py --pmc` (2^22 frames, 2^19 of 9043 B; three calls
and nothing else after the build and repack), then wave-instructions per frame byte and the wave
count, as scripts/verify_pmc.py gives them for pb_vst_kernel.

    python3 scripts/wire_pmc.py DIR [--log2 22] [--rows a,b] > profiles/wire/wire_pmc.jsonl

This process does not open the GPU; each profiled run is a child of its own."""
import argparse
import collections
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ["c2_udp_64", "c4_tcp_syn", "c5_icmp_echo", "c2_udp_1500", "c3_udp_var", "c2_udp_64+vxlan", "c2_udp_1500+vxlan",
        "c2_udp_64+xlat6", "udp_jumbo_fixed_odd+fragment1500"]
COUNTERS = ["SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_WAVES"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--log2", type=int, default=22)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()
    for row in a.rows.split(","):
        tag = row.replace("+", "_")
        out_dir, meta_path = os.path.join(a.dir, tag), os.path.join(a.dir, tag + ".json")
        log2 = a.log2 - 3 if row.startswith("udp_jumbo") else a.log2
        cmd = ["rocprofv3", "--pmc"] + COUNTERS + ["--output-format", "csv", "-d", out_dir, "--", sys.executable,
                                                    os.path.join(ROOT, "scripts", "wire_bench.py"), "--pmc", "--rows", row,
                                                    "--log2", str(log2), "--meta", meta_path]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("rocprofv3 run of %s failed (%d); stopping" % (row, r.returncode))
        meta = json.load(open(meta_path))[0]
        acc, kernel = collections.defaultdict(list), None
        for path in glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"), recursive=True):
            for rec in csv.DictReader(open(path)):
                if "pb_wire_kernel" in rec["Kernel_Name"]:
                    kernel = rec["Kernel_Name"].split("(")[0]
                    acc[rec["Counter_Name"]].append(float(rec["Counter_Value"]))
        if not acc:
            sys.exit("no pb_wire_kernel rows for %s; stopping" % row)
        mean = {c: sum(v) / len(v) for c, v in acc.items()}
        b = meta["bytes"]
        out = {"row": row, "kernel": kernel, "frames": meta["frames"], "frame_bytes": b,
               "dispatches": {c: len(v) for c, v in acc.items()}, "counters_mean": {c: round(v) for c, v in mean.items()}}
        for c, key in (("SQ_INSTS_VALU", "valu_wave_insts_per_byte"), ("SQ_INSTS_SALU", "salu_wave_insts_per_byte"),
                       ("SQ_INSTS_LDS", "lds_wave_insts_per_byte")):
            if c in mean:
                out[key] = round(mean[c] / b, 5)
        if "SQ_INSTS_VALU" in mean:
            out["valu_wave_insts_per_frame"] = round(mean["SQ_INSTS_VALU"] / meta["frames"], 2)
        if "SQ_WAVES" in mean:
            out["waves"] = round(mean["SQ_WAVES"])
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
