"""Counters of pb_stamp_kernel: for each row config:position one
`rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVES --output-format csv`
run, with no tracing flag beside --pmc, of `scripts/stamp_bench.py --pmc` (2^22 frames, three calls
and nothing else after the build), then the kernel's mean counters and VALU instructions per frame
(wave instructions times 64 lanes over the frames: one lane owns one frame).

    python3 scripts/stamp_pmc.py DIR [--log2 22] [--rows a:head,b:tail] > profiles/stamp/stamp_pmc.jsonl

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
ROWS = ["c2_udp_64:head", "c4_tcp_syn:head", "c5_icmp_echo:head", "c2_udp_1500:head", "c3_udp_var:head", "c3_udp_var:tail"]
COUNTERS = ["SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR", "SQ_WAVES"]
KERNEL = "pb_stamp_kernel"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--log2", type=int, default=22)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()
    for item in a.rows.split(","):
        tag = item.replace(":", "_")
        out_dir, meta_path = os.path.join(a.dir, tag), os.path.join(a.dir, tag + ".json")
        cmd = ["rocprofv3", "--pmc"] + COUNTERS + ["--output-format", "csv", "-d", out_dir, "--", sys.executable,
                                                    os.path.join(ROOT, "scripts", "stamp_bench.py"), "--pmc", "--rows",
                                                    item, "--log2", str(a.log2), "--meta", meta_path]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("rocprofv3 run of %s failed (%d); stopping" % (item, r.returncode))
        meta = json.load(open(meta_path))[0]
        acc = collections.defaultdict(list)
        for path in glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if KERNEL in row["Kernel_Name"].split("(")[0]:
                    acc[row["Counter_Name"]].append(float(row["Counter_Value"]))
        if not acc:
            sys.exit("no %s rows for %s; stopping" % (KERNEL, item))
        mean = {c: round(sum(v) / len(v)) for c, v in acc.items()}
        n = meta["frames"]
        out = {"config": meta["config"], "position": meta["position"], "frames": n, "frame_bytes": meta["frame_bytes"],
               "dispatches": len(next(iter(acc.values()))), "counters_mean": mean}
        for c, key in (("SQ_INSTS_VALU", "valu_insts_per_frame"), ("SQ_INSTS_SALU", "salu_wave_insts_x64_per_frame"),
                       ("SQ_INSTS_VMEM_RD", "vmem_rd_insts_per_frame"), ("SQ_INSTS_VMEM_WR", "vmem_wr_insts_per_frame")):
            if c in mean:
                out[key] = round(mean[c] * 64 / n, 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
