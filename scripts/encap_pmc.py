"""Counters of pb_encap_kernel: for each config:mode one
`rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES --output-format csv` run, with no
tracing flag beside --pmc, of `scripts/encap_bench.py --pmc` (2^22 frames, three encapsulations and
nothing else after the build), then wave-instructions per output byte and VALU instructions per
16-B chunk, as scripts/pcap_pmc.py gives them for pb_pcap_kernel.

    python3 scripts/encap_pmc.py DIR [--log2 22] [--configs a:vxlan,b:vlan] > profiles/encap/encap_pmc.jsonl

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
CONFIGS = ["c2_udp_64:vxlan", "c2_udp_1500:vxlan", "c3_udp_var:vxlan", "c2_udp_64:vlan"]
COUNTERS = ["SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_WAVES"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--log2", type=int, default=22)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()
    for item in a.configs.split(","):
        tag = item.replace(":", "_")
        out_dir, meta_path = os.path.join(a.dir, tag), os.path.join(a.dir, tag + ".json")
        cmd = ["rocprofv3", "--pmc"] + COUNTERS + ["--output-format", "csv", "-d", out_dir, "--", sys.executable,
                                                    os.path.join(ROOT, "scripts", "encap_bench.py"), "--pmc", "--configs",
                                                    item, "--log2", str(a.log2), "--meta", meta_path]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("rocprofv3 run of %s failed (%d); stopping" % (item, r.returncode))
        meta = json.load(open(meta_path))[0]
        acc = collections.defaultdict(list)
        kernel = None
        for path in glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if "pb_encap_kernel" in row["Kernel_Name"]:
                    kernel = row["Kernel_Name"].split("(")[0]
                    acc[row["Counter_Name"]].append(float(row["Counter_Value"]))
        if not acc:
            sys.exit("no pb_encap_kernel rows for %s; stopping" % item)
        mean = {c: sum(v) / len(v) for c, v in acc.items()}
        b = meta["out_bytes"]
        out = {"config": meta["config"], "mode": meta["mode"], "kernel": kernel, "frames": meta["frames"],
               "frame_bytes": meta["frame_bytes"], "out_bytes": b, "dispatches": {c: len(v) for c, v in acc.items()},
               "counters_mean": {c: round(v) for c, v in mean.items()}}
        for c, key in (("SQ_INSTS_VALU", "valu_wave_insts_per_out_byte"), ("SQ_INSTS_SALU", "salu_wave_insts_per_out_byte"),
                       ("SQ_INSTS_LDS", "lds_wave_insts_per_out_byte")):
            if c in mean:
                out[key] = round(mean[c] / b, 5)
        if "SQ_INSTS_VALU" in mean:
            out["valu_wave_insts_per_16B_chunk_lane"] = round(mean["SQ_INSTS_VALU"] * 64 / (b / 16), 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
