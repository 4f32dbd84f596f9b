"""Counters of pb_xlat_kernel and pb_xlat_class_kernel: for each config one
`rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES --output-format csv` run, with no
tracing flag beside --pmc, of `scripts/xlat_bench.py --pmc` (2^22 frames, three translations and
nothing else after the build), then wave-instructions per output byte and VALU instructions per
16-B chunk of the writer, as scripts/encap_pmc.py gives them for pb_encap_kernel, and the classify
pass's VALU instructions per frame.

    python3 scripts/xlat_pmc.py DIR [--log2 22] [--configs a,b] > profiles/xlat/xlat_pmc.jsonl

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
CONFIGS = ["c2_udp_64", "c4_tcp_syn", "c5_icmp_echo", "c2_udp_1500", "c3_udp_var"]
COUNTERS = ["SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_WAVES"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--log2", type=int, default=22)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()
    for item in a.configs.split(","):
        out_dir, meta_path = os.path.join(a.dir, item), os.path.join(a.dir, item + ".json")
        cmd = ["rocprofv3", "--pmc"] + COUNTERS + ["--output-format", "csv", "-d", out_dir, "--", sys.executable,
                                                    os.path.join(ROOT, "scripts", "xlat_bench.py"), "--pmc", "--configs",
                                                    item, "--log2", str(a.log2), "--meta", meta_path]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("rocprofv3 run of %s failed (%d); stopping" % (item, r.returncode))
        meta = json.load(open(meta_path))[0]
        acc = {"pb_xlat_kernel": collections.defaultdict(list), "pb_xlat_class_kernel": collections.defaultdict(list)}
        names = {}
        for path in glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for k in acc:
                    if k + "<" in row["Kernel_Name"] or row["Kernel_Name"].split("(")[0].endswith(k):
                        names[k] = row["Kernel_Name"].split("(")[0]
                        acc[k][row["Counter_Name"]].append(float(row["Counter_Value"]))
        if not acc["pb_xlat_kernel"]:
            sys.exit("no pb_xlat_kernel rows for %s; stopping" % item)
        b, n = meta["out_bytes"], meta["frames"]
        out = {"config": meta["config"], "frames": n, "frame_bytes": meta["frame_bytes"], "out_bytes": b}
        for k, tag in (("pb_xlat_kernel", "writer"), ("pb_xlat_class_kernel", "classify")):
            mean = {c: sum(v) / len(v) for c, v in acc[k].items()}
            out[tag] = {"kernel": names.get(k), "dispatches": {c: len(v) for c, v in acc[k].items()},
                        "counters_mean": {c: round(v) for c, v in mean.items()}}
            if tag == "writer":
                for c, key in (("SQ_INSTS_VALU", "valu_wave_insts_per_out_byte"),
                               ("SQ_INSTS_SALU", "salu_wave_insts_per_out_byte"),
                               ("SQ_INSTS_LDS", "lds_wave_insts_per_out_byte")):
                    if c in mean:
                        out[tag][key] = round(mean[c] / b, 5)
                if "SQ_INSTS_VALU" in mean:
                    out[tag]["valu_wave_insts_per_16B_chunk_lane"] = round(mean["SQ_INSTS_VALU"] * 64 / (b / 16), 1)
            elif "SQ_INSTS_VALU" in mean:
                out[tag]["valu_wave_insts_per_frame_lane"] = round(mean["SQ_INSTS_VALU"] * 64 / n, 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
