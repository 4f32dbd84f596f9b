"""Counters of pbgpu_segment's kernels: for each config:mss[:nocsum] one
`rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES --output-format csv` run, with no
tracing flag beside --pmc, of `scripts/seg_bench.py --pmc` (2^22 frames, 2^19 for the 9-KB configs,
three calls and nothing else after the build), then per kernel the mean counters; for the writer
wave-instructions per output byte and VALU instructions per 16-B chunk, as scripts/frag_pmc.py gives
them for pb_frag_kernel, and for the sum pass VALU instructions per 16-B chunk of source payload.

    python3 scripts/seg_pmc.py DIR [--log2 22] [--configs a:1472,b:536] > profiles/seg/seg_pmc.jsonl

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
CONFIGS = ["udp_jumbo_fixed_odd:1472", "tcp_jumbo_fixed_odd:1460", "c2_udp_1500:536", "c3_udp_var:536", "c2_udp_64:1460",
           "udp_jumbo_fixed_odd:1472:nocsum"]
COUNTERS = ["SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_WAVES"]
KERNELS = ["pb_seg_count_kernel", "pb_seg_map_kernel", "pb_seg_sum_kernel", "pb_frag_copy_kernel",
           "pb_seg_kernel"]  # the writer last


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
                                                    os.path.join(ROOT, "scripts", "seg_bench.py"), "--pmc", "--configs",
                                                    item, "--log2", str(a.log2), "--meta", meta_path]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("rocprofv3 run of %s failed (%d); stopping" % (item, r.returncode))
        meta = json.load(open(meta_path))[0]
        acc = {k: collections.defaultdict(list) for k in KERNELS}
        for path in glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row["Kernel_Name"].split("(")[0]
                for k in KERNELS:
                    if k in name:
                        acc[k][row["Counter_Name"]].append(float(row["Counter_Value"]))
                        break
        writer = "pb_frag_copy_kernel" if acc["pb_frag_copy_kernel"] else "pb_seg_kernel"
        if not acc[writer]:
            sys.exit("no writer rows for %s; stopping" % item)
        b = meta["out_bytes"]
        out = {"config": meta["config"], "mss": meta["mss"], "no_l4_csum": meta["no_l4_csum"], "frames": meta["frames"],
               "frame_bytes": meta["frame_bytes"], "out_frames": meta["out_frames"], "out_bytes": b, "writer": writer,
               "kernels": {}}
        for k in KERNELS:
            if acc[k]:
                out["kernels"][k] = {"dispatches": len(next(iter(acc[k].values()))),
                                     "counters_mean": {c: round(sum(v) / len(v)) for c, v in acc[k].items()}}
        mean = out["kernels"][writer]["counters_mean"]
        for c, key in (("SQ_INSTS_VALU", "valu_wave_insts_per_out_byte"), ("SQ_INSTS_SALU", "salu_wave_insts_per_out_byte"),
                       ("SQ_INSTS_LDS", "lds_wave_insts_per_out_byte")):
            if c in mean:
                out[key] = round(mean[c] / b, 5)
        if "SQ_INSTS_VALU" in mean:
            out["valu_wave_insts_per_16B_chunk_lane"] = round(mean["SQ_INSTS_VALU"] * 64 / (b / 16), 1)
        if acc["pb_seg_sum_kernel"] and "SQ_INSTS_VALU" in out["kernels"]["pb_seg_sum_kernel"]["counters_mean"]:
            out["sum_valu_wave_insts_per_16B_source_chunk_lane"] = round(
                out["kernels"]["pb_seg_sum_kernel"]["counters_mean"]["SQ_INSTS_VALU"] * 64 / (meta["frame_bytes"] / 16), 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
