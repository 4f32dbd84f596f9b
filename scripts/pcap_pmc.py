"""Counters of pb_pcap_kernel from `rocprofv3 --pmc ... --output-format csv` runs of
`scripts/pcap_bench.py --pmc` (one run per config and counter group, no tracing flags beside
--pmc): wave-instructions per stream byte and, where collected, fetched and written bytes over the
frame and stream bytes.

    python3 scripts/pcap_pmc.py DIR > profiles/pcap/pcap_pmc.jsonl

DIR holds <config>.json (pcap_bench.py --meta) and <config>_<group>/**/*counter_collection.csv.
FETCH_SIZE and WRITE_SIZE are in KiB; the raw figures are kept (scripts/verify_pmc.py notes that
FETCH_SIZE reports half of a wide streaming read on gfx950)."""
import collections
import csv
import glob
import json
import os
import sys

d = sys.argv[1]
for meta_path in sorted(glob.glob(os.path.join(d, "*.json"))):
    meta = json.load(open(meta_path))[0]
    name = meta["config"]
    acc = collections.defaultdict(list)
    kernel = None
    for path in glob.glob(os.path.join(d, name + "_*", "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "pb_pcap_kernel" in r["Kernel_Name"]:
                kernel = r["Kernel_Name"].split("(")[0]
                acc[r["Counter_Name"]].append(float(r["Counter_Value"]))
    if not acc:
        continue
    mean = {c: sum(v) / len(v) for c, v in acc.items()}
    b = meta["stream_bytes"]
    out = {"config": name, "kernel": kernel, "frames": meta["frames"], "frame_bytes": meta["frame_bytes"],
           "stream_bytes": b, "dispatches": {c: len(v) for c, v in acc.items()},
           "counters_mean": {c: round(v) for c, v in mean.items()}}
    for c, key in (("SQ_INSTS_VALU", "valu_wave_insts_per_stream_byte"), ("SQ_INSTS_LDS", "lds_wave_insts_per_stream_byte"),
                   ("SQ_INSTS_SALU", "salu_wave_insts_per_stream_byte"),
                   ("SQ_INSTS_VMEM_RD", "vmem_rd_wave_insts_per_stream_byte"),
                   ("SQ_INSTS_VMEM_WR", "vmem_wr_wave_insts_per_stream_byte")):
        if c in mean:
            out[key] = round(mean[c] / b, 5)
    if "SQ_INSTS_VALU" in mean:
        out["valu_wave_insts_per_16B_chunk_lane"] = round(mean["SQ_INSTS_VALU"] * 64 / (b / 16), 1)
    if "FETCH_SIZE" in mean:
        out["fetch_size_bytes_raw_over_frame_bytes"] = round(mean["FETCH_SIZE"] * 1024 / meta["frame_bytes"], 4)
    if "WRITE_SIZE" in mean:
        out["write_size_bytes_raw_over_stream_bytes"] = round(mean["WRITE_SIZE"] * 1024 / b, 4)
    print(json.dumps(out))
