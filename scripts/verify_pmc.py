"""Counters of the verify kernels from `rocprofv3 --pmc ... --output-format csv` runs of
`scripts/verify_bench.py --pmc` (one run per config and counter group, no tracing flags beside
--pmc): fetched bytes over frame bytes and VALU / LDS wave-instructions per frame byte.

    python3 scripts/verify_pmc.py DIR > profiles/verify/verify_pmc.jsonl

DIR holds <config>.json (verify_bench.py --meta) and <config>_<group>/**/*counter_collection.csv.
FETCH_SIZE is in KiB and, on gfx950, reports half of what a wide streaming read fetches: it is
doubled here (the raw figure is kept beside it)."""
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
            k = r["Kernel_Name"]
            if "pb_vpg_kernel" in k or "pb_vst_kernel" in k:
                kernel = k.split("(")[0]
                acc[r["Counter_Name"]].append(float(r["Counter_Value"]))
    if not acc:
        continue
    mean = {c: sum(v) / len(v) for c, v in acc.items()}
    out = {"config": name, "kernel": kernel, "frames": meta["frames"], "frame_bytes": meta["bytes"],
           "dispatches": {c: len(v) for c, v in acc.items()}, "counters_mean": {c: round(v) for c, v in mean.items()}}
    b = meta["bytes"]
    if "FETCH_SIZE" in mean:
        out["fetch_size_bytes_raw"] = round(mean["FETCH_SIZE"] * 1024)
        out["fetched_over_frame_bytes"] = round(2 * mean["FETCH_SIZE"] * 1024 / b, 4)
    for c, key in (("SQ_INSTS_VALU", "valu_wave_insts_per_byte"), ("SQ_INSTS_LDS", "lds_wave_insts_per_byte"),
                   ("SQ_INSTS_SALU", "salu_wave_insts_per_byte")):
        if c in mean:
            out[key] = round(mean[c] / b, 5)
    if "SQ_LDS_BANK_CONFLICT" in mean and "SQ_LDS_IDX_ACTIVE" in mean and mean["SQ_LDS_IDX_ACTIVE"]:
        out["lds_bank_conflict_over_active"] = round(mean["SQ_LDS_BANK_CONFLICT"] / mean["SQ_LDS_IDX_ACTIVE"], 4)
    print(json.dumps(out))
