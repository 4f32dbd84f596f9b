"""End-to-end rate of `pcktbatch-gpu --pcapdump FILE` beside `--pcap FILE` with the same arguments
(DESIGN.md 5.9): 64-B UDP, --maxpckts 2^LOG2, --delay 0, one thread, the file on tmpfs.

    python3 scripts/pcap_e2e.py [--log2 24] [--dir /dev/shm] [--pcap-bin OTHER/bin/pcktbatch-gpu]
                                [--pcap-label TEXT] [--reps 3] [--out FILE.json]

--pcap-bin: the binary timed for --pcap (a build of the commit before --pcapdump existed, for the
recorded comparison); default: this tree's.  Wall time of the whole process, start-up included;
frames per second = frames in the file / wall time.  Each file's record count and size are checked
and the file removed.  One JSON object on stdout and in --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pb-af-xdp_amd"))

import pb_configs as pc  # noqa: E402

BIN = os.path.join(ROOT, "pb-af-xdp_amd", "bin", "pcktbatch-gpu")


def timed(cmd, path, n):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    dt = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    size = os.path.getsize(path)
    os.remove(path)
    assert size == 24 + 80 * n, (size, n)
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=24)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--pcap-bin", default=BIN)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gpubatch", default="1048576")
    ap.add_argument("--pcap-label", default="this tree", help="what --pcap-bin is, for the record")
    ap.add_argument("--out")
    a = ap.parse_args()
    n = 1 << a.log2
    args = ["-z", "--interface", "pbnodev0", "--smac", pc.SMAC, "--dmac", pc.DMAC, "--dip", pc.DIP, "--sip",
            "10.20.0.0/16", "--protocol", "udp", "--udport", "27015", "--pmin", "22", "--pmax", "22", "--maxpckts",
            str(n), "--delay", "0", "--threads", "1", "--gpubatch", a.gpubatch, "--seed", "7"]
    path = os.path.join(a.dir, "pcap_e2e_%d.pcap" % os.getpid())
    dump, pcap = [], []
    for _ in range(a.reps):  # alternating
        dump.append(timed([BIN] + args + ["--pcapdump", path], path, n))
        pcap.append(timed([a.pcap_bin] + args + ["--pcap", path], path, n))
    d, p = statistics.median(dump), statistics.median(pcap)
    out = {"frames": n, "frame_len": 64, "file_bytes": 24 + 80 * n, "dir": a.dir, "reps": a.reps,
           "gpubatch": int(a.gpubatch), "pcapdump_s": [round(x, 3) for x in dump], "pcap_s": [round(x, 3) for x in pcap],
           "pcapdump_fps_median": round(n / d), "pcap_fps_median": round(n / p), "ratio": round(p / d, 2),
           "pcap_binary": a.pcap_label}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
