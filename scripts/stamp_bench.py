"""pbgpu_stamp against the read and write probes on the same buffer, against the bytes of the lines
it touches, and against the host method it replaces.

For each row config:position: build N = 2^LOG2 frames once, warm up, stamp REPS times (device_ms from
the call's own HIP event pair, the median reported), then in the same process: the host method on a
chunk of 2^21 frames (pbgpu_copy_packed down, scripts/stamp_host.c on 16 threads, an upload back up;
scaled to N), pbgpu_read_probe_at over the frames' bytes and last, because it overwrites them,
pbgpu_fill_probe_at over the same bytes (the 4-KiB page fill is the row's write yardstick).  The
bytes of the lines a stamp touches are counted from the frames' offsets: the 128-B lines under the
header dwords (frame bytes 9..27 at the widest), the checksum field, the byte at 46 of a TCP frame and
the 16 stamp bytes, once as loads and once more for the lines that are stored to.  Before anything is
timed the chunk stamped on the GPU is compared with the chunk stamped by stamp_host.c.

    python3 scripts/stamp_bench.py [--out FILE.jsonl] [--log2 24] [--reps 20] [--rows a:head,b:tail]
    python3 scripts/stamp_bench.py --pmc --rows c2_udp_64:head --meta FILE.json
        (under `rocprofv3 --pmc ...`, no tracing flags: three calls and nothing else after the
         build; scripts/stamp_pmc.py runs it that way)

One JSON line per row on stdout and in --out.  Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pb-af-xdp_amd"))

import pb_configs as pc  # noqa: E402
from pbgpu import GpuContext, Sequence  # noqa: E402

ROWS = ["c2_udp_64:head", "c4_tcp_syn:head", "c5_icmp_echo:head", "c2_udp_1500:head", "c3_udp_var:head",
        "c3_udp_var:tail"]
PAGE_FILL = "4KiB/wg 1 st/lane (8 wg/CU)"
HOST_CHUNK = 1 << 21
T0, STEP = 1_700_000_000_000_000_000, 6_720
LINE = 128


def host_lib():
    """scripts/stamp_host.c compiled into a temporary directory."""
    d = tempfile.mkdtemp(prefix="stamp_host_")
    so = os.path.join(d, "libstamp_host.so")
    subprocess.run(["gcc", "-O2", "-Wall", "-shared", "-fPIC", "-pthread", "-o", so,
                    os.path.join(ROOT, "scripts", "stamp_host.c")], check=True)
    lib = C.CDLL(so)
    lib.stamp_host.restype = C.c_int
    lib.stamp_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                               C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)]
    return lib


def touched_line_bytes(off, proto, tail):
    """Bytes of the distinct 128-B lines a stamp of these frames loads, and of those it stores to
    (frames that have room; head or tail at offset 0; TCP without options)."""
    o, L = off[:-1].astype(np.int64), (off[1:] - off[:-1]).astype(np.int64)
    H = 20 if proto == 6 else 8
    Q = {17: 40, 6: 50, 1: 36}[proto]
    S = np.where(tail, L - 16, 34 + H)
    fits = (S >= 34 + H) & (S + 16 <= L)
    spans = [((o + 12) & ~3, o + 28)]  # header dwords, every frame of 34 B or more
    if proto == 6:
        spans.append((o + 46, o + 47))
    wspans = [(np.where(fits, o + Q, 0), np.where(fits, o + Q + 2, 0)),
              (np.where(fits, (o + S) & ~3, 0), np.where(fits, o + S + 16, 0))]
    def union(spans_):  # a span is shorter than a line: its first and last line are all of them
        ids = np.concatenate([np.concatenate([(a // LINE)[b > a], ((b - 1) // LINE)[b > a]]) for a, b in spans_])
        return len(np.unique(ids)) * LINE

    return union(spans + wspans), union(wspans)


def host_method(ctx, lib, fb, n, tail):
    """One chunk through the host: copy down, the C stamp on 16 threads, copy up."""
    n = min(n, HOST_CHUNK)
    flen = int(fb.f.fixed_len)
    off = None if flen else fb.offsets()[:n + 1].copy()
    nbytes = n * flen if flen else int(off[n])
    t = time.perf_counter()
    data = fb.stream(nbytes)
    copy_ms = (time.perf_counter() - t) * 1e3
    counts = (C.c_uint64 * 3)()
    t = time.perf_counter()
    rc = lib.stamp_host(data.ctypes.data, None if flen else off.ctypes.data, flen, n, T0, STEP, 0, 0, 1 if tail else 0,
                        16, counts)
    cpu_ms = (time.perf_counter() - t) * 1e3
    assert rc == 0
    up = ctx.alloc_frames(n, max(16, (nbytes + 15) & ~15))
    try:
        t = time.perf_counter()
        up.upload(data, offsets=off, fixed_len=flen)
        up_ms = (time.perf_counter() - t) * 1e3
    finally:
        up.free()
    return {"frames": n, "bytes": nbytes, "copy_down_ms": copy_ms, "cpu_stamp_ms": cpu_ms, "copy_up_ms": up_ms,
            "stamped": int(counts[0])}, data


def run(ctx, lib, name, where, n, reps, warmup, pmc):
    tail = where == "tail"
    seq = Sequence.from_config(pc.get(name))
    ctx.load_sequence(0, seq, pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n))
    try:
        ctx.build(0, 0, n, fb)
        ctx.sync()
        total = fb.total_bytes()
        kw = dict(t0_ns=T0, step_ps=STEP, first_index=0, tail=tail)
        base = {"config": name, "position": where, "frames": n, "fixed_len": int(fb.f.fixed_len), "frame_bytes": total}
        if pmc:
            for _ in range(3):
                fb.stamp(**kw)
            return dict(base, calls=3)
        h, ref = host_method(ctx, lib, fb, n, tail)  # from the unstamped frames
        for _ in range(warmup):
            res = fb.stamp(**kw)
        assert np.array_equal(fb.stream(len(ref)), ref), "the GPU's chunk differs from stamp_host.c's"
        ms = [fb.stamp(**kw).device_ms for _ in range(reps)]
        extent = (total + 15) & ~15
        read_ms = min(ctx.read_probe_at(fb, extent, 10) for _ in range(2))
        off = fb.offsets()
        proto = {"udp": 17, "tcp": 6, "icmp": 1}[pc.get(name)["ip"]["protocol"]]
        loaded, stored = touched_line_bytes(off, proto, tail)
        del off
        fills = ctx.fill_probe_at(fb, extent, 10)  # last: it overwrites the frames
        med = statistics.median(ms)
        host_ms = (h["copy_down_ms"] + h["cpu_stamp_ms"] + h["copy_up_ms"]) * n / h["frames"]
        return dict(base, **{
            "reps": reps, "n_stamped": int(res.n_stamped), "n_short": int(res.n_short), "n_other": int(res.n_other),
            "stamp_ms_median": round(med, 4), "stamp_ms_min": round(min(ms), 4), "stamp_ms_max": round(max(ms), 4),
            "stamp_mfps": round(n / med / 1e3, 1),
            "read_probe_ms": round(read_ms, 4), "read_probe_gbps": round(extent / read_ms / 1e6, 1),
            "page_fill_ms": round(fills[PAGE_FILL], 4), "page_fill_gbps": round(extent / fills[PAGE_FILL] / 1e6, 1),
            "stamp_over_read_plus_page_fill": round(med / (read_ms + fills[PAGE_FILL]), 3),
            "stamp_over_read_probe": round(med / read_ms, 3),
            "line_bytes_loaded": loaded, "line_bytes_stored": stored,
            "line_gbps": round((loaded + stored) / med / 1e6, 1),
            "line_share_of_buffer": round(loaded / extent, 4),
            "host_method_chunk": {k: (round(v, 2) if isinstance(v, float) else v) for k, v in h.items()},
            "host_method_ms_scaled_to_frames": round(host_ms, 1),
            "host_method_over_stamp": round(host_ms / med, 1),
        })
    finally:
        fb.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--log2", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--meta")
    a = ap.parse_args()
    lib = None if a.pmc else host_lib()
    lines = []
    with GpuContext(0) as ctx:
        for item in a.rows.split(","):
            name, where = item.split(":")
            r = run(ctx, lib, name, where, 1 << a.log2, a.reps, a.warmup, a.pmc)
            print(json.dumps(r), flush=True)
            lines.append(r)
            if a.out:  # row by row: a later row's failure keeps the earlier ones
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    f.write("".join(json.dumps(x) + "\n" for x in lines))
    if a.meta:
        os.makedirs(os.path.dirname(os.path.abspath(a.meta)), exist_ok=True)
        with open(a.meta, "w") as f:
            f.write(json.dumps(lines))


if __name__ == "__main__":
    main()
