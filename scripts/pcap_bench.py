"""pbgpu_pcap_pack against the read and write probes on the same buffers.

For each config: build N = 2^LOG2 frames once, pack them into a stream buffer of the stream's size,
warm up, pack REPS times (device_ms from the call's own HIP events), then in the same process run
pbgpu_read_probe_at over the source's frame bytes and pbgpu_fill_probe_at over the stream's bytes
of the destination buffer.  The yardstick is read probe + the 4-KiB page fill (one workgroup per
4-KiB page, one 16-B store per lane: the pack's own store shape); the fastest fill shape is kept
beside it.  The first and last MiB of the stream are compared with the stream definition in plain
Python over the built frames, so a wrong pack is not timed.

    python3 scripts/pcap_bench.py [--out FILE.jsonl] [--log2 24] [--reps 10] [--configs a,b]
    python3 scripts/pcap_bench.py --pmc --configs c2_udp_64 --meta FILE.json
        (under `rocprofv3 --pmc ... --output-format csv`, no tracing flags: three packs and nothing
         else after the build; FILE.json gets the stream bytes scripts/pcap_pmc.py needs)

One JSON line per config on stdout and in --out.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pb-af-xdp_amd"))

import pb_configs as pc  # noqa: E402
import pbgpu  # noqa: E402
from pbgpu import GpuContext, Sequence  # noqa: E402

CONFIGS = ["c2_udp_64", "c4_tcp_syn", "c2_udp_1500", "c3_udp_var"]
PAGE_FILL = "4KiB/wg 1 st/lane (8 wg/CU)"
T0, STEP = 1_700_000_000_000_000_000, 6_720  # 148.8 Mpps: 64-B line rate of 100 GbE
WIN = 1 << 20


def reference(frames, first_index, header):
    """The stream definition (include/pbgpu.h), microsecond resolution."""
    out = [struct.pack("<6I", 0xA1B2C3D4, 0x00040002, 0, 0, 65535, 1)] if header else []
    for j, f in enumerate(frames):
        t = T0 + ((first_index + j) * STEP) // 1000
        out.append(struct.pack("<4I", (t // 10**9) % 2**32, (t % 10**9) // 1000, len(f), len(f)))
        out.append(f)
    return b"".join(out)


def spot_check(fb, dst, n, nbytes):
    """The stream's first and last WIN bytes against the definition over the frames there."""
    off = fb.offsets()
    for lo in (0, n - min(n, WIN // 16)):  # a window's worth of frames at either end
        hi = min(n, lo + WIN // 16)
        data = fb.stream(int(off[hi] - off[lo]), int(off[lo])).tobytes()
        frames = [data[int(off[i] - off[lo]):int(off[i + 1] - off[lo])] for i in range(lo, hi)]
        ref = reference(frames, lo, lo == 0)
        if lo == 0:
            got = dst.stream(min(WIN, len(ref), nbytes)).tobytes()
            assert got == ref[:len(got)], "stream start differs"
        else:
            k = min(WIN, len(ref))
            assert dst.stream(k, nbytes - k).tobytes() == ref[-k:], "stream end differs"


def run(ctx, name, n, reps, warmup, pmc):
    ctx.load_sequence(0, Sequence.from_config(pc.get(name)), pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n))
    dst = None
    try:
        ctx.build(0, 0, n, fb)
        ctx.sync()
        total = fb.total_bytes()
        nbytes = ctx.pcap_size(fb)
        dst = ctx.alloc_frames(1, nbytes)
        if pmc:
            for _ in range(3):
                assert fb.pcap_pack(dst, t0_ns=T0, step_ps=STEP)[0] == nbytes
            return {"config": name, "frames": n, "frame_bytes": total, "stream_bytes": nbytes, "packs": 3}
        for _ in range(warmup):
            fb.pcap_pack(dst, t0_ns=T0, step_ps=STEP)
        spot_check(fb, dst, n, nbytes)
        ms = [fb.pcap_pack(dst, t0_ns=T0, step_ps=STEP)[1] for _ in range(reps)]
        src_extent, dst_extent = (total + 15) & ~15, (nbytes + 15) & ~15
        read_ms = min(ctx.read_probe_at(fb, src_extent, reps) for _ in range(2))
        fills = ctx.fill_probe_at(dst, dst_extent, reps)
        ms2 = [fb.pcap_pack(dst, t0_ns=T0, step_ps=STEP)[1] for _ in range(reps)]  # and again after the probes
        spot_check(fb, dst, n, nbytes)
        med = statistics.median(ms + ms2)
        best = min(fills, key=fills.get)
        return {
            "config": name, "frames": n, "fixed_len": int(fb.f.fixed_len), "frame_bytes": total,
            "stream_bytes": nbytes, "reps": 2 * reps,
            "pack_ms_median": round(med, 4), "pack_ms_min": round(min(ms + ms2), 4),
            "pack_ms_max": round(max(ms + ms2), 4),
            "pack_ms_median_before_probes": round(statistics.median(ms), 4),
            "pack_ms_median_after_probes": round(statistics.median(ms2), 4),
            "pack_gbps_read_plus_written": round((total + nbytes) / med / 1e6, 1),
            "pack_gfps": round(n / med / 1e6, 2),
            "read_probe_ms": round(read_ms, 4), "read_probe_gbps": round(src_extent / read_ms / 1e6, 1),
            "page_fill_ms": round(fills[PAGE_FILL], 4), "page_fill_gbps": round(dst_extent / fills[PAGE_FILL] / 1e6, 1),
            "best_fill_shape": best, "best_fill_ms": round(fills[best], 4),
            "pack_over_read_plus_page_fill": round(med / (read_ms + fills[PAGE_FILL]), 3),
        }
    finally:
        if dst is not None:
            dst.free()
        fb.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--log2", type=int, default=24)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--meta")
    ap.add_argument("--lib", default=pbgpu.LIB_PATH, help="another build of libpbgpu.so (side-by-side A/B)")
    a = ap.parse_args()
    lines = []
    with GpuContext(0, a.lib) as ctx:
        for name in a.configs.split(","):
            r = run(ctx, name, 1 << a.log2, a.reps, a.warmup, a.pmc)
            print(json.dumps(r), flush=True)
            lines.append(r)
    for path, text in ((a.out, "".join(json.dumps(r) + "\n" for r in lines)), (a.meta, json.dumps(lines))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
