"""pbgpu_segment against the read and write probes, and against pbgpu_fragment at the MTU that gives
the same cut, on the same buffers.

For each config:mss[:nocsum]: build N = 2^LOG2 frames once (2^(LOG2 - 3) for the 9-KB configs, so the
output stays in memory), segment them into a buffer of pbgpu_segment_size's size, warm up, segment
REPS times (device_ms from the call's one HIP event pair: count, scans, map, sums and writer, and
the read-back between them), then in the same process run pbgpu_read_probe_at over the source's
frame bytes and pbgpu_fill_probe_at over the output's bytes of the destination, and segment REPS
more times.  The floor is read probe + the 4-KiB page fill (one read of the source, one write of the
output).  The yardstick is pbgpu_fragment on the same source at mtu = 20 + H + mss: the same writer
shape without the sums.  The count and scans' share is a host clock around pbgpu_segment_size over a
host clock around pbgpu_segment; the sum pass's share is what the same call under NO_L4_CSUM, which
skips exactly that pass, takes less.  The first and last MiB of the output are compared with
tests/pyseg.py over the built frames before anything is timed.

    python3 scripts/seg_bench.py [--out FILE.jsonl] [--log2 24] [--reps 10] [--configs a:1472,b:536:nocsum]
    python3 scripts/seg_bench.py --pmc --configs c2_udp_1500:536 --meta FILE.json
        (under `rocprofv3 --pmc ...`, no tracing flags: three calls and nothing else after the
         build; scripts/seg_pmc.py runs it that way)

One JSON line per row on stdout and in --out.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pb-af-xdp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pb_configs as pc  # noqa: E402
import pyseg  # noqa: E402
from pbgpu import GpuContext, Sequence  # noqa: E402

CONFIGS = ["udp_jumbo_fixed_odd:1472", "tcp_jumbo_fixed_odd:1460", "c2_udp_1500:536", "c3_udp_var:536", "c2_udp_64:1460",
           "udp_jumbo_fixed_odd:1472:nocsum"]
PAGE_FILL = "4KiB/wg 1 st/lane (8 wg/CU)"
WIN = 1 << 20


def config(name):
    if name == "tcp_jumbo_fixed_odd":  # TCP, 9001-B payloads: 9055-B frames
        c = pc.c4_tcp_syn()
        c["tcp"] = {"sport": 0, "dport": 80, "ack": 1, "psh": 1}
        c["payloads"] = [{"length": {"min": 9001, "max": 9001}}]
        return c
    return pc.get(name)


def spot_check(fb, dst, n, nbytes, mss, flags):
    """The output's first and last WIN bytes against the definition over the frames there."""
    off = fb.offsets()
    longest = int((off[1:] - off[:-1]).max())
    k_frames = min(n, WIN // 18 if longest < 4096 else 2 + WIN // longest * 2)
    for lo in (0, n - k_frames):
        hi = lo + k_frames
        data = fb.stream(int(off[hi] - off[lo]), int(off[lo])).tobytes()
        frames = [data[int(off[i] - off[lo]):int(off[i + 1] - off[lo])] for i in range(lo, hi)]
        ref = b"".join(b"".join(pyseg.segment(f, mss, flags)) for f in frames)
        k = min(WIN, len(ref), nbytes)
        if lo == 0:
            assert dst.stream(k).tobytes() == ref[:k], "output start differs"
        else:
            assert dst.stream(k, nbytes - k).tobytes() == ref[-k:], "output end differs"


def host_ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def run(ctx, name, mss, nocsum, n, reps, warmup, pmc):
    cfg = config(name)
    ctx.load_sequence(0, Sequence.from_config(cfg), pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n))
    dst = fdst = None
    try:
        ctx.build(0, 0, n, fb)
        ctx.sync()
        total = fb.total_bytes()
        nf, nbytes = ctx.segment_size(fb, 0, None, mss, nocsum)
        dst = ctx.alloc_frames(nf, nbytes)
        base = {"config": name, "mss": mss, "no_l4_csum": nocsum, "frames": n, "fixed_len": int(fb.f.fixed_len),
                "frame_bytes": total, "out_frames": nf, "out_bytes": nbytes}
        if pmc:
            for _ in range(3):
                fb.segment(dst, mss=mss, no_l4_csum=nocsum)
            return dict(base, calls=3)
        for _ in range(warmup):
            res = fb.segment(dst, mss=mss, no_l4_csum=nocsum)
        assert (int(res.n_out), int(res.out_bytes)) == (nf, nbytes)
        spot_check(fb, dst, n, nbytes, mss, 1 if nocsum else 0)
        ms = [fb.segment(dst, mss=mss, no_l4_csum=nocsum).device_ms for _ in range(reps)]
        src_extent, dst_extent = (total + 15) & ~15, (nbytes + 15) & ~15
        read_ms = min(ctx.read_probe_at(fb, src_extent, reps) for _ in range(2))
        fills = ctx.fill_probe_at(dst, dst_extent, reps)
        size_ms = statistics.median(host_ms(lambda: ctx.segment_size(fb, 0, None, mss, nocsum)) for _ in range(reps))
        call_ms = statistics.median(host_ms(lambda: fb.segment(dst, mss=mss, no_l4_csum=nocsum)) for _ in range(reps))
        nosum = [fb.segment(dst, mss=mss, no_l4_csum=True).device_ms for _ in range(reps)]  # the call without the sum pass
        ms2 = [fb.segment(dst, mss=mss, no_l4_csum=nocsum).device_ms for _ in range(reps)]  # and again after the probes
        spot_check(fb, dst, n, nbytes, mss, 1 if nocsum else 0)
        med = statistics.median(ms + ms2)
        floor = read_ms + fills[PAGE_FILL]
        out = dict(base, **{
            "reps": 2 * reps, "n_split": int(res.n_split_tcp) + int(res.n_split_udp),
            "seg_ms_median": round(med, 4), "seg_ms_min": round(min(ms + ms2), 4), "seg_ms_max": round(max(ms + ms2), 4),
            "seg_ms_median_before_probes": round(statistics.median(ms), 4),
            "seg_ms_median_after_probes": round(statistics.median(ms2), 4),
            "seg_gbps_read_plus_written": round((total + nbytes) / med / 1e6, 1),
            "read_probe_ms": round(read_ms, 4), "read_probe_gbps": round(src_extent / read_ms / 1e6, 1),
            "page_fill_ms": round(fills[PAGE_FILL], 4), "page_fill_gbps": round(dst_extent / fills[PAGE_FILL] / 1e6, 1),
            "seg_over_read_plus_page_fill": round(med / floor, 3),
            "segment_size_host_ms_median": round(size_ms, 4), "segment_host_ms_median": round(call_ms, 4),
            "count_scan_share_of_call_host_clock": round(size_ms / call_ms, 3),
            "seg_no_l4_csum_ms_median": round(statistics.median(nosum), 4),
            "sum_pass_share_of_call": round(max(0.0, med - statistics.median(nosum)) / med, 3),
        })
        # the yardstick: the fragmenter on the same source at the MTU that gives the same cut
        proto = cfg["ip"]["protocol"]
        mtu = 20 + (20 if proto == "tcp" else 8) + mss
        ff, fbytes = ctx.fragment_size(fb, 0, None, mtu)
        fdst = ctx.alloc_frames(ff, fbytes)
        for _ in range(warmup):
            fb.fragment(fdst, mtu=mtu)
        fms = [fb.fragment(fdst, mtu=mtu).device_ms for _ in range(2 * reps)]
        ffills = ctx.fill_probe_at(fdst, (fbytes + 15) & ~15, reps)
        fmed = statistics.median(fms)
        out.update({"frag_mtu": mtu, "frag_out_frames": ff, "frag_out_bytes": fbytes, "frag_ms_median": round(fmed, 4),
                    "frag_ms_min": round(min(fms), 4), "frag_ms_max": round(max(fms), 4),
                    "frag_page_fill_ms": round(ffills[PAGE_FILL], 4),
                    "frag_over_read_plus_page_fill": round(fmed / (read_ms + ffills[PAGE_FILL]), 3),
                    "seg_over_frag": round(med / fmed, 3)})
        return out
    finally:
        for b in (fdst, dst, fb):
            if b is not None:
                b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--log2", type=int, default=24)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--meta")
    a = ap.parse_args()
    lines = []
    with GpuContext(0) as ctx:
        for item in a.configs.split(","):
            parts = item.split(":")
            name, mss, nocsum = parts[0], int(parts[1]), parts[2:] == ["nocsum"]
            log2 = a.log2 - 3 if "jumbo" in name else a.log2
            r = run(ctx, name, mss, nocsum, 1 << log2, a.reps, a.warmup, a.pmc)
            print(json.dumps(r), flush=True)
            lines.append(r)
    for path, text in ((a.out, "".join(json.dumps(r) + "\n" for r in lines)), (a.meta, json.dumps(lines))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
