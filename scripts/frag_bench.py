"""pbgpu_fragment against the read and write probes, and against pbgpu_encap, on the same buffers
(DESIGN.md 5.11).

For each config:mtu: build N = 2^LOG2 frames once (2^(LOG2 - 3) for the 9043-B config, so the output
stays in memory), fragment them into a buffer of pbgpu_fragment_size's size, warm up, fragment REPS
times (device_ms from the call's one HIP event pair: count, scan, map and writer, and the read-back
between them), then in the same process run pbgpu_read_probe_at over the source's frame bytes and
pbgpu_fill_probe_at over the output's bytes of the destination, and fragment REPS more times.  The
yardstick is read probe + the 4-KiB page fill (one workgroup per 4-KiB page, one 16-B store per
lane: the writer's store shape).  The count and scan stages' share is a host clock around
pbgpu_fragment_size (those stages and their read-back, ending in a synchronise) over a host clock
around pbgpu_fragment.  c2_udp_1500 is also encapsulated (VXLAN) in the same run: the nearest
existing kernel and its ratio to its own yardstick.  The first and last MiB of the output are
compared with tests/pyfrag.py over the built frames before anything is timed.

    python3 scripts/frag_bench.py [--out FILE.jsonl] [--log2 24] [--reps 10] [--configs a:1500,b:576]
    python3 scripts/frag_bench.py --pmc --configs c2_udp_1500:576 --meta FILE.json
        (under `rocprofv3 --pmc ...`, no tracing flags: three calls and nothing else after the
         build; scripts/frag_pmc.py runs it that way)

One JSON line per config on stdout and in --out.  Needs a GPU: there is no fallback."""
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
import pyfrag  # noqa: E402
from pbgpu import ENCAP_VXLAN, EncapOpts, GpuContext, Sequence  # noqa: E402

CONFIGS = ["udp_jumbo_fixed_odd:1500", "c2_udp_1500:576", "c3_udp_var:576", "c2_udp_64:1500"]
PAGE_FILL = "4KiB/wg 1 st/lane (8 wg/CU)"
WIN = 1 << 20
VX = dict(dst_mac=bytes.fromhex("0200000000a2"), src_mac=bytes.fromhex("0200000000a1"), src_ip=bytes([192, 0, 2, 1]),
          dst_ip=bytes([198, 51, 100, 2]), vni=0x123456)


def spot_check(fb, dst, n, nbytes, mtu):
    """The output's first and last WIN bytes against the definition over the frames there."""
    off = fb.offsets()
    longest = int((off[1:] - off[:-1]).max())
    k_frames = min(n, WIN // 18 if longest < 4096 else 2 + WIN // longest * 2)
    for lo in (0, n - k_frames):
        hi = lo + k_frames
        data = fb.stream(int(off[hi] - off[lo]), int(off[lo])).tobytes()
        frames = [data[int(off[i] - off[lo]):int(off[i + 1] - off[lo])] for i in range(lo, hi)]
        ref = b"".join(b"".join(pyfrag.fragment(f, mtu)) for f in frames)
        k = min(WIN, len(ref), nbytes)
        if lo == 0:
            assert dst.stream(k).tobytes() == ref[:k], "output start differs"
        else:
            assert dst.stream(k, nbytes - k).tobytes() == ref[-k:], "output end differs"


def host_ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def run(ctx, name, mtu, n, reps, warmup, pmc):
    ctx.load_sequence(0, Sequence.from_config(pc.get(name)), pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n))
    dst = edst = None
    try:
        ctx.build(0, 0, n, fb)
        ctx.sync()
        total = fb.total_bytes()
        nf, nbytes = ctx.fragment_size(fb, 0, None, mtu)
        dst = ctx.alloc_frames(nf, nbytes)
        base = {"config": name, "mtu": mtu, "frames": n, "fixed_len": int(fb.f.fixed_len), "frame_bytes": total,
                "out_frames": nf, "out_bytes": nbytes}
        if pmc:
            for _ in range(3):
                fb.fragment(dst, mtu=mtu)
            return dict(base, calls=3)
        for _ in range(warmup):
            res = fb.fragment(dst, mtu=mtu)
        assert (int(res.n_out), int(res.out_bytes)) == (nf, nbytes)
        spot_check(fb, dst, n, nbytes, mtu)
        ms = [fb.fragment(dst, mtu=mtu).device_ms for _ in range(reps)]
        src_extent, dst_extent = (total + 15) & ~15, (nbytes + 15) & ~15
        read_ms = min(ctx.read_probe_at(fb, src_extent, reps) for _ in range(2))
        fills = ctx.fill_probe_at(dst, dst_extent, reps)
        size_ms = statistics.median(host_ms(lambda: ctx.fragment_size(fb, 0, None, mtu)) for _ in range(reps))
        call_ms = statistics.median(host_ms(lambda: fb.fragment(dst, mtu=mtu)) for _ in range(reps))
        ms2 = [fb.fragment(dst, mtu=mtu).device_ms for _ in range(reps)]  # and again after the probes
        spot_check(fb, dst, n, nbytes, mtu)
        med = statistics.median(ms + ms2)
        best = min(fills, key=fills.get)
        out = dict(base, **{
            "reps": 2 * reps, "n_split": int(res.n_split),
            "frag_ms_median": round(med, 4), "frag_ms_min": round(min(ms + ms2), 4),
            "frag_ms_max": round(max(ms + ms2), 4),
            "frag_ms_median_before_probes": round(statistics.median(ms), 4),
            "frag_ms_median_after_probes": round(statistics.median(ms2), 4),
            "frag_gbps_read_plus_written": round((total + nbytes) / med / 1e6, 1),
            "read_probe_ms": round(read_ms, 4), "read_probe_gbps": round(src_extent / read_ms / 1e6, 1),
            "page_fill_ms": round(fills[PAGE_FILL], 4), "page_fill_gbps": round(dst_extent / fills[PAGE_FILL] / 1e6, 1),
            "best_fill_shape": best, "best_fill_ms": round(fills[best], 4),
            "frag_over_read_plus_page_fill": round(med / (read_ms + fills[PAGE_FILL]), 3),
            "fragment_size_host_ms_median": round(size_ms, 4), "fragment_host_ms_median": round(call_ms, 4),
            "count_scan_share_of_call_host_clock": round(size_ms / call_ms, 3),
        })
        if name == "c2_udp_1500":  # the nearest existing kernel on the same source
            opts = EncapOpts.make(ENCAP_VXLAN, **VX)
            ef, eb = ctx.encap_size(fb, 0, None, opts)
            edst = ctx.alloc_frames(ef, eb)
            for _ in range(warmup):
                fb.encap(edst, opts=opts)
            ems = [fb.encap(edst, opts=opts) for _ in range(2 * reps)]
            efills = ctx.fill_probe_at(edst, (eb + 15) & ~15, reps)
            emed = statistics.median(ems)
            out.update({"encap_vxlan_out_bytes": eb, "encap_ms_median": round(emed, 4), "encap_ms_min": round(min(ems), 4),
                        "encap_ms_max": round(max(ems), 4), "encap_page_fill_ms": round(efills[PAGE_FILL], 4),
                        "encap_over_read_plus_page_fill": round(emed / (read_ms + efills[PAGE_FILL]), 3)})
        return out
    finally:
        for b in (edst, dst, fb):
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
            name, mtu = item.split(":")
            log2 = a.log2 - 3 if name.startswith("udp_jumbo") else a.log2
            r = run(ctx, name, int(mtu), 1 << log2, a.reps, a.warmup, a.pmc)
            print(json.dumps(r), flush=True)
            lines.append(r)
    for path, text in ((a.out, "".join(json.dumps(r) + "\n" for r in lines)), (a.meta, json.dumps(lines))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
