"""pbgpu_encap against the read and write probes, and against pbgpu_pcap_pack, on the same buffers
(DESIGN.md 5.10).

For each config:mode: build N = 2^LOG2 frames once, encapsulate them into a buffer of the output's
size, warm up, encapsulate REPS times (device_ms from the call's own HIP events), then in the same
process run pbgpu_read_probe_at over the source's frame bytes, pbgpu_fill_probe_at over the output's
bytes of the destination, pbgpu_pcap_pack of the same source into a stream buffer with the fill probe
over that buffer, and REPS more encapsulations.  The yardstick is read probe + the 4-KiB page fill
(one workgroup per 4-KiB page, one 16-B store per lane: the store shape of both kernels).  The first
and last MiB of the output are compared with tests/pyencap.py over the built frames before anything
is timed.

    python3 scripts/encap_bench.py [--out FILE.jsonl] [--log2 24] [--reps 10] [--configs a:vxlan,b:vlan]
    python3 scripts/encap_bench.py --pmc --configs c2_udp_64:vxlan --meta FILE.json
        (under `rocprofv3 --pmc ...`, no tracing flags: three encapsulations and nothing else after
         the build; scripts/encap_pmc.py runs it that way)

One JSON line per config on stdout and in --out.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pb-af-xdp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pb_configs as pc  # noqa: E402
import pyencap  # noqa: E402
import pbgpu  # noqa: E402
from pbgpu import ENCAP_VLAN, ENCAP_VXLAN, EncapOpts, GpuContext, Sequence  # noqa: E402

CONFIGS = ["c2_udp_64:vxlan", "c4_tcp_syn:vxlan", "c2_udp_1500:vxlan", "c3_udp_var:vxlan", "c2_udp_64:vlan"]
PAGE_FILL = "4KiB/wg 1 st/lane (8 wg/CU)"
T0, STEP = 1_700_000_000_000_000_000, 6_720
WIN = 1 << 20
VX = dict(dst_mac=bytes.fromhex("0200000000a2"), src_mac=bytes.fromhex("0200000000a1"), src_ip=bytes([192, 0, 2, 1]),
          dst_ip=bytes([198, 51, 100, 2]), vni=0x123456)
TCI = 0xA064


def opts_of(mode):
    return EncapOpts.make(ENCAP_VXLAN, **VX) if mode == "vxlan" else EncapOpts.make(ENCAP_VLAN, tci=TCI)


def reference(frames, mode):
    return b"".join(pyencap.vxlan(f, **VX) if mode == "vxlan" else pyencap.vlan(f, TCI) for f in frames)


def spot_check(fb, dst, n, nbytes, mode):
    """The output's first and last WIN bytes against the definition over the frames there."""
    off = fb.offsets()
    for lo in (0, n - min(n, WIN // 18)):  # a window's worth of frames at either end
        hi = min(n, lo + WIN // 18)
        data = fb.stream(int(off[hi] - off[lo]), int(off[lo])).tobytes()
        ref = reference([data[int(off[i] - off[lo]):int(off[i + 1] - off[lo])] for i in range(lo, hi)], mode)
        k = min(WIN, len(ref), nbytes)
        if lo == 0:
            assert dst.stream(k).tobytes() == ref[:k], "output start differs"
        else:
            assert dst.stream(k, nbytes - k).tobytes() == ref[-k:], "output end differs"


def run(ctx, name, mode, n, reps, warmup, pmc):
    ctx.load_sequence(0, Sequence.from_config(pc.get(name)), pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n))
    dst = pdst = None
    opts = opts_of(mode)
    try:
        ctx.build(0, 0, n, fb)
        ctx.sync()
        total = fb.total_bytes()
        nf, nbytes = ctx.encap_size(fb, 0, None, opts)
        dst = ctx.alloc_frames(nf, nbytes)
        base = {"config": name, "mode": mode, "frames": n, "fixed_len": int(fb.f.fixed_len), "frame_bytes": total,
                "out_bytes": nbytes}
        if pmc:
            for _ in range(3):
                fb.encap(dst, opts=opts)
            return dict(base, encaps=3)
        for _ in range(warmup):
            fb.encap(dst, opts=opts)
        spot_check(fb, dst, n, nbytes, mode)
        ms = [fb.encap(dst, opts=opts) for _ in range(reps)]
        src_extent, dst_extent = (total + 15) & ~15, (nbytes + 15) & ~15
        read_ms = min(ctx.read_probe_at(fb, src_extent, reps) for _ in range(2))
        fills = ctx.fill_probe_at(dst, dst_extent, reps)
        # the pcap packer on the same source, its own yardstick measured the same way
        pbytes = ctx.pcap_size(fb)
        pdst = ctx.alloc_frames(1, pbytes)
        for _ in range(warmup):
            fb.pcap_pack(pdst, t0_ns=T0, step_ps=STEP)
        pms = [fb.pcap_pack(pdst, t0_ns=T0, step_ps=STEP)[1] for _ in range(reps)]
        pfills = ctx.fill_probe_at(pdst, (pbytes + 15) & ~15, reps)
        ms2 = [fb.encap(dst, opts=opts) for _ in range(reps)]  # and again after the probes
        spot_check(fb, dst, n, nbytes, mode)
        med, pmed = statistics.median(ms + ms2), statistics.median(pms)
        best = min(fills, key=fills.get)
        return dict(base, **{
            "reps": 2 * reps,
            "encap_ms_median": round(med, 4), "encap_ms_min": round(min(ms + ms2), 4),
            "encap_ms_max": round(max(ms + ms2), 4),
            "encap_ms_median_before_probes": round(statistics.median(ms), 4),
            "encap_ms_median_after_probes": round(statistics.median(ms2), 4),
            "encap_gbps_read_plus_written": round((total + nbytes) / med / 1e6, 1),
            "read_probe_ms": round(read_ms, 4), "read_probe_gbps": round(src_extent / read_ms / 1e6, 1),
            "page_fill_ms": round(fills[PAGE_FILL], 4), "page_fill_gbps": round(dst_extent / fills[PAGE_FILL] / 1e6, 1),
            "best_fill_shape": best, "best_fill_ms": round(fills[best], 4),
            "encap_over_read_plus_page_fill": round(med / (read_ms + fills[PAGE_FILL]), 3),
            "pcap_stream_bytes": pbytes, "pcap_pack_ms_median": round(pmed, 4),
            "pcap_pack_ms_min": round(min(pms), 4), "pcap_pack_ms_max": round(max(pms), 4),
            "pcap_page_fill_ms": round(pfills[PAGE_FILL], 4),
            "pcap_pack_over_read_plus_page_fill": round(pmed / (read_ms + pfills[PAGE_FILL]), 3),
        })
    finally:
        for b in (pdst, dst, fb):
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
    ap.add_argument("--lib", default=pbgpu.LIB_PATH, help="another build of libpbgpu.so (side-by-side A/B)")
    a = ap.parse_args()
    lines = []
    with GpuContext(0, a.lib) as ctx:
        for item in a.configs.split(","):
            name, mode = item.split(":")
            r = run(ctx, name, mode, 1 << a.log2, a.reps, a.warmup, a.pmc)
            print(json.dumps(r), flush=True)
            lines.append(r)
    for path, text in ((a.out, "".join(json.dumps(r) + "\n" for r in lines)), (a.meta, json.dumps(lines))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
