"""pbgpu_xlat46 against the read and write probes, and beside pbgpu_encap VXLAN, on the same buffers
(DESIGN.md 5.13).

For each config: build N = 2^LOG2 frames once, translate them into a buffer of the output's size,
warm up, translate REPS times (device_ms from the call's own HIP event pair: classify pass and
writer), then in the same process run pbgpu_read_probe_at over the source's frame bytes,
pbgpu_fill_probe_at over the output's bytes of the destination, pbgpu_encap VXLAN of the same source
into a buffer of its own with the fill probe over that buffer, and REPS more translations.  The
yardstick is read probe + the 4-KiB page fill (one workgroup per 4-KiB page, one 16-B store per lane:
the store shape of both kernels).  The classify pass's share is measured on the translated output:
every frame of it is `other`, so the call stops after the classify pass and reports that pass alone
(the same one lane per frame reading bytes 12..23, the records 20 B further apart).  The first and
last MiB of the output are compared with tests/pyxlat.py over the built frames before anything is timed.

    python3 scripts/xlat_bench.py [--out FILE.jsonl] [--log2 24] [--reps 10] [--configs a,b]
    python3 scripts/xlat_bench.py --pmc --configs c2_udp_64 --meta FILE.json
        (under `rocprofv3 --pmc ...`, no tracing flags: three translations and nothing else after
         the build; scripts/xlat_pmc.py runs it that way)

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
import pyxlat  # noqa: E402
import pbgpu  # noqa: E402
from pbgpu import ENCAP_VXLAN, EncapOpts, GpuContext, PbError, Sequence, XlatOpts, XlatResult  # noqa: E402

CONFIGS = ["c2_udp_64", "c4_tcp_syn", "c5_icmp_echo", "c2_udp_1500", "c3_udp_var"]
PAGE_FILL = "4KiB/wg 1 st/lane (8 wg/CU)"
WIN = 1 << 20
SRC_P, DST_P = pyxlat.prefix96("2001:db8:ffff:ffff:ffff:ffff::/96"), pyxlat.prefix96("64:ff9b::/96")
VX = dict(dst_mac=bytes.fromhex("0200000000a2"), src_mac=bytes.fromhex("0200000000a1"), src_ip=bytes([192, 0, 2, 1]),
          dst_ip=bytes([198, 51, 100, 2]), vni=0x123456)


def spot_check(fb, dst, n, nbytes):
    """The output's first and last WIN bytes against the definition over the frames there."""
    off = fb.offsets()
    for lo in (0, n - min(n, WIN // 62)):  # a window's worth of frames at either end
        hi = min(n, lo + WIN // 62)
        data = fb.stream(int(off[hi] - off[lo]), int(off[lo])).tobytes()
        ref = b"".join(pyxlat.xlat46(data[int(off[i] - off[lo]):int(off[i + 1] - off[lo])], SRC_P, DST_P, hash_flow=True)
                       for i in range(lo, hi))
        k = min(WIN, len(ref), nbytes)
        if lo == 0:
            assert dst.stream(k).tobytes() == ref[:k], "output start differs"
        else:
            assert dst.stream(k, nbytes - k).tobytes() == ref[-k:], "output end differs"


def run(ctx, name, n, reps, warmup, pmc):
    ctx.load_sequence(0, Sequence.from_config(pc.get(name)), pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n))
    dst = edst = None
    opts = XlatOpts.make(SRC_P, DST_P, hash_flow=True)
    eopts = EncapOpts.make(ENCAP_VXLAN, **VX)
    xl = lambda: float(fb.xlat46(dst, opts=opts).device_ms)
    try:
        ctx.build(0, 0, n, fb)
        ctx.sync()
        total = fb.total_bytes()
        nf, nbytes = ctx.xlat46_size(fb, 0, None, opts)
        dst = ctx.alloc_frames(nf, nbytes)
        base = {"config": name, "frames": n, "fixed_len": int(fb.f.fixed_len), "frame_bytes": total, "out_bytes": nbytes}
        if pmc:
            for _ in range(3):
                xl()
            return dict(base, xlats=3)
        for _ in range(warmup):
            xl()
        spot_check(fb, dst, n, nbytes)
        ms = [xl() for _ in range(reps)]
        src_extent, dst_extent = (total + 15) & ~15, (nbytes + 15) & ~15
        read_ms = min(ctx.read_probe_at(fb, src_extent, reps) for _ in range(2))
        fills = ctx.fill_probe_at(dst, dst_extent, reps)
        # pbgpu_encap VXLAN on the same source, its own yardstick measured the same way
        _, ebytes = ctx.encap_size(fb, 0, None, eopts)
        edst = ctx.alloc_frames(n, ebytes)
        for _ in range(warmup):
            fb.encap(edst, opts=eopts)
        ems = [fb.encap(edst, opts=eopts) for _ in range(2 * reps)]
        efills = ctx.fill_probe_at(edst, (ebytes + 15) & ~15, reps)
        edst.free()
        edst = None
        ms2 = [xl() for _ in range(reps)]  # and again after the probes
        spot_check(fb, dst, n, nbytes)
        # the classify pass alone: the output needs a destination with room, or -ENOSPC comes first
        edst = ctx.alloc_frames(n, nbytes + 20 * n)
        res = XlatResult()
        cms = []
        for _ in range(warmup + reps):
            try:
                dst.xlat46(edst, 0, n, opts, res=res)
                raise AssertionError("an IPv6 buffer was translated again")
            except PbError as e:
                assert e.code == -22 and int(res.n_other) == n, (e.code, int(res.n_other))
            cms.append(float(res.device_ms))
        cmed = statistics.median(cms[warmup:])
        med, emed = statistics.median(ms + ms2), statistics.median(ems)
        best = min(fills, key=fills.get)
        x_ratio = med / (read_ms + fills[PAGE_FILL])
        e_ratio = emed / (read_ms + efills[PAGE_FILL])
        return dict(base, **{
            "reps": 2 * reps,
            "xlat_ms_median": round(med, 4), "xlat_ms_min": round(min(ms + ms2), 4), "xlat_ms_max": round(max(ms + ms2), 4),
            "xlat_ms_median_before_probes": round(statistics.median(ms), 4),
            "xlat_ms_median_after_probes": round(statistics.median(ms2), 4),
            "xlat_gbps_read_plus_written": round((total + nbytes) / med / 1e6, 1),
            "classify_ms_median": round(cmed, 4), "classify_share": round(cmed / med, 3),
            "read_probe_ms": round(read_ms, 4), "read_probe_gbps": round(src_extent / read_ms / 1e6, 1),
            "page_fill_ms": round(fills[PAGE_FILL], 4), "page_fill_gbps": round(dst_extent / fills[PAGE_FILL] / 1e6, 1),
            "best_fill_shape": best, "best_fill_ms": round(fills[best], 4),
            "xlat_over_read_plus_page_fill": round(x_ratio, 3),
            "encap_vxlan_out_bytes": ebytes, "encap_vxlan_ms_median": round(emed, 4),
            "encap_vxlan_ms_min": round(min(ems), 4), "encap_vxlan_ms_max": round(max(ems), 4),
            "encap_vxlan_page_fill_ms": round(efills[PAGE_FILL], 4),
            "encap_vxlan_over_read_plus_page_fill": round(e_ratio, 3),
            "xlat_ratio_over_encap_ratio": round(x_ratio / e_ratio, 3),
        })
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
