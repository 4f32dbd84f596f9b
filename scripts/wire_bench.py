"""pbgpu_verify_wire against the read probe, beside pbgpu_verify, on the same buffers in one process
(DESIGN.md 5.14).

For each row: build N = 2^LOG2 frames (2^21 for the 9043-B source), repack them as the row says,
warm up, call pbgpu_verify_wire REPS times (device_ms from the call's own event pair), run
pbgpu_read_probe_at over the same extent of the same buffer and, where the buffer is one that
pbgpu_verify parses (plain frames), pbgpu_verify with PBGPU_VERIFY_ALL the same way.

    python3 scripts/wire_bench.py [--out profiles/wire/wire_bench.jsonl] [--log2 24] [--reps 20] [--rows a,b]
    python3 scripts/wire_bench.py --pmc --rows c2_udp_64 --meta FILE.json
        (under `rocprofv3 --pmc ...`, no tracing flags: three calls and nothing else after the
         build and repack; FILE.json gets the frame bytes scripts/wire_pmc.py needs)

One JSON line per row on stdout and in --out.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pb-af-xdp_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import pb_configs as pc  # noqa: E402
import pbgpu  # noqa: E402
from pbgpu import ENCAP_VLAN, ENCAP_VXLAN, GpuContext, Sequence, XlatOpts  # noqa: E402

VX = dict(dst_mac=bytes.fromhex("0200000000a2"), src_mac=bytes.fromhex("0200000000a1"), src_ip=bytes([192, 0, 2, 1]),
          dst_ip=bytes([198, 51, 100, 2]), vni=0x123456)
PREFIX = bytes.fromhex("0064ff9b") + bytes(8)
# row: (config, repack)
ROWS = {name: (name, None) for name in ("c2_udp_64", "c4_tcp_syn", "c5_icmp_echo", "c2_udp_1500", "c3_udp_var")}
for _name in ("c2_udp_64", "c2_udp_1500"):
    for _rp in ("vxlan", "vlan", "xlat6"):
        ROWS[_name + "+" + _rp] = (_name, _rp)
ROWS["udp_jumbo_fixed_odd+fragment1500"] = ("udp_jumbo_fixed_odd", "fragment")


def repacked(ctx, fb, n, how):
    """The buffer to check and the VXLAN port to give; fb itself for a plain row."""
    if how is None:
        return fb, 0
    mf, mb = int(fb.f.capacity_frames), int(fb.f.capacity_bytes)
    if how == "fragment":
        frames, nbytes = ctx.fragment_size(fb, 0, None, 1500)
        dst = ctx.alloc_frames(frames, nbytes + 64)
        fb.fragment(dst, mtu=1500)
        return dst, 0
    dst = ctx.alloc_frames(mf, mb + 64 * mf)
    if how == "vxlan":
        fb.encap(dst, mode=ENCAP_VXLAN, **VX)
        return dst, 4789
    if how == "vlan":
        fb.encap(dst, mode=ENCAP_VLAN, tci=100)
    else:
        fb.xlat46(dst, opts=XlatOpts.make(PREFIX))
    return dst, 0


def run(ctx, row, log2, reps, warmup, pmc):
    name, how = ROWS[row]
    n = 1 << (min(log2, 21) if name == "udp_jumbo_fixed_odd" else log2)
    ctx.load_sequence(0, Sequence.from_config(pc.get(name)), pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n))
    buf = None
    try:
        ctx.build(0, 0, n, fb)
        ctx.sync()
        buf, port = repacked(ctx, fb, n, how)
        if buf is not fb:  # the source is not needed any more
            fb.free()
            fb = None
        nf, total = int(buf.f.n_frames), buf.total_bytes()
        if pmc:
            for _ in range(3):
                res = buf.verify_wire(vxlan_port=port)
                assert res.n_bad == 0 and res.n_checked == nf
            return {"row": row, "frames": nf, "bytes": total, "calls": 3}
        for _ in range(warmup):
            buf.verify_wire(vxlan_port=port)
        ms = []
        for _ in range(reps):
            res = buf.verify_wire(vxlan_port=port)
            assert res.n_bad == 0 and res.n_checked == nf
            ms.append(res.device_ms)
        extent = (total + 15) & ~15
        probe = min(ctx.read_probe_at(buf, extent, reps) for _ in range(2))
        med = statistics.median(ms)
        out = {
            "row": row, "frames": nf, "bytes": total, "reps": reps, "vxlan_port": port,
            "n_ipv4": int(res.n_ipv4), "n_ipv6": int(res.n_ipv6), "n_inner": int(res.n_inner), "n_nol4": int(res.n_nol4),
            "wire_ms_median": round(med, 4), "wire_ms_min": round(min(ms), 4), "wire_ms_max": round(max(ms), 4),
            "wire_gbps": round(total / med / 1e6, 1),
            "read_probe_ms": round(probe, 4), "read_probe_gbps": round(extent / probe / 1e6, 1),
            "wire_over_probe": round(med / probe, 3),
        }
        if how is None:  # a buffer pbgpu_verify parses
            for _ in range(warmup):
                buf.verify(checks=pbgpu.VERIFY_ALL)
            vms = []
            for _ in range(reps):
                v = buf.verify(checks=pbgpu.VERIFY_ALL)
                assert v.n_bad == 0 and v.n_checked == nf
                vms.append(v.device_ms)
            vmed = statistics.median(vms)
            out.update(verify_ms_median=round(vmed, 4), verify_over_probe=round(vmed / probe, 3),
                       wire_over_verify=round(med / vmed, 3))
        return out
    finally:
        if buf is not None and buf is not fb:
            buf.free()
        if fb is not None:
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
    ap.add_argument("--lib", default=pbgpu.LIB_PATH, help="another build of libpbgpu.so (side-by-side A/B)")
    a = ap.parse_args()
    lines = []
    with GpuContext(0, a.lib) as ctx:
        for row in a.rows.split(","):
            r = run(ctx, row, a.log2, a.reps, a.warmup, a.pmc)
            print(json.dumps(r), flush=True)
            lines.append(r)
    for path, text in ((a.out, "".join(json.dumps(r) + "\n" for r in lines)), (a.meta, json.dumps(lines))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
