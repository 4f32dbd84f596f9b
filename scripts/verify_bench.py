"""pbgpu_verify against the read probe on the same buffer.

For each config: build N = 2^LOG2 frames once, warm up, verify REPS times (device_ms from the
call's own HIP events), run pbgpu_read_probe_at over the same extent of the same buffer, and time
the build beside them.  The host method the verifier replaces (pbgpu_copy_packed +
pbo_verify_frames on 16 threads) is timed once on one 2^21-frame chunk; its per-N figure is that
chunk's time scaled by N / 2^21, not measured at N.

    python3 scripts/verify_bench.py [--out FILE.jsonl] [--log2 25] [--reps 20] [--configs a,b]
                                    [--lib OTHER/libpbgpu.so] [--no-host]
    python3 scripts/verify_bench.py --pmc --configs c2_udp_64 --meta FILE.json
        (under `rocprofv3 --pmc ... --output-format csv`, no tracing flags: three verifies and
         nothing else after the build; FILE.json gets the frame bytes scripts/verify_pmc.py needs)

One JSON line per config on stdout and in --out.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pb-af-xdp_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import pb_configs as pc  # noqa: E402
import pbgpu  # noqa: E402
from pbgpu import GpuContext, Sequence  # noqa: E402

CONFIGS = ["c2_udp_64", "c4_tcp_syn", "c5_icmp_echo", "c2_udp_1500", "c3_udp_var"]
HOST_CHUNK = 1 << 21


def cfg_mask(cfg):
    m = 0
    if cfg.get("ip", {}).get("csum", 1):
        m |= pbgpu.VERIFY_IP_CSUM | pbgpu.VERIFY_TOT_LEN
    if cfg.get("l4csum", 1):
        m |= pbgpu.VERIFY_L4_CSUM
    return m


def host_method(ctx, fb, n):
    """The parent's check of one chunk: device -> host copy, then the CPU checker on 16 threads."""
    import oracle_binding as ob

    n = min(n, HOST_CHUNK)
    flen = int(fb.f.fixed_len)
    off = None if flen else fb.offsets()[:n + 1]
    nbytes = n * flen if flen else int(off[n])
    buf = np.empty(nbytes, dtype=np.uint8)
    buf[:] = 0  # touch the pages first: the copy is timed, not the page faults
    t0 = time.perf_counter()
    assert ctx.lib.pbgpu_copy_packed(ctx.h, fb.ptr, buf.ctypes.data, 0, nbytes) == 0
    t1 = time.perf_counter()
    bad = ob.verify_frames(buf, off, flen, n, 16)
    t2 = time.perf_counter()
    assert bad == 0
    return {"frames": n, "bytes": nbytes, "copy_ms": (t1 - t0) * 1e3, "cpu_verify_ms": (t2 - t1) * 1e3}


def run(ctx, name, n, reps, warmup, pmc, host=True):
    cfg = pc.get(name)
    ctx.load_sequence(0, Sequence.from_config(cfg), pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n))
    try:
        ctx.build(0, 0, n, fb)
        ctx.sync()
        total = fb.total_bytes()
        mask = cfg_mask(cfg)
        if pmc:
            for _ in range(3):
                res = fb.verify(checks=mask)
                assert res.n_bad == 0 and res.n_checked == n
            return {"config": name, "frames": n, "bytes": total, "verifies": 3}
        ctx.kernel_time()
        build_ms = []
        for _ in range(5):
            ctx.build(0, 0, n, fb)
            ctx.sync()
            build_ms.append(ctx.kernel_time()[0])
        for _ in range(warmup):
            fb.verify(checks=mask)
        ms = []
        for _ in range(reps):
            res = fb.verify(checks=mask)
            assert res.n_bad == 0 and res.n_checked == n
            ms.append(res.device_ms)
        extent = (total + 15) & ~15
        probe = min(ctx.read_probe_at(fb, extent, reps) for _ in range(2))
        med = statistics.median(ms)
        out = {
            "config": name, "frames": n, "bytes": total, "checks": mask, "reps": reps,
            "verify_ms_median": round(med, 4), "verify_ms_min": round(min(ms), 4), "verify_ms_max": round(max(ms), 4),
            "verify_gbps": round(total / med / 1e6, 1),
            "read_probe_ms": round(probe, 4), "read_probe_gbps": round(extent / probe / 1e6, 1),
            "verify_over_probe": round(med / probe, 3),
            "build_ms_median": round(statistics.median(build_ms), 4),
        }
        if host:
            h = host_method(ctx, fb, n)
            out["host_method_chunk"] = {k: (round(v, 2) if isinstance(v, float) else v) for k, v in h.items()}
            out["host_method_ms_scaled_to_frames"] = round((h["copy_ms"] + h["cpu_verify_ms"]) * n / h["frames"], 1)
            out["host_method_scaled_from_frames"] = h["frames"]
        return out
    finally:
        fb.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--log2", type=int, default=25)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--meta")
    ap.add_argument("--lib", default=pbgpu.LIB_PATH, help="another build of libpbgpu.so (side-by-side A/B)")
    ap.add_argument("--no-host", action="store_true", help="skip the host method (copy + CPU checker)")
    a = ap.parse_args()
    lines = []
    with GpuContext(0, a.lib) as ctx:
        for name in a.configs.split(","):
            r = run(ctx, name, 1 << a.log2, a.reps, a.warmup, a.pmc, not a.no_host)
            print(json.dumps(r), flush=True)
            lines.append(r)
    for path, text in ((a.out, "".join(json.dumps(r) + "\n" for r in lines)), (a.meta, json.dumps(lines))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
