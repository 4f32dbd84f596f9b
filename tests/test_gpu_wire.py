"""pbgpu_verify_wire on the GPU against tests/pywire.py: every case compares the whole codes array
and every result field, checks that the variant without codes agrees and that the buffer's bytes
are what was put there.  Frames come from tests/wire_frames.py (clean by class), from byte mutants
of them, and from the library's own pipelines."""
import ctypes as C

import numpy as np
import pytest

import pb_configs as pc
import pbgpu
import pywire as pw
import verify_ref as vr
import wire_frames as wf
from pbgpu import ENCAP_VLAN, ENCAP_VXLAN, GpuContext, Sequence, WireOpts, WireResult, XlatOpts

pytestmark = pytest.mark.gpu
NONE = pbgpu.NO_BAD_FRAME
PORT = wf.VXLAN_PORT
EINVAL = -22
K = vr.shape_constants()
STAGE, BF_MAX, WT = K["PB_VS_STAGE"], K["PB_VS_BF_MAX"], K["PB_VST_WT"]
VX = dict(dst_mac=bytes.fromhex("0200000000a2"), src_mac=bytes.fromhex("0200000000a1"), src_ip=bytes([192, 0, 2, 1]),
          dst_ip=bytes([198, 51, 100, 2]), vni=0x123456)
PREFIX = bytes.fromhex("0064ff9b") + bytes(8)


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def wire_shape(fixed_len, n, mean=None):
    """pbgpu_verify_wire's launch: pb_vst_kernel's sizing (the second half of vr.verify_shape) at every length."""
    mean = fixed_len or mean
    G = 8 if mean <= 192 else (16 if mean <= 768 else (32 if mean <= 3072 else 64))
    ng = WT // G
    bf = min(max((STAGE - 16 if fixed_len else STAGE * 3 // 4) // max(mean, 1) // ng * ng, ng), BF_MAX)
    nw = min(max(n // (bf * 16384), 1), 64)
    return {"G": G, "bf": bf, "nw": nw, "wgf": bf * nw, "grid": (n + bf * nw - 1) // (bf * nw)}


def reference(frames, port=PORT):
    """(codes under WIRE_ALL, 4 / 6 / 0 per frame) as arrays."""
    w = [pw.walk(f, pw.ALL, port) for f in frames]
    return np.array([c for c, _ in w], dtype=np.uint8), np.array([k for _, k in w], dtype=np.uint8)


def expect(res, codes, ref, l3, first=0):
    """A WireResult and its codes against the reference's codes and L3 kinds of the same range."""
    assert np.array_equal(codes, ref), [(int(i), int(codes[i]), int(ref[i])) for i in np.nonzero(codes != ref)[0][:8]]
    bad = np.nonzero(ref & pw.BAD)[0]
    want = dict(n_checked=len(ref), n_bad=len(bad), bad_malformed=np.count_nonzero(ref & 16),
                bad_l3_csum=np.count_nonzero(ref & 1), bad_l3_len=np.count_nonzero(ref & 2),
                bad_l4_csum=np.count_nonzero(ref & 4), bad_udp_len=np.count_nonzero(ref & 8),
                first_bad=first + int(bad[0]) if len(bad) else NONE, n_ipv4=np.count_nonzero(l3 == 4),
                n_ipv6=np.count_nonzero(l3 == 6), n_inner=np.count_nonzero(ref & 64),
                n_nol4=np.count_nonzero(ref & 32), n_other=np.count_nonzero(ref & 128))
    got = {k: int(getattr(res, k)) for k in want}
    assert got == {k: int(v) for k, v in want.items()}


def check(fb, ref, l3, first=0, n=None, checks=pw.ALL, port=PORT, before=None):
    """One call with codes against the reference's slice (its failure bits masked as `checks` says);
    the call without codes gives the same result; the buffer's bytes are unchanged."""
    n = len(ref) - first if n is None else n
    want = ref[first:first + n] & np.uint8(checks | 0xF0)
    res, codes = fb.verify_wire(first=first, n=n, checks=checks, vxlan_port=port, codes=True)
    expect(res, codes, want, l3[first:first + n], first)
    plain = fb.verify_wire(first=first, n=n, checks=checks, vxlan_port=port)
    for k in pw.FIELDS:
        assert getattr(plain, k) == getattr(res, k), k
    if before is not None:
        assert np.array_equal(fb.packed(), before)
    return res, codes


def uploaded(ctx, data, off=None, flen=0):
    n = len(off) - 1 if off is not None else len(data) // flen
    fb = ctx.alloc_frames(max(n, 1), max(len(data), 16))
    fb.upload(data, offsets=off, fixed_len=flen)
    return fb


def packed_check(ctx, frames, ref=None, l3=None, **kw):
    data, off = wf.pack(frames)
    if ref is None:
        ref, l3 = reference(frames, kw.get("port", PORT))
    fb = uploaded(ctx, data, off)
    try:
        return check(fb, ref, l3, before=data, **kw)
    finally:
        fb.free()


# ------------------------------------------------------------------ 1. the class zoo and its byte mutants
@pytest.fixture(scope="module")
def zoo():
    z = wf.zoo()
    frames = []
    for _, f in z:
        frames.append(f)
        frames += wf.mutants(f)
    ref, l3 = reference(frames)
    return z, frames, ref, l3


def test_zoo_is_clean_by_its_own_sums(zoo):
    z, frames, ref, l3 = zoo
    assert len(frames) < 60000 and max(len(f) for f in frames) <= 200
    for label, f in z:
        assert pw.code(f, pw.ALL, PORT) == wf.expected_info(label), label
    for bit in (1, 2, 4, 8, 16, 32, 64, 128):  # the mutants reach every bit
        assert np.count_nonzero(ref & bit) > 50, bit


@pytest.mark.parametrize("lead", [0, 1], ids=["as-is", "behind-1-byte"])
def test_zoo_mutants(ctx, zoo, lead):
    """Every zoo frame and one copy of it per byte position with that byte changed, packed into one
    upload; then the same behind a leading 1-byte frame: every range starts on the other parity."""
    _, frames, ref, l3 = zoo
    if lead:
        frames = [b"\x5a"] + frames
        ref, l3 = np.concatenate(([16], ref)).astype(np.uint8), np.concatenate(([0], l3)).astype(np.uint8)
    res, _ = packed_check(ctx, frames, ref, l3)
    assert res.n_bad > 30000


# ------------------------------------------------------------------ 2. short and empty frames
def test_short_and_empty_frames(ctx):
    """Lengths 0..13 (MALFORMED) and 14..61 byte by byte, cut from clean frames of several classes; two
    runs of 512 empty frames (whole windows of them, the clean frames between keep the mean up); an
    empty frame last."""
    rng = np.random.default_rng(3)
    bases = [wf.frame(rng, t, l3, l4, 20) for t, l3, l4 in (("none", "v4", "udp"), ("q", "v4", "tcp"), ("none", "v6", "udp"),
                                                          ("adq", "v4", "icmp"), ("none", "v6", "tcp"))]
    frames = [b[:L] for L in range(0, 62) for b in bases]
    frames += [b""] * 512 + [bases[0], bases[2]] + bases * 400 + [b""] * 512 + [bases[1], b""]
    sh = wire_shape(0, len(frames), sum(map(len, frames)) // len(frames))
    assert 2 * sh["bf"] <= 512
    ref, l3 = reference(frames)
    assert np.all(ref[:14 * len(bases)] == 16) and ref[-1] == 16 and ref[-2] == 0
    packed_check(ctx, frames, ref, l3)
    for L in (1, 13):  # a fixed length under 14 is answered without a launch
        fb = uploaded(ctx, np.zeros(L * 9, np.uint8), flen=L)
        try:
            check(fb, np.full(9, 16, np.uint8), np.zeros(9, np.uint8), first=2, n=5)
        finally:
            fb.free()
    for L in (14, 15, 33, 60):
        fs = [bases[k % 5][:L] if len(bases[k % 5]) >= L else bases[0][:L] for k in range(40)]
        fb = uploaded(ctx, np.frombuffer(b"".join(fs), np.uint8), flen=L)
        try:
            check(fb, *reference(fs))
        finally:
            fb.free()


# ------------------------------------------------------------------ 3. the stage's edges
EDGE_LENGTHS = (STAGE // 8, STAGE // 4 - 1, STAGE // 4, STAGE // 4 + 1, 9043, 65535)


def _edge_positions(f, port=PORT):
    """Header bytes, and both edges of the first and last 16-B chunk (for a frame at an even and at
    an odd 16-B phase) of each range a frame of this shape has summed."""
    L = len(f)
    hdr = 74 if f[12:14] == b"\x86\xdd" else 92
    pos = set(range(0, hdr + 2))
    for lo in ((54,) if hdr == 74 else (34, 84)):
        for phase in (0, 1, 15):
            e0 = ((phase + lo) | 15) - phase
            s1 = ((phase + L - 1) & ~15) - phase
            pos |= {lo, e0, e0 + 1, s1 - 1, s1, L - 1}
    return sorted(p for p in pos if 0 <= p < L)


def _edge_set(kind, L):
    base = wf.long_frame(kind, L)
    out = [base]
    for p in _edge_positions(base):
        m = bytearray(base)
        m[p] ^= 1 << (p % 8)
        out.append(bytes(m))
    return out


@pytest.fixture(scope="module")
def edges():
    sets = {(k, L): _edge_set(k, L) for k in ("vx4", "tcp6") for L in EDGE_LENGTHS}
    sets[("vx4_zero", 4097)] = _edge_set("vx4_zero", 4097)
    sets[("tcp6", 65535)].append(wf.long_frame("tcp6", 65535, fill=0xFF))
    return {key: (fs,) + reference(fs) for key, fs in sets.items()}


def test_stage_lengths_are_the_edges():
    assert EDGE_LENGTHS[:4] == (2048, 4095, 4096, 4097)
    got = {L: vr.shape_class(L, 100) for L in EDGE_LENGTHS[:4]}  # pb_vst_kernel's table holds for this kernel
    assert {L: wire_shape(L, 100)["G"] for L in EDGE_LENGTHS[:4]} == {L: g for L, (g, _) in got.items()}
    assert got == {2048: (32, "staged"), 4095: (64, "both"), 4096: (64, "staged"), 4097: (64, "unstaged")}


@pytest.mark.parametrize("kind,L", [(k, L) for k in ("vx4", "tcp6") for L in EDGE_LENGTHS] + [("vx4_zero", 4097)])
def test_stage_edges_fixed(ctx, edges, kind, L):
    """Copies of one long clean frame at a fixed length: one per header byte and per edge of its summed
    ranges' first and last chunks, with that byte changed; at 65,535 B also one of 0xFF payload bytes."""
    fs, ref, l3 = edges[(kind, L)]
    assert ref[0] == (64 if kind != "tcp6" else 0) and np.count_nonzero(ref & pw.BAD) >= len(fs) // 2
    if kind == "tcp6" and L == 65535:
        assert ref[-1] == 0 and fs[-1][-1000:] == b"\xff" * 1000
    data = np.frombuffer(b"".join(fs), np.uint8)
    fb = uploaded(ctx, data, flen=L)
    try:
        check(fb, ref, l3, before=data)
    finally:
        fb.free()


@pytest.mark.parametrize("lead", [0, 1])
def test_stage_edges_packed(ctx, edges, lead):
    """All of them in one packed upload with a 1-byte frame after every long one (the next starts on the
    other parity), short frames among them: staged and unstaged windows in one launch."""
    rng = np.random.default_rng(5)
    small = [wf.frame(rng, "none", "v4", "udp", 18), wf.frame(rng, "q", "v6", "tcp", 7)]
    frames = [b"\x00"] * lead
    for key in sorted(edges):
        fs = edges[key][0]
        step = 1 if key[1] <= 4097 else 4  # a sample of the two largest sets
        for k, f in enumerate(fs[::step]):
            frames += [f, b"\x01"] if k % 3 else [f, small[k % 2]]
        frames += small * 40
    off = np.cumsum([0] + [len(f) for f in frames])
    long_at = [int(off[i]) & 1 for i, f in enumerate(frames) if len(f) > 2000]
    assert 0 in long_at and 1 in long_at
    mean = int(off[-1]) // len(frames)
    fl = vr.window_flags(off, 0, len(frames), wire_shape(0, len(frames), mean)["bf"])
    assert {s for _, s in fl} == {True, False}
    packed_check(ctx, frames)


# ------------------------------------------------------------------ 4. G, sub-ranges, masks, port
@pytest.mark.parametrize("G,L,k", [(8, 0, 0), (16, 1500, 30), (32, 4097, 40), (64, 9043, 60)])
def test_each_group_size(ctx, zoo, edges, G, L, k):
    """Zoo frames and mutants with k long frames (clean and changed) mixed in: the mean picks G."""
    _, zf, _, _ = zoo
    frames = list(zf[:4000:50])
    if k:
        longs = edges[("vx4", L)][0] if L != 1500 else _edge_set("vx4", 1500)
        for i in range(k):
            frames.insert(1 + 2 * i, longs[(i * 7) % len(longs)])
    mean = sum(map(len, frames)) // len(frames)
    assert wire_shape(0, len(frames), mean)["G"] == G
    packed_check(ctx, frames)


def test_sub_ranges(ctx, zoo):
    """first_frame != 0 and n < n_frames, bad frames just outside the range and at its ends."""
    _, frames, ref, l3 = zoo
    frames, ref, l3 = list(frames[:2995]), ref[:2995], l3[:2995]
    assert not ref[0] & pw.BAD
    for at in (40, 600, 1300, 2100, 2900):  # a clean frame between two mutants
        i = next(i for i in range(at, len(ref)) if ref[i - 1] & pw.BAD and ref[i] & pw.BAD)
        frames.insert(i, frames[0])
        ref, l3 = np.insert(ref, i, ref[0]), np.insert(l3, i, l3[0])
    clean = [i for i in range(len(ref)) if not ref[i] & pw.BAD]
    data, off = wf.pack(frames)
    fb = uploaded(ctx, data, off)
    try:
        for a, b in ((clean[1], clean[2]), (clean[1] + 1, clean[2]), (clean[1], clean[2] + 1), (1, 2), (7, 2999),
                     (clean[3], clean[3] + 1), (2999, 3000), (0, 3000)):
            res, _ = check(fb, ref, l3, first=a, n=b - a, before=data)
        bad = (ref & pw.BAD) != 0
        lone = [i for i in range(1, 2999) if not bad[i] and bad[i - 1] and bad[i + 1]]
        assert len(lone) >= 5
        for i in lone:
            res, _ = check(fb, ref, l3, first=i, n=1)
            assert res.n_bad == 0 and res.first_bad == NONE
    finally:
        fb.free()


def test_masks(ctx, zoo):
    """Every mask 0..15 over frames of every code: failure bits only where enabled, info bits always."""
    _, frames, ref, l3 = zoo
    pick = sorted({int(np.nonzero(ref == c)[0][k]) for c in np.unique(ref) for k in range(min(3, np.count_nonzero(ref == c)))})
    frames = [frames[i] for i in pick]
    assert len(np.unique(ref)) > 20
    data, off = wf.pack(frames)
    kinds = reference(frames)[1]
    fb = uploaded(ctx, data, off)
    try:
        for m in range(16):
            want = np.array([pw.code(f, m, PORT) for f in frames], dtype=np.uint8)
            res, codes = fb.verify_wire(checks=m, vxlan_port=PORT, codes=True)
            expect(res, codes, want, kinds)
            assert not np.any(codes & (15 & ~m))
    finally:
        fb.free()


@pytest.mark.parametrize("port", [0, 4790])
def test_port_off_or_wrong(ctx, zoo, port):
    """No INNER without the port: the outer verdict alone."""
    z, _, _, _ = zoo
    frames = [f for label, f in z if "-vx" in label]
    frames += [wf.mutants(f)[len(f) - 3] for f in frames[:60]]  # an inner byte changed
    ref, l3 = reference(frames, port)
    assert not np.any(ref & 64)
    res, codes = packed_check(ctx, frames, ref, l3, port=port)
    assert res.n_inner == 0
    with_port = reference(frames, PORT)[0]
    assert np.all(with_port & 64) and np.count_nonzero(with_port != ref | 64) > 20


# ------------------------------------------------------------------ 5. arguments
def test_argument_errors_and_empty_range(ctx, zoo):
    lib = ctx.lib
    _, frames, ref, l3 = zoo
    data, off = wf.pack(frames[:50])
    fb = uploaded(ctx, data, off)
    never = ctx.alloc_frames(16, 4096)
    try:
        ok, res = WireOpts(15, 0, PORT), WireResult()

        def call(c=ctx.h, f=fb.ptr, first=0, n=50, o=ok, r=res):
            return lib.pbgpu_verify_wire(c, f, first, n, C.byref(o) if o is not None else None,
                                         C.byref(r) if r is not None else None, None)

        assert call() == 0
        assert call(c=None) == EINVAL and call(f=None) == EINVAL and call(o=None) == EINVAL and call(r=None) == EINVAL
        assert call(f=never.ptr, n=1) == EINVAL
        assert call(first=1, n=50) == EINVAL and call(first=51, n=0) == EINVAL and call(first=2**63, n=2**63) == EINVAL
        for bad in (WireOpts(16, 0, PORT), WireOpts(0x100, 0, 0), WireOpts(15, 1, 0)):
            assert call(o=bad) == EINVAL
        for k in range(3):
            o = WireOpts(15, 0, 0)
            o.reserved[k] = 1
            assert call(o=o) == EINVAL
        for first in (0, 17, 50):  # n == 0
            res, codes = fb.verify_wire(first=first, n=0, vxlan_port=PORT, codes=True)
            assert len(codes) == 0 and res.first_bad == NONE and res.device_ms == 0
            assert all(getattr(res, k) == 0 for k in pw.FIELDS if k != "first_bad")
        assert np.array_equal(fb.packed(), data)
    finally:
        fb.free()
        never.free()


# ------------------------------------------------------------------ 6. loops
def _edge_indices(sh, n):
    """Frames at both edges of every window turn, in the workgroup regions at both ends of
    pb_xcd_region's numbering (workgroup b takes region (b & 7) * per + (b >> 3)), and the ragged tail."""
    grid, wgf, bf = sh["grid"], sh["wgf"], sh["bf"]
    per = grid >> 3
    out = {n - 1}
    for r in (0, 1, per - 1, per, per + 1, 2 * per, 4 * per - 1, 7 * per, 8 * per - 1, 8 * per, grid // 2, grid - 2,
              grid - 1):
        for k in range(0, wgf, bf):
            out |= {r * wgf + k, r * wgf + k + bf - 1}
    out |= set(range(n - (n % wgf), n))
    return sorted(i for i in out if 0 <= i < n)


def _loop_case(ctx, base, n, fixed, nw):
    """n frames tiled from a few clean ones, some 50 of them changed near their end; the reference's
    codes are the clean ones' tiled, the changed frames' computed one by one."""
    lens = np.array([len(f) for f in base])
    reps = -(-n // len(base))
    off = np.concatenate(([0], np.cumsum(np.tile(lens, reps)[:n]))).astype(np.uint64)
    data = np.tile(np.frombuffer(b"".join(base), np.uint8), reps)[:int(off[-1])].copy()
    cref, cl3 = reference(base)
    assert not np.any(cref & (pw.BAD | pw.NOL4))
    ref, l3 = np.tile(cref, reps)[:n].copy(), np.tile(cl3, reps)[:n].copy()
    sh = wire_shape(fixed, n, int(off[-1]) // n)
    assert sh["nw"] == nw and sh["grid"] >= 16 and (nw > 1 or sh["bf"] >= 2 * (WT // sh["G"]))  # a loop in the workgroup
    idx = _edge_indices(sh, n)
    assert 20 <= len(idx) <= 100
    for j, i in enumerate(idx):
        a, L = int(off[i]), int(lens[i % len(base)])
        data[a + L - 1 - j % 4] ^= 0x10
        ref[i], l3[i] = pw.walk(data[a:a + L].tobytes(), pw.ALL, PORT)
        assert ref[i] & pw.BAD
    fb = uploaded(ctx, data, None if fixed else off, flen=fixed)
    try:
        res, _ = check(fb, ref, l3, before=data)
        assert res.first_bad == idx[0] == 0 and res.n_bad == len(idx)
        res, _ = check(fb, ref, l3, first=1, n=n - 2)
        assert res.first_bad == idx[1] and res.n_bad == len(idx) - 2
    finally:
        fb.free()


def test_loops_packed(ctx):
    """2^18 + 29 packed frames of 640..1459 B: a workgroup takes two windows, the last one is ragged."""
    base = [wf.long_frame(("vx4_zero", "tcp6", "vx4")[k % 3], 640 + 13 * k) for k in range(64)]
    _loop_case(ctx, base, (1 << 18) + 29, 0, 2)


def test_loops_fixed_60(ctx):
    """2^21 frames of 60 B: eight rounds per window, 8192 workgroups."""
    rng = np.random.default_rng(11)
    base = [wf.frame(rng, "none", "v4", "tcp", 6), wf.frame(rng, "none", "v4", "udp", 18),
            wf.frame(rng, "q", "v4", "udp", 14), wf.frame(rng, "none", "v4", "icmp", 18)]
    assert {len(f) for f in base} == {60}
    _loop_case(ctx, base, 1 << 21, 60, 1)


# ------------------------------------------------------------------ 7. the library's own pipelines
def _clean(fb, n, port=0, **counts):
    """Clean under WIRE_ALL, with the expected counts; the codes agree with pywire on the frames fetched."""
    res, codes = fb.verify_wire(vxlan_port=port, codes=True)
    frames = fb.frames()
    assert len(frames) == n
    ref, l3 = reference(frames, port)
    expect(res, codes, ref, l3)
    assert res.n_checked == n and res.n_bad == 0 and res.first_bad == NONE
    want = dict(n_ipv4=n, n_ipv6=0, n_inner=0, n_nol4=0, n_other=0)
    want.update(counts)
    assert {k: int(getattr(res, k)) for k in want} == want
    return res


@pytest.mark.parametrize("cfg", ["c2_udp_64", "c4_tcp_syn", "c5_icmp_echo", "c3_udp_var"])
def test_pipelines(ctx, cfg):
    n = 1 << 12
    seq = Sequence.from_config(pc.get(cfg))
    ctx.load_sequence(0, seq, pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n))
    mf, mb = ctx.build_size(0, n)
    a = ctx.alloc_frames(mf, mb + 80 * mf)
    b = ctx.alloc_frames(mf, mb + 80 * mf)
    try:
        ctx.build(0, 3, n, fb)
        _clean(fb, n)  # follows the build on the stream
        fb.encap(a, mode=ENCAP_VLAN, tci=100)
        _clean(a, n)
        fb.encap(a, mode=ENCAP_VXLAN, **VX)
        _clean(a, n, PORT, n_inner=n)
        res = a.verify_wire()  # without the port: the outer header alone, its UDP checksum 00 00
        assert res.n_bad == 0 and res.n_inner == 0 and res.n_nol4 == n
        a.encap(b, mode=ENCAP_VLAN, tci=0x2064)  # a tag in front of the tunnel
        _clean(b, n, PORT, n_inner=n)
        fb.xlat46(a, opts=XlatOpts.make(PREFIX))
        _clean(a, n, n_ipv4=0, n_ipv6=n)
        a.encap(b, mode=ENCAP_VXLAN, **VX)
        _clean(b, n, PORT, n_inner=n)
        st = fb.stamp(t0_ns=1_700_000_000_000_000_000, step_ps=672000, first_index=9)
        assert st.n_stamped == (0 if cfg == "c4_tcp_syn" else n)  # 16 bytes do not fit a SYN's 6-B payload
        _clean(fb, n)
    finally:
        for x in (fb, a, b):
            x.free()


def test_pipeline_fragments(ctx):
    """9043-B frames fragmented at mtu 1500: every output frame is a fragment, so none has an L4 checksum to check."""
    n = 64
    ctx.load_sequence(0, Sequence.from_config(pc.get("udp_jumbo_fixed_odd")), pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n))
    dst = ctx.alloc_frames(n * 8, n * 9043 + n * 8 * 34 + 64)
    try:
        ctx.build(0, 0, n, fb)
        assert int(fb.f.fixed_len) == 9043
        _clean(fb, n)
        fr = fb.fragment(dst, mtu=1500)
        assert fr.n_out == 7 * n
        _clean(dst, int(fr.n_out), n_nol4=int(fr.n_out))
    finally:
        fb.free()
        dst.free()


def test_inner_payload_flip_is_seen_here_only(ctx):
    """One inner payload byte of a VXLAN buffer flipped: pbgpu_verify with IP_CSUM | TOT_LEN - all it can
    ask of a VXLAN frame - passes the buffer; pbgpu_verify_wire reports L4_CSUM on that frame alone."""
    n, victim = 1 << 10, 777
    ctx.load_sequence(0, Sequence.from_config(pc.get("c2_udp_64")), pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n))
    vx = ctx.alloc_frames(n, n * 114 + 64)
    try:
        ctx.build(0, 0, n, fb)
        fb.encap(vx, mode=ENCAP_VXLAN, **VX)
        data = vx.packed().copy()
        assert len(data) == n * 114
        data[victim * 114 + 113] ^= 0x40
        vx.upload(data, fixed_len=114)
        old = vx.verify(checks=pbgpu.VERIFY_IP_CSUM | pbgpu.VERIFY_TOT_LEN)
        assert old.n_bad == 0
        res, codes = vx.verify_wire(vxlan_port=PORT, codes=True)
        assert res.n_bad == 1 and res.bad_l4_csum == 1 and res.first_bad == victim and res.n_inner == n
        want = np.full(n, pw.INNER, np.uint8)
        want[victim] |= pw.L4_CSUM
        assert np.array_equal(codes, want)
    finally:
        fb.free()
        vx.free()


# ------------------------------------------------------------------ 8. both verifiers on one context
def test_both_verifiers_take_turns_on_one_context(ctx):
    """pbgpu_verify and pbgpu_verify_wire share one record scratch and one mapped result buffer; their
    records have 5 and 11 counts.  Three buffers on one context: 4,096 frames of 64 B with mutants (19
    workgroups of the wire verifier, 64 waves of the page verifier), 8 clean frames of 1500 B (one
    workgroup in both) and 300 packed frames of c3_udp_var; the calls alternate, each with codes, and
    every result and code array is compared with its reference: a stale count, a stale first_bad or a
    record read at the other call's stride shows as a wrong count.  Every failure count of both calls
    is nonzero on the first buffer except pbgpu_verify's bad_short, which no frame of 64 B can raise."""
    def built(cfg, n):
        ctx.load_sequence(0, Sequence.from_config(pc.get(cfg)), pc.SEED_BASE)
        fb = ctx.alloc_frames(*ctx.build_size(0, n))
        ctx.build(0, 0, n, fb)
        return fb

    bufs = [built("c2_udp_64", 4096), built("c2_udp_1500", 8), built("c3_udp_var", 300)]
    try:
        a = bufs[0]
        assert [int(b.f.fixed_len) for b in bufs] == [64, 1500, 0]
        assert wire_shape(64, 4096)["grid"] == 19 and vr.verify_shape(64, 0, 4096, 64)["grid"] == 64
        assert wire_shape(1500, 8)["grid"] == 1 and vr.verify_shape(1500, 0, 8, 1500)["grid"] == 1
        data = a.packed().copy()
        for k, f in enumerate((5, 700, 2045, 3333, 4090)):  # in several workgroups and pages, not frame 0
            o = f * 64
            data[o + 22] ^= 0x01 << k              # TTL: the IPv4 checksum
            data[o + 64 + 17] ^= 0x04              # the next frame's tot_len (and its IPv4 checksum)
            data[o + 128 + 63 - k] ^= 0x80         # a payload byte: the L4 checksum
            data[o + 192 + 39] ^= 0x02             # the UDP length (and the L4 checksum)
            data[o + 256 + 14] = 0x55              # version 5: malformed as sent, a wrong IPv4 sum to pbgpu_verify
        a.upload(data, fixed_len=64)
        refs = []
        for b in bufs:
            d, off = b.packed(), b.offsets()
            frames = [d[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(off) - 1)]
            refs.append((vr.ref_codes(d, off),) + reference(frames))
        v0, w0, _ = refs[0]
        assert all(np.count_nonzero(v0 & bit) for bit in (1, 2, 4)) and all(np.count_nonzero(w0 & bit) for bit in (1, 2, 4, 8, 16))
        assert v0[0] == 0 and w0[0] == 0 and not refs[1][0].any() and not (refs[1][1] & pw.BAD).any()
        for call, i in (("wire", 0), ("verify", 1), ("wire", 1), ("verify", 0), ("wire", 2), ("verify", 2), ("wire", 0)):
            vref, wref, l3 = refs[i]
            if call == "wire":
                res, codes = bufs[i].verify_wire(vxlan_port=PORT, codes=True)
                expect(res, codes, wref, l3)
            else:
                res, codes = bufs[i].verify(codes=True)
                vr.expect(res, codes, vref)
    finally:
        for b in bufs:
            b.free()
