"""pbgpu_segment on the GPU: every output byte and every field of the result against tests/pyseg.py,
which writes the segments from their definition with `struct` and Python integers, and the product's
other halves (pbgpu_verify, pbgpu_verify_wire) as judges of the built batches.

Every destination is first filled with 0xA5 by an upload, so a stray write shows, and is compared
whole: the frames, zeros up to the next multiple of 16, 0xA5 after that.  The destination's
metadata and device offsets are checked, and the source is compared with itself afterwards."""
import ctypes as C
import struct

import numpy as np
import pytest

import pb_configs as pc
import pbgpu
import pyencap
import pyfrag
import pypcap
import pyseg
import seg_frames as sf
from pbgpu import ENCAP_VXLAN, GpuContext, PbError, SegOpts, SegResult, Sequence, XlatOpts

pytestmark = pytest.mark.gpu

SLACK = 4096 + 64  # bytes of the destination past the frames, watched for stray writes
EINVAL, ENOSPC = -22, -28
VX = dict(dst_mac=bytes.fromhex("0200000000a2"), src_mac=bytes.fromhex("0200000000a1"), src_ip=bytes([192, 0, 2, 1]),
          dst_ip=bytes([198, 51, 100, 2]), vni=0x123456)
PREFIX = bytes.fromhex("0064ff9b") + bytes(8)


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def uploaded(ctx, data, off=None, flen=0):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = len(off) - 1 if off is not None else len(data) // flen
    fb = ctx.alloc_frames(max(n, 1), max(len(data), 16))
    fb.upload(data, offsets=off, fixed_len=flen)
    return fb


def fresh_dst(ctx, nbytes, frames=0):
    """A destination of nbytes rounded up to 16 plus SLACK, every byte 0xA5."""
    cap = ((nbytes + 15) & ~15) + SLACK
    dst = ctx.alloc_frames(max(cap // 16, frames), cap)
    dst.upload(np.full(cap, 0xA5, dtype=np.uint8), fixed_len=16)
    return dst, cap


def pack(frames):
    off = np.concatenate([[0], np.cumsum([len(f) for f in frames], dtype=np.uint64)]).astype(np.uint64)
    return np.frombuffer(b"".join(frames), dtype=np.uint8), off


def check_seg(ctx, fb, frames, mss, flags=0, first=0, n=None, keep=False):
    """Segments fb's frames [first, first + n) and compares the whole destination and the result;
    `frames` are the buffer's frames as bytes.  Returns the reference frames (and with keep the
    destination)."""
    n = len(frames) - first if n is None else n
    nl4, fid = bool(flags & 1), bool(flags & 2)
    refs, cnt = pyseg.segment_all(frames[first:first + n], mss, flags)
    ref = b"".join(refs)
    total = len(ref)
    assert ctx.segment_size(fb, first, n, mss, nl4, fid) == (len(refs), total)
    bf, bb = ctx.segment_bound(fb, first, n, mss, nl4, fid)
    assert bf >= len(refs) and bb >= total
    before = fb.packed().copy()
    meta_before = (int(fb.f.n_frames), int(fb.f.fixed_len))
    dst, cap = fresh_dst(ctx, total, len(refs))
    try:
        res = fb.segment(dst, first, n, mss, nl4, fid)
        got_res = {k: int(getattr(res, k)) for k in cnt}
        assert got_res == cnt
        assert res.device_ms >= 0
        got = dst.stream(cap)
        r16 = (total + 15) & ~15
        want = np.frombuffer(ref, dtype=np.uint8)
        if not np.array_equal(got[:total], want):
            bad = int(np.nonzero(got[:total] != want)[0][0])
            raise AssertionError((bad, got[max(0, bad - 8):bad + 8].tobytes().hex(), ref[max(0, bad - 8):bad + 8].hex()))
        assert not got[total:r16].any()
        assert (got[r16:] == 0xA5).all()
        flen = int(fb.f.fixed_len)
        keeps = flen and flen - 42 <= mss and n
        assert (int(dst.f.n_frames), int(dst.f.fixed_len), int(dst.f.total_bytes)) == \
            (len(refs), flen if keeps else 0, total)
        if not keeps and n:
            want_off = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.uint64)
            assert np.array_equal(dst.offsets(), want_off)
        assert (int(fb.f.n_frames), int(fb.f.fixed_len)) == meta_before and np.array_equal(fb.packed(), before)
    except BaseException:
        dst.free()
        raise
    if keep:
        return refs, dst
    dst.free()
    return refs


def frame_of(proto, L, seed):
    """An L-byte frame: UDP or TCP (H = 20) with right checksums where L holds the headers, else bytes."""
    hl = 42 if proto == "udp" else 54
    if L < hl:
        return sf.payload(L, seed)
    return sf.udp(L - 42, seed, ident=seed) if proto == "udp" else sf.tcp(L - 54, seed, ident=seed, seq=seed * 977,
                                                                            flags=seed & 0xFF)


# ------------------------------------------------------------------ 1. fixed lengths, uploaded
def _fixed_cases():
    out = []
    for proto, hl in (("udp", 42), ("tcp", 54)):
        for mss in (8, 9, 1460, 8960):
            for L in sorted({14, 34, hl, hl + 1, hl + mss - 1, hl + mss, hl + mss + 1, hl + 2 * mss - 1, hl + 2 * mss,
                             hl + 2 * mss + 1, 65535}):
                out.append((proto, mss, L))
    return out


@pytest.mark.parametrize("proto,mss,L", _fixed_cases())
def test_fixed_uploaded(ctx, proto, mss, L):
    hl = 42 if proto == "udp" else 54
    k = 1 if L - hl <= mss else -(-(L - hl) // mss)
    rec = L + hl * (k - 1)  # output bytes per source frame
    if rec <= 4096:  # records ending one before, on and one after output byte 4096
        ns = {1, max(1, 4096 // rec - 1), 4096 // rec, 4096 // rec + 1, 4096 // rec + 2}
    else:
        ns = {1, 3}
    nmax = max(ns)
    frames = [frame_of(proto, L, 1000 * L + j) for j in range(nmax)]
    fb = uploaded(ctx, pack(frames)[0], flen=L)
    try:
        for n in sorted(ns - {0}):
            check_seg(ctx, fb, frames, mss, n=n)
            if n > 1:  # a range that starts on another source alignment
                check_seg(ctx, fb, frames, mss, first=1, n=n - 1)
    finally:
        fb.free()


# ------------------------------------------------------------------ 2. variable lengths, uploaded
def _mixed_frames():
    rng = np.random.default_rng(15)
    frames = []
    for j in range(3000):
        u = rng.random()
        ident = (0xFFFD + j) & 0xFFFF if j % 7 == 0 else int(rng.integers(0, 65536))
        seq = 0xFFFFFF00 + (j & 0xFF) if j % 5 == 0 else int(rng.integers(0, 1 << 32))
        fl = j & 0xFF  # every flag combination
        if 1000 <= j < 1400 or u < 0.25:
            frames.append(sf.payload(14, j))  # runs of 14-B frames: 293 records to a page
        elif u < 0.35:
            frames.append(sf.udp(18, j, ident))
        elif u < 0.45:
            frames.append(sf.udp(int(rng.integers(0, 3000)), j, ident))
        elif u < 0.55:
            frames.append(sf.tcp(int(rng.integers(0, 3000)), j, ident, seq, fl))
        elif u < 0.62:
            frames.append(sf.tcp(int(rng.integers(0, 3000)), j, ident, seq, fl, H=24))
        elif u < 0.69:
            frames.append(sf.tcp(int(rng.integers(0, 3000)), j, ident, seq, fl, H=60))
        elif u < 0.75:
            frames.append(sf.udp([537, 1461][j & 1], j, ident))  # P = mss + 1: a last segment of one byte
        elif u < 0.81:
            frames.append(sf.tcp([537, 1461][j & 1], j, ident, seq, fl, H=[20, 32][(j >> 1) & 1]))
        elif u < 0.85:
            frames.append(sf.tcp(9001, j, ident, seq, fl))
        elif u < 0.93:
            frames.append(list(sf.ineligible(int(rng.integers(60, 2500)), j).values())[j % 7])
        else:
            frames.append(sf.payload(int(rng.integers(15, 1700)), j))
    frames[500] = sf.udp(65493, 500, 0xFFFE, pay=b"\xff" * 65493)  # 65,535 B of 0xFF payload
    frames[501] = sf.tcp(65481, 501, 0xFFFF, 0xFFFFFF00, 0x99, pay=b"\xff" * 65481)
    for i, (name, f) in enumerate(sorted(sf.ineligible(1700, 77).items())):
        frames[2000 + i] = f
    f = bytearray(sf.tcp(39, 9, H=20))
    f[46] = 0xF0  # a TCP header past the frame's end
    frames[2010] = bytes(f)
    for i, mss in enumerate((536, 1460, 8)):  # a computed UDP checksum of 0x0000, stored as 0xFFFF
        frames[2020 + i] = sf.udp_zero_first(mss, 30 + i)
        assert pyseg.segment(frames[2020 + i], mss)[0][40:42] == b"\xff\xff"
    return frames


@pytest.fixture(scope="module")
def mixed(ctx):
    frames = _mixed_frames()
    data, off = pack(frames)
    fb = uploaded(ctx, data, off=off)
    yield fb, frames
    fb.free()


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("mss", [536, 1460])
def test_variable_mixed(ctx, mixed, mss, flags):
    fb, frames = mixed
    refs = check_seg(ctx, fb, frames, mss, flags)
    if flags == 0:
        pyseg.check_all(frames, refs, mss, flags)


@pytest.mark.parametrize("mss", [8, 9])
def test_variable_mixed_small_mss(ctx, mixed, mss):
    fb, frames = mixed
    check_seg(ctx, fb, frames, mss, first=495, n=10)  # the two 65,535-B frames of 0xFF among them
    check_seg(ctx, fb, frames, mss, first=1990, n=40)
    check_seg(ctx, fb, frames, mss, flags=3, first=1395, n=30)


def test_one_frame_into_8187_records(ctx):
    """A 65,535-B UDP frame at mss 8 among short ones: 8,187 records of 50 B, 81 to a page."""
    frames = [sf.payload(14, 1), sf.udp(18, 2), sf.payload(14, 3), sf.udp(65493, 4, 0xFFF0), sf.payload(14, 5),
              sf.udp(9, 6), sf.udp(8, 7), sf.tcp(17, 8, H=60)]
    data, off = pack(frames)
    fb = uploaded(ctx, data, off=off)
    try:
        refs = check_seg(ctx, fb, frames, 8)
        assert len(refs) == 1 + 3 + 1 + 8187 + 1 + 2 + 1 + 3
    finally:
        fb.free()


# ------------------------------------------------------------------ 3. sub-ranges
def test_subrange_every_source_alignment(ctx, mixed):
    """1621-B frames from first_frame 0..16: the range's first source byte, and with it every slice
    boundary, at every alignment mod 16."""
    for proto in ("udp", "tcp"):
        frames = [frame_of(proto, 1621, 7000 + j) for j in range(30)]
        fb = uploaded(ctx, pack(frames)[0], flen=1621)
        try:
            assert {(1621 * f) % 16 for f in range(17)} == set(range(16))
            for first in range(17):
                check_seg(ctx, fb, frames, 536, first=first, n=12)
            check_seg(ctx, fb, frames, 9, first=3, n=2)
        finally:
            fb.free()
    fb, frames = mixed
    for first in range(990, 1007):
        check_seg(ctx, fb, frames, 1460, first=first, n=500)
    check_seg(ctx, fb, frames, 1460, first=2999, n=1)


# ------------------------------------------------------------------ 4. built on the GPU, judged by the verifiers
def tcp_jumbo():
    c = pc.c4_tcp_syn()
    c["tcp"] = {"sport": 0, "dport": 80, "ack": 1, "psh": 1, "fin": 1, "cwr": 1}
    c["payloads"] = [{"length": {"min": 9001, "max": 9001}}]
    return c


def built(ctx, cfg, n_iter, first_iter=777):
    seq = Sequence.from_config(cfg)
    ctx.load_sequence(0, seq, pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n_iter))
    ctx.build(0, first_iter, n_iter, fb)
    ctx.sync()
    return fb


def test_copy_path_c4_tcp_syn(ctx):
    fb = built(ctx, pc.get("c4_tcp_syn"), 4096)
    try:
        frames = fb.frames()
        refs, dst = check_seg(ctx, fb, frames, 1460, keep=True)
        try:
            assert int(dst.f.fixed_len) == 60 and refs == frames
        finally:
            dst.free()
    finally:
        fb.free()


@pytest.mark.parametrize("proto", ["udp", "tcp"])
def test_built_jumbo_judged_by_the_verifiers(ctx, proto):
    n_iter = 1 << 10
    fb = built(ctx, pc.get("udp_jumbo_fixed_odd") if proto == "udp" else tcp_jumbo(), n_iter)
    mss = 1472 if proto == "udp" else 1460
    try:
        frames = fb.frames()
        assert len(frames) == n_iter and len(frames[0]) == (9043 if proto == "udp" else 9055)
        refs, dst = check_seg(ctx, fb, frames, mss, keep=True)
        try:
            m = len(refs)
            assert m == 7 * n_iter
            pyseg.check_all(frames[:40], refs[:280], mss)
            res = dst.verify(checks=pbgpu.VERIFY_ALL)
            assert (int(res.n_checked), int(res.n_bad)) == (m, 0)
            wres = dst.verify_wire(checks=pbgpu.WIRE_ALL)
            assert (int(wres.n_checked), int(wres.n_bad), int(wres.n_nol4)) == (m, 0, 0)
            # landed in 2-KiB slots, which the 9-KB source frames do not fit
            slot, k0, kn = 2048, 7 * 500 - 3, 64
            umem = np.zeros(slot * kn, dtype=np.uint8)
            lens = dst.to_umem(umem, slot, k0, kn)
            assert [bytes(umem[i * slot:i * slot + int(lens[i])]) for i in range(kn)] == refs[k0:k0 + kn]
            with pytest.raises(PbError):
                fb.to_umem(umem, slot, 0, 8)
            # one payload byte flipped in dst: exactly the segment holding it is bad
            victim = 7 * 333 + 4
            off = dst.offsets()
            data = dst.packed().copy()
            data[int(off[victim]) + 700] ^= 0x40
            bad = uploaded(ctx, data, off=off)
            try:
                res, codes = bad.verify(checks=pbgpu.VERIFY_ALL, codes=True)
                assert int(res.n_bad) == 1 and int(res.first_bad) == victim
                assert codes[victim] == pbgpu.VERIFY_L4_CSUM and not np.delete(codes, victim).any()
                wres, wcodes = bad.verify_wire(checks=pbgpu.WIRE_ALL, codes=True)
                assert int(wres.n_bad) == 1 and wcodes[victim] == pbgpu.WIRE_L4_CSUM
            finally:
                bad.free()
            # a flip in the source's checksum field changes nothing: the checksum is recomputed
            at = 40 if proto == "udp" else 50
            sdata = fb.packed().copy()
            L = len(frames[0])
            sdata[L * 100 + at] ^= 0xFF
            sdata[L * 101 + at + 1] ^= 0x01
            src2 = uploaded(ctx, sdata, flen=L)
            dst2, cap2 = fresh_dst(ctx, len(data), m)
            try:
                src2.segment(dst2, mss=mss)
                assert np.array_equal(dst2.packed(), dst.packed())
                # under NO_L4_CSUM the flipped bytes are what every segment of that frame carries
                src2.segment(dst2, mss=mss, no_l4_csum=True)
                out = dst2.frames()
                assert all(out[700 + i][at] == sdata[L * 100 + at] for i in range(7))
            finally:
                dst2.free()
                src2.free()
        finally:
            dst.free()
    finally:
        fb.free()


# ------------------------------------------------------------------ 5. composition
def test_composition(ctx, mixed):
    fb, frames = mixed
    n = 700
    refs, sg = check_seg(ctx, fb, frames, 1460, flags=2, first=1450, n=n, keep=True)
    try:
        assert sg.frames() == refs
        m = len(refs)
        # landed in 4-KiB slots: the longest frame left is a copied one under 2500 B
        slot = 4096
        umem = np.zeros(slot * m, dtype=np.uint8)
        lens = sg.to_umem(umem, slot, 0, m)
        assert [bytes(umem[i * slot:i * slot + int(lens[i])]) for i in range(m)] == refs
        # packed into a pcap stream
        assert sg.pcap_bytes(t0_ns=10**18, step_ps=6_720_000).tobytes() == pypcap.pcap_stream(refs, 10**18, 6_720_000)
        # segmented again at a smaller mss that divides the first: as segmenting the source at that mss
        again = check_seg(ctx, sg, refs, 365, flags=2)
        direct, _ = pyseg.segment_all(frames[1450:1450 + n], 365, 2)
        assert again == direct
        # fragmented
        frs, cnt = pyfrag.fragment_all(refs, 576, True)
        fr = ctx.alloc_frames(len(frs), sum(map(len, frs)) + 16)
        try:
            sg.fragment(fr, mtu=576, ignore_df=True)
            assert fr.frames() == frs
        finally:
            fr.free()
        # VXLAN-encapsulated, the inner segments checked
        vx_refs = [pyencap.vxlan(f, **VX) for f in refs]
        vx = ctx.alloc_frames(m, sum(len(f) for f in vx_refs) + 16)
        try:
            sg.encap(vx, mode=ENCAP_VXLAN, **VX)
            assert vx.frames() == vx_refs
        finally:
            vx.free()
    finally:
        sg.free()


def test_segments_translated_and_encapsulated_stay_clean(ctx):
    """Built TCP segments through pbgpu_xlat46, and through a VXLAN tunnel: pbgpu_verify_wire finds
    every L4 checksum, the inner ones too, right."""
    n = 256
    fb = built(ctx, tcp_jumbo(), n)
    sg = ctx.alloc_frames(7 * n, 7 * n * 1600)
    x6 = ctx.alloc_frames(7 * n, 7 * n * 1700)
    try:
        res = fb.segment(sg, mss=1460)
        m = int(res.n_out)
        assert (m, int(res.n_split_tcp)) == (7 * n, n)
        fb_x = sg.xlat46(x6, opts=XlatOpts.make(PREFIX))
        w = x6.verify_wire(checks=pbgpu.WIRE_ALL)
        assert (int(w.n_checked), int(w.n_bad), int(w.n_ipv6), int(w.n_nol4)) == (m, 0, m, 0)
        sg.encap(x6, mode=ENCAP_VXLAN, **VX)
        w = x6.verify_wire(checks=pbgpu.WIRE_ALL, vxlan_port=4789)
        assert (int(w.n_checked), int(w.n_bad), int(w.n_inner), int(w.n_nol4)) == (m, 0, m, 0)
    finally:
        x6.free()
        sg.free()
        fb.free()


# ------------------------------------------------------------------ 6. the empty range
def test_empty_range(ctx, mixed):
    fb, frames = mixed
    assert check_seg(ctx, fb, frames, 1460, first=5, n=0) == []
    assert check_seg(ctx, fb, frames, 8, first=3000, n=0) == []


# ------------------------------------------------------------------ 7. refusals
def _seg(ctx, src, dst, first, n, opts):
    return ctx.lib.pbgpu_segment(ctx.h, src, first, n, opts, dst, None)


def _sizes(ctx, src, first, n, opts):
    a, b = C.c_uint64(), C.c_uint64()
    return (ctx.lib.pbgpu_segment_size(ctx.h, src, first, n, opts, C.byref(a), C.byref(b)),
            ctx.lib.pbgpu_segment_bound(ctx.h, src, first, n, opts, C.byref(a), C.byref(b)))


def _state(ctx, dst, cap):
    return (int(dst.f.n_frames), int(dst.f.fixed_len), int(dst.f.total_bytes), dst.stream(cap).tobytes())


def test_refusals(ctx):
    frames = [sf.udp(2958, j) for j in range(100)]  # 3000 B: 3 segments each at mss 1460, 3084 B
    fb = uploaded(ctx, pack(frames)[0], flen=3000)
    never = ctx.alloc_frames(16, 1024)
    need = 3084 * 100
    dst, cap = fresh_dst(ctx, need, 300)
    state = _state(ctx, dst, cap)
    ok = SegOpts(1460, 0, 0)

    def refused(rc, src, first, n, opts, d=dst, sized=True):
        assert _seg(ctx, src, d.ptr if d is not None else None, first, n, opts) == rc
        if sized and rc == EINVAL:
            assert _sizes(ctx, src, first, n, opts) == (rc, rc)
        assert _state(ctx, dst, cap) == state

    try:
        # NULL arguments
        refused(EINVAL, None, 0, 100, C.byref(ok))
        refused(EINVAL, fb.ptr, 0, 100, None)
        refused(EINVAL, fb.ptr, 0, 100, C.byref(ok), d=None, sized=False)
        assert ctx.lib.pbgpu_segment(None, fb.ptr, 0, 100, C.byref(ok), dst.ptr, None) == EINVAL
        a = C.c_uint64()
        for fn in (ctx.lib.pbgpu_segment_size, ctx.lib.pbgpu_segment_bound):
            assert fn(ctx.h, fb.ptr, 0, 100, C.byref(ok), None, C.byref(a)) == EINVAL
            assert fn(ctx.h, fb.ptr, 0, 100, C.byref(ok), C.byref(a), None) == EINVAL
        # a source never built or uploaded
        refused(EINVAL, never.ptr, 0, 0, C.byref(ok))
        # a range past n_frames
        refused(EINVAL, fb.ptr, 1, 100, C.byref(ok))
        refused(EINVAL, fb.ptr, 101, 0, C.byref(ok))
        # src == dst, overlapping allocations
        assert _seg(ctx, fb.ptr, fb.ptr, 0, 1, C.byref(ok)) == EINVAL
        alias = pbgpu.Frames.from_buffer_copy(dst.f)
        alias.data = fb.f.data + 4096
        alias.capacity_bytes = 1024
        assert _seg(ctx, fb.ptr, C.byref(alias), 0, 1, C.byref(ok)) == EINVAL
        # mss, flags, reserved
        for bad in (SegOpts(7, 0, 0), SegOpts(0, 0, 0), SegOpts(65536, 0, 0), SegOpts(1460, 4, 0),
                    SegOpts(1460, 7, 0), SegOpts(1460, 0x80000000, 0), SegOpts(1460, 0, 1), SegOpts(1460, 0, 1 << 40)):
            refused(EINVAL, fb.ptr, 0, 100, C.byref(bad))
        # a source holding a frame below 14 B
        for tiny in (uploaded(ctx, np.zeros(13 * 8, dtype=np.uint8), flen=13),
                     uploaded(ctx, *pack([bytes(60), bytes(14), bytes(13), bytes(60)]))):
            try:
                refused(EINVAL, tiny.ptr, 0, 1, C.byref(ok))
            finally:
                tiny.free()
        # a destination too small: frames, bytes
        few = pbgpu.Frames.from_buffer_copy(dst.f)
        few.capacity_frames = 299
        assert _seg(ctx, fb.ptr, C.byref(few), 0, 100, C.byref(ok)) == ENOSPC
        short = pbgpu.Frames.from_buffer_copy(dst.f)
        assert need % 16 == 0
        short.capacity_bytes = need - 1
        assert _seg(ctx, fb.ptr, C.byref(short), 0, 100, C.byref(ok)) == ENOSPC
        short.capacity_bytes = 3084 * 99 + 11  # 99 frames give 305316 B: rounded up to 16, one more
        assert (3084 * 99) % 16 == 4
        assert _seg(ctx, fb.ptr, C.byref(short), 0, 99, C.byref(ok)) == ENOSPC
        assert _state(ctx, dst, cap) == state
        with pytest.raises(PbError) as e:
            small = ctx.alloc_frames(300, 1024)
            try:
                fb.segment(small)
            finally:
                small.free()
        assert e.value.code == ENOSPC
        short.capacity_bytes = need
        res = SegResult()
        assert ctx.lib.pbgpu_segment(ctx.h, fb.ptr, 0, 100, C.byref(ok), C.byref(short), C.byref(res)) == 0
        assert (res.n_in, res.n_out, res.n_split_tcp, res.n_split_udp, res.n_other, res.out_bytes, res.out_min_len,
                res.out_max_len) == (100, 300, 0, 100, 0, need, 42 + 38, 1502)
    finally:
        dst.free()
        never.free()
        fb.free()


# ------------------------------------------------------------------ 8. past 2^32 output bytes
def test_output_past_4_gib(ctx):
    """9043-B UDP frames built on the GPU at mss 1472: 9295 output bytes each, past byte 2^32 of the
    output.  pbgpu_verify over the whole output; the first and the last MiB and 384 KiB around byte
    2^32 against pyseg over the source's frames."""
    rec, L, mss = 9043 + 6 * 42, 9043, 1472
    n, first_iter = (1 << 32) // rec + 300, 1000
    seq = Sequence.from_config(pc.get("udp_jumbo_fixed_odd"))
    ctx.load_sequence(0, seq, pc.SEED_BASE)
    total = rec * n
    assert total > (1 << 32) + (1 << 20)
    try:
        fb = ctx.alloc_frames(*ctx.build_size(0, n))
    except PbError as e:
        pytest.skip("cannot allocate the 4.2-GB frame buffer: %s" % e)
    try:
        try:
            dst = ctx.alloc_frames(7 * n, total)
        except PbError as e:
            pytest.skip("cannot allocate the 4.3-GB output buffer: %s" % e)
        try:
            ctx.build(0, first_iter, n, fb)
            ctx.sync()
            assert int(fb.f.fixed_len) == L
            res = fb.segment(dst, mss=mss)
            assert (int(res.n_out), int(res.n_split_udp), int(res.out_bytes)) == (7 * n, n, total)
            assert (int(res.out_min_len), int(res.out_max_len)) == (42 + 9001 - 6 * mss, 42 + mss)
            assert (int(dst.f.n_frames), int(dst.f.fixed_len), int(dst.f.total_bytes)) == (7 * n, 0, total)
            v = dst.verify(checks=pbgpu.VERIFY_ALL)
            assert (int(v.n_checked), int(v.n_bad)) == (7 * n, 0)
            for a, win in (((1 << 32) - (192 << 10), 384 << 10), (total - (1 << 20), 1 << 20), (0, 1 << 20)):
                b = a + win
                j_lo, j_hi = a // rec, (b - 1) // rec
                src = fb.stream((j_hi - j_lo + 1) * L, j_lo * L).tobytes()
                ref = b"".join(b"".join(pyseg.segment(src[i:i + L], mss)) for i in range(0, len(src), L))
                assert dst.stream(win, a).tobytes() == ref[a - rec * j_lo:b - rec * j_lo], a
        finally:
            dst.free()
    finally:
        fb.free()


# ------------------------------------------------------------------ 9. one scratch under both calls
def _one_call(ctx, call, refs, cnt):
    """One fragment or segment call into a watched destination: every byte, the result, the offsets."""
    ref = b"".join(refs)
    total, r16 = len(ref), (len(ref) + 15) & ~15
    dst, cap = fresh_dst(ctx, total, len(refs))
    try:
        res = call(dst)
        assert {k: int(getattr(res, k)) for k in cnt} == cnt
        got = dst.stream(cap)
        assert np.array_equal(got[:total], np.frombuffer(ref, dtype=np.uint8))
        assert not got[total:r16].any() and (got[r16:] == 0xA5).all()
        assert (int(dst.f.n_frames), int(dst.f.fixed_len), int(dst.f.total_bytes)) == (len(refs), 0, total)
        want_off = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.uint64)
        assert np.array_equal(dst.offsets(), want_off)
    finally:
        dst.free()


def test_fragment_and_segment_share_their_scratch():
    """pbgpu_fragment and pbgpu_segment keep one count scratch, one map and one slice-sum buffer in
    the context, and lay the count scratch out differently (one row sum, or two).  On one fresh
    context a small segment call, a fragment call whose count takes two workgroups (4,200 frames:
    all three buffers grow), the first call again, then the two _size calls on the other kind's
    buffer and a small fragment call: each output whole against pyseg / pyfrag."""
    small = []
    for j in range(40):
        if j % 5 == 4:
            small.append(sf.payload(14 + j, j))
        elif j % 5 == 3:
            small.append(sf.tcp(700 + 37 * j, j, ident=j, seq=j * 977, flags=j, H=(20, 24, 60)[j % 3]))
        else:
            small.append(frame_of(("udp", "tcp")[j & 1], 60 + 83 * j, 500 + j))
    kinds = [frame_of(("udp", "tcp")[j & 1], 1621, 40 + j) for j in range(8)]
    large = [kinds[(j * 5 + j // 8) % 8] for j in range(4200)]
    assert len(large) > 16 * 256  # the count's rows per workgroup times its frames per row
    seg_small = pyseg.segment_all(small, 536, 0)
    frag_small = pyfrag.fragment_all(small, 576, True)
    frag_large = pyfrag.fragment_all(large, 576, True)
    seg_large, _ = pyseg.segment_all(large, 536, 0)
    assert frag_large[1]["n_split"] == 4200 and seg_small[1]["n_out"] > 40 and frag_small[1]["n_out"] > 40
    ctx = GpuContext(0)
    try:
        sd, so = pack(small)
        fs, fl = uploaded(ctx, sd, off=so), uploaded(ctx, pack(large)[0], flen=1621)
        try:
            _one_call(ctx, lambda d: fs.segment(d, 0, 40, 536), *seg_small)
            _one_call(ctx, lambda d: fl.fragment(d, 0, 4200, 576, True), *frag_large)
            _one_call(ctx, lambda d: fs.segment(d, 0, 40, 536), *seg_small)
            assert ctx.fragment_size(fs, 0, 40, 576, True) == (len(frag_small[0]), sum(map(len, frag_small[0])))
            assert ctx.segment_size(fl, 0, 4200, 536) == (len(seg_large), sum(map(len, seg_large)))
            _one_call(ctx, lambda d: fs.fragment(d, 0, 40, 576, True), *frag_small)
        finally:
            fs.free()
            fl.free()
    finally:
        ctx.close()
