"""pbgpu_fragment on the GPU: every output byte and every field of the result against tests/pyfrag.py,
which writes the fragments from their definition with `struct` and Python integers.

Every destination is first filled with 0xA5 by an upload, so a stray write shows, and is compared
whole: the frames, zeros up to the next multiple of 16, 0xA5 after that.  The destination's
metadata and device offsets are checked, and the source is compared with itself afterwards."""
import ctypes as C
import struct

import numpy as np
import pytest

import pb_configs as pc
import pbgpu
import pyfrag
import pypcap
import pyverify
from pbgpu import ENCAP_VXLAN, FragOpts, FragResult, GpuContext, PbError, Sequence

pytestmark = pytest.mark.gpu

SLACK = 4096 + 64  # bytes of the destination past the frames, watched for stray writes
EINVAL, ENOSPC = -22, -28
VX = dict(dst_mac=bytes.fromhex("0200000000a2"), src_mac=bytes.fromhex("0200000000a1"), src_ip=bytes([192, 0, 2, 1]),
          dst_ip=bytes([198, 51, 100, 2]), vni=0x123456)


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


def ip_frame(L, seed, fo=0, ethertype=b"\x08\x00", vihl=0x45):
    """L random bytes; from 34 B on with an Ethernet + IPv4 header whose tot_len and checksum hold."""
    f = bytearray(np.random.default_rng(seed).integers(0, 256, L, dtype=np.uint8).tobytes())
    if L >= 34:
        f[12:14] = ethertype
        f[14:34] = struct.pack("!BBHHHBBH", vihl, seed & 0xFF, L - 14, seed & 0xFFFF, fo, 64, 17, 0) + bytes(f[26:34])
        f[24:26] = struct.pack("!H", pyverify.ip_csum_value(bytes(f)))
    return bytes(f)


def pack(frames):
    off = np.concatenate([[0], np.cumsum([len(f) for f in frames], dtype=np.uint64)]).astype(np.uint64)
    return np.frombuffer(b"".join(frames), dtype=np.uint8), off


def check_frag(ctx, fb, frames, mtu, ignore_df=False, first=0, n=None, keep=False):
    """Fragments fb's frames [first, first + n) and compares the whole destination and the result;
    `frames` are the buffer's frames as bytes.  Returns the reference frames (and with keep the
    destination)."""
    n = len(frames) - first if n is None else n
    refs, cnt = pyfrag.fragment_all(frames[first:first + n], mtu, ignore_df)
    ref = b"".join(refs)
    total = len(ref)
    assert ctx.fragment_size(fb, first, n, mtu, ignore_df) == (len(refs), total)
    bf, bb = ctx.fragment_bound(fb, first, n, mtu, ignore_df)
    assert bf >= len(refs) and bb >= total
    before = fb.packed().copy()
    meta_before = (int(fb.f.n_frames), int(fb.f.fixed_len))
    dst, cap = fresh_dst(ctx, total, len(refs))
    try:
        res = fb.fragment(dst, first, n, mtu, ignore_df)
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
        keeps = flen and flen - 14 <= mtu and n
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


# ------------------------------------------------------------------ 1. fixed lengths, uploaded
def _fixed_cases():
    out = []
    for mtu in (68, 576, 1500):
        c = (mtu - 20) & ~7
        for L in (14, 34, 35, mtu + 13, mtu + 14, mtu + 15, 34 + c, 34 + c + 1, 34 + 2 * c, 9043, 65535):
            k = 1 if L - 14 <= mtu else -(-(L - 34) // c)
            rec = L + 34 * (k - 1)  # output bytes per source frame
            ns = {1}
            if rec <= 4096:  # records ending one before, on and one after output byte 4096
                ns |= {max(1, 4096 // rec - 1), 4096 // rec, 4096 // rec + 1, 4096 // rec + 2}
            else:
                ns |= {2, 3}
            out += [(mtu, L, n) for n in sorted(ns - {0})]
    return out


@pytest.mark.parametrize("mtu,L,n", _fixed_cases())
def test_fixed_uploaded(ctx, mtu, L, n):
    frames = [ip_frame(L, 1000 * L + j) for j in range(n)]
    data, _ = pack(frames)
    fb = uploaded(ctx, data, flen=L)
    try:
        check_frag(ctx, fb, frames, mtu)
    finally:
        fb.free()


# ------------------------------------------------------------------ 2. variable lengths, uploaded
def _mixed_frames():
    rng = np.random.default_rng(11)
    frames = []
    for j in range(3000):
        u = rng.random()
        if 1000 <= j < 1700 or u < 0.35:
            frames.append(ip_frame(14, j))  # runs of 14-B frames: 293 records to a page
        elif u < 0.55:
            frames.append(ip_frame(60, j))
        elif u < 0.70:
            frames.append(ip_frame(1514, j))
        elif u < 0.85:
            frames.append(ip_frame(1515, j))
        elif u < 0.90:
            frames.append(ip_frame(9043, j))
        elif u < 0.93:
            frames.append(ip_frame(int(rng.integers(1515, 4000)), j, fo=0x4000))  # DF
        elif u < 0.95:
            frames.append(ip_frame(1600, j, ethertype=b"\x86\xdd"))
        elif u < 0.97:
            frames.append(ip_frame(1600, j, vihl=0x46))
        elif u < 0.99:
            frames.append(ip_frame(int(rng.integers(1515, 4000)), j, fo=0x2000 | int(rng.integers(1, 4000))))
        else:
            frames.append(ip_frame(int(rng.integers(15, 1700)), j))
    frames[500] = ip_frame(65535, 500)
    frames[2500] = ip_frame(1549, 2500)  # a last fragment of one data byte
    frames[2501] = ip_frame(14, 2501)
    frames[2502] = ip_frame(1515, 2502)
    return frames


@pytest.fixture(scope="module")
def mixed(ctx):
    frames = _mixed_frames()
    data, off = pack(frames)
    fb = uploaded(ctx, data, off=off)
    yield fb, frames
    fb.free()


@pytest.mark.parametrize("ignore_df", [False, True])
@pytest.mark.parametrize("mtu", [1500, 576])
def test_variable_mixed(ctx, mixed, mtu, ignore_df):
    fb, frames = mixed
    check_frag(ctx, fb, frames, mtu, ignore_df)


def test_one_frame_into_1365_records(ctx):
    """A 65535-B frame at mtu 68 among short ones: 1365 records from one source."""
    frames = [ip_frame(L, 40 + j) for j, L in enumerate([14, 60, 14, 65535, 14, 83, 82, 14, 35, 130])]
    data, off = pack(frames)
    fb = uploaded(ctx, data, off=off)
    try:
        refs = check_frag(ctx, fb, frames, 68)
        assert len(refs) == 5 + 1365 + 2 + 1 + 1 + 2
    finally:
        fb.free()


# ------------------------------------------------------------------ 3. sub-ranges
def test_subrange_every_source_alignment(ctx, mixed):
    """1621-B frames from first_frame 0..16: the range's first source byte at every alignment mod 16."""
    frames = [ip_frame(1621, 7000 + j) for j in range(40)]
    data, _ = pack(frames)
    fb = uploaded(ctx, data, flen=1621)
    try:
        assert {(1621 * f) % 16 for f in range(17)} == set(range(16))
        for first in range(17):
            check_frag(ctx, fb, frames, 576, first=first, n=20)
    finally:
        fb.free()
    fb, frames = mixed
    for first in range(990, 1007):
        check_frag(ctx, fb, frames, 1500, first=first, n=800)
    check_frag(ctx, fb, frames, 1500, first=2999, n=1)
    check_frag(ctx, fb, frames, 68, first=495, n=10)


# ------------------------------------------------------------------ 4. built on the GPU
@pytest.mark.parametrize("cfg,mtu,n_iter", [("udp_jumbo_fixed_odd", 1500, 300), ("udp_jumbo_var", 1500, 300),
                                            ("c3_udp_var", 576, 4096), ("c2_udp_64", 1500, 4096)])
def test_built_on_the_gpu(ctx, cfg, mtu, n_iter):
    seq = Sequence.from_config(pc.get(cfg))
    ctx.load_sequence(0, seq, pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n_iter))
    try:
        ctx.build(0, 777, n_iter, fb)
        ctx.sync()
        frames = fb.frames()
        assert len(frames) >= n_iter
        refs, dst = check_frag(ctx, fb, frames, mtu, keep=True)
        try:
            if cfg == "c2_udp_64":
                assert int(dst.f.fixed_len) == 64 and refs == frames
            else:
                assert len(refs) > len(frames)
            res = dst.verify(checks=pbgpu.VERIFY_IP_CSUM | pbgpu.VERIFY_TOT_LEN)
            assert (int(res.n_checked), int(res.n_bad)) == (len(refs), 0)
        finally:
            dst.free()
    finally:
        fb.free()


# ------------------------------------------------------------------ 5. composition
def test_composition(ctx, mixed):
    fb, frames = mixed
    n = 900
    refs, fr = check_frag(ctx, fb, frames, 1500, ignore_df=True, first=1650, n=n, keep=True)
    try:
        assert fr.frames() == refs
        # landed in 4-KiB slots: the longest frame left is a copied 1600-B one
        m, slot = len(refs), 4096
        umem = np.zeros(slot * m, dtype=np.uint8)
        lens = fr.to_umem(umem, slot, 0, m)
        assert [bytes(umem[i * slot:i * slot + int(lens[i])]) for i in range(m)] == refs
        # packed into a pcap stream
        assert fr.pcap_bytes(t0_ns=10**18, step_ps=6_720_000).tobytes() == pypcap.pcap_stream(refs, 10**18, 6_720_000)
        # fragmented again at a smaller mtu
        check_frag(ctx, fr, refs, 576)
        # encapsulated, then fragmented again: the outer packet is the one that is split
        import pyencap
        vx_refs = [pyencap.vxlan(f, **VX) for f in refs]
        vx = ctx.alloc_frames(m, sum(len(f) for f in vx_refs) + 16)
        try:
            fr.encap(vx, mode=ENCAP_VXLAN, **VX)
            assert vx.frames() == vx_refs
            check_frag(ctx, vx, vx_refs, 576, ignore_df=True)
        finally:
            vx.free()
    finally:
        fr.free()


# ------------------------------------------------------------------ 6. the empty range
def test_empty_range(ctx, mixed):
    fb, frames = mixed
    assert check_frag(ctx, fb, frames, 1500, first=5, n=0) == []
    assert check_frag(ctx, fb, frames, 68, first=3000, n=0) == []


# ------------------------------------------------------------------ 7. refusals
def _frag(ctx, src, dst, first, n, opts):
    return ctx.lib.pbgpu_fragment(ctx.h, src, first, n, opts, dst, None)


def _sizes(ctx, src, first, n, opts):
    a, b = C.c_uint64(), C.c_uint64()
    return (ctx.lib.pbgpu_fragment_size(ctx.h, src, first, n, opts, C.byref(a), C.byref(b)),
            ctx.lib.pbgpu_fragment_bound(ctx.h, src, first, n, opts, C.byref(a), C.byref(b)))


def _state(ctx, dst, cap):
    return (int(dst.f.n_frames), int(dst.f.fixed_len), int(dst.f.total_bytes), dst.stream(cap).tobytes())


def test_refusals(ctx):
    frames = [ip_frame(3000, j) for j in range(100)]  # 3 fragments each at mtu 1500: 3068 B
    fb = uploaded(ctx, pack(frames)[0], flen=3000)
    never = ctx.alloc_frames(16, 1024)
    need = 3068 * 100
    dst, cap = fresh_dst(ctx, need, 300)
    state = _state(ctx, dst, cap)
    ok = FragOpts(1500, 0, 0)

    def refused(rc, src, first, n, opts, d=dst, sized=True):
        assert _frag(ctx, src, d.ptr if d is not None else None, first, n, opts) == rc
        if sized and rc == EINVAL:
            assert _sizes(ctx, src, first, n, opts) == (rc, rc)
        assert _state(ctx, dst, cap) == state

    try:
        # NULL arguments
        refused(EINVAL, None, 0, 100, C.byref(ok))
        refused(EINVAL, fb.ptr, 0, 100, None)
        refused(EINVAL, fb.ptr, 0, 100, C.byref(ok), d=None, sized=False)
        assert ctx.lib.pbgpu_fragment(None, fb.ptr, 0, 100, C.byref(ok), dst.ptr, None) == EINVAL
        a = C.c_uint64()
        for fn in (ctx.lib.pbgpu_fragment_size, ctx.lib.pbgpu_fragment_bound):
            assert fn(ctx.h, fb.ptr, 0, 100, C.byref(ok), None, C.byref(a)) == EINVAL
            assert fn(ctx.h, fb.ptr, 0, 100, C.byref(ok), C.byref(a), None) == EINVAL
        # a source never built or uploaded
        refused(EINVAL, never.ptr, 0, 0, C.byref(ok))
        # a range past n_frames
        refused(EINVAL, fb.ptr, 1, 100, C.byref(ok))
        refused(EINVAL, fb.ptr, 101, 0, C.byref(ok))
        # src == dst, overlapping allocations
        assert _frag(ctx, fb.ptr, fb.ptr, 0, 1, C.byref(ok)) == EINVAL
        alias = pbgpu.Frames.from_buffer_copy(dst.f)
        alias.data = fb.f.data + 4096
        alias.capacity_bytes = 1024
        assert _frag(ctx, fb.ptr, C.byref(alias), 0, 1, C.byref(ok)) == EINVAL
        # mtu, flags, reserved
        for bad in (FragOpts(67, 0, 0), FragOpts(0, 0, 0), FragOpts(65536, 0, 0), FragOpts(1500, 2, 0),
                    FragOpts(1500, 3, 0), FragOpts(1500, 0, 1), FragOpts(1500, 0, 1 << 40)):
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
        assert _frag(ctx, fb.ptr, C.byref(few), 0, 100, C.byref(ok)) == ENOSPC
        short = pbgpu.Frames.from_buffer_copy(dst.f)
        assert need % 16 == 0
        short.capacity_bytes = need - 1
        assert _frag(ctx, fb.ptr, C.byref(short), 0, 100, C.byref(ok)) == ENOSPC
        short.capacity_bytes = 303743  # 99 frames give 303732 B: rounded up to 16, one more
        assert _frag(ctx, fb.ptr, C.byref(short), 0, 99, C.byref(ok)) == ENOSPC
        assert _state(ctx, dst, cap) == state
        with pytest.raises(PbError) as e:
            small = ctx.alloc_frames(300, 1024)
            try:
                fb.fragment(small)
            finally:
                small.free()
        assert e.value.code == ENOSPC
        short.capacity_bytes = need
        res = FragResult()
        assert ctx.lib.pbgpu_fragment(ctx.h, fb.ptr, 0, 100, C.byref(ok), C.byref(short), C.byref(res)) == 0
        assert (res.n_in, res.n_out, res.n_split, res.out_bytes, res.out_min_len, res.out_max_len) == \
            (100, 300, 100, need, 40, 1514)
    finally:
        dst.free()
        never.free()
        fb.free()


# ------------------------------------------------------------------ 8. past 2^32 output bytes
def test_output_past_4_gib(ctx):
    """9043-B frames built on the GPU at mtu 1500: 9247 output bytes each, past byte 2^32 of the output;
    384 KiB around byte 2^32, the first and the last 64 KiB against pyfrag over the source's frames."""
    rec, L = 9247, 9043
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
            res = fb.fragment(dst, mtu=1500)
            assert (int(res.n_out), int(res.n_split), int(res.out_bytes)) == (7 * n, n, total)
            assert (int(dst.f.n_frames), int(dst.f.fixed_len), int(dst.f.total_bytes)) == (7 * n, 0, total)
            for a, win in (((1 << 32) - (192 << 10), 384 << 10), (total - (64 << 10), 64 << 10), (0, 64 << 10)):
                b = a + win
                j_lo, j_hi = a // rec, (b - 1) // rec
                src = fb.stream((j_hi - j_lo + 1) * L, j_lo * L).tobytes()
                ref = b"".join(b"".join(pyfrag.fragment(src[i:i + L], 1500)) for i in range(0, len(src), L))
                assert dst.stream(win, a).tobytes() == ref[a - rec * j_lo:b - rec * j_lo], a
        finally:
            dst.free()
    finally:
        fb.free()
