"""pbgpu_encap on the GPU: every output byte against tests/pyencap.py, which writes the encapsulated
frames from their definition with `struct` and Python integers.

Every destination is first filled with 0xA5 by an upload, so a stray write shows, and is compared
whole: the frames, zeros up to the next multiple of 16, 0xA5 after that.  The destination's
metadata and device offsets are checked, and the source is compared with itself afterwards."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import pb_configs as pc
import pbgpu
import pyencap
import pypcap
from pbgpu import ENCAP_VLAN, ENCAP_VXLAN, EncapOpts, GpuContext, PbError, Sequence

pytestmark = pytest.mark.gpu

SLACK = 4096 + 64  # bytes of the destination past the frames, watched for stray writes
VX = dict(dst_mac=bytes.fromhex("0200000000a2"), src_mac=bytes.fromhex("0200000000a1"), src_ip=bytes([192, 0, 2, 1]),
          dst_ip=bytes([198, 51, 100, 2]), vni=0x123456)
MODES = {"vlan": (ENCAP_VLAN, dict(tci=0xA064)), "vxlan": (ENCAP_VXLAN, VX)}
P_OF = {ENCAP_VLAN: 4, ENCAP_VXLAN: 50}
EINVAL, ENOSPC = -22, -28


def ref_frame(frame, mode, fields):
    if mode == ENCAP_VLAN:
        return pyencap.vlan(frame, fields.get("tci", 0), fields.get("tpid", 0))
    return pyencap.vxlan(frame, **fields)


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


def fixed_frames(data, flen):
    return [bytes(data[i * flen:(i + 1) * flen]) for i in range(len(data) // flen)]


def lens_to_frames(lens, seed):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.uint64))]).astype(np.uint64)
    data = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    return data, off


def split(data, off):
    return [bytes(data[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def check_encap(ctx, fb, frames, mode, fields, first=0, n=None, keep=False):
    """Encapsulates fb's frames [first, first + n) and compares the whole destination; `frames` are
    the buffer's frames as bytes.  Returns the reference frames (and with keep the destination)."""
    n = len(frames) - first if n is None else n
    refs = [ref_frame(f, mode, fields) for f in frames[first:first + n]]
    ref = b"".join(refs)
    opts = EncapOpts.make(mode, **fields)
    assert ctx.encap_size(fb, first, n, opts) == (n, len(ref))
    before = fb.packed().copy()
    meta_before = (int(fb.f.n_frames), int(fb.f.fixed_len))
    dst, cap = fresh_dst(ctx, len(ref), n)
    try:
        ms = fb.encap(dst, first, n, opts=opts)
        assert ms >= 0
        got = dst.stream(cap)
        total = len(ref)
        r16 = (total + 15) & ~15
        want = np.frombuffer(ref, dtype=np.uint8)
        if not np.array_equal(got[:total], want):
            bad = int(np.nonzero(got[:total] != want)[0][0])
            raise AssertionError((bad, got[max(0, bad - 8):bad + 8].tobytes().hex(), ref[max(0, bad - 8):bad + 8].hex()))
        assert not got[total:r16].any()
        assert (got[r16:] == 0xA5).all()
        flen = int(fb.f.fixed_len)
        assert (int(dst.f.n_frames), int(dst.f.fixed_len), int(dst.f.total_bytes)) == \
            (n, flen + P_OF[mode] if flen else 0, total)
        if not flen and n:
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
    for name, (mode, _) in MODES.items():
        P = P_OF[mode]
        for L in (14, 15, 16, 17, 37, 38, 46, 60, 61, 64, 98, 1500, 4046, 4092):
            ns = {1, 2, 257}
            if L in (60, 64):  # either side of the first output page edge
                k = 4096 // (L + P)
                ns |= {k, k + 1} | ({k - 1} if 4096 % (L + P) == 0 else set())
            out += [(name, L, n) for n in sorted(ns)]
    return out + [("vxlan", 65485, 3), ("vlan", 65531, 3)]


@pytest.mark.parametrize("name,L,n", _fixed_cases())
def test_fixed_uploaded(ctx, name, L, n):
    mode, fields = MODES[name]
    data = np.random.default_rng(L).integers(0, 256, L * n, dtype=np.uint8)
    fb = uploaded(ctx, data, flen=L)
    try:
        check_encap(ctx, fb, fixed_frames(data, L), mode, fields)
    finally:
        fb.free()


# ------------------------------------------------------------------ 2. variable lengths, uploaded
def random3000_frames():
    """14..300 B with many 14-B frames: more records than one LDS window, up to 227 to a page."""
    rng = np.random.default_rng(99)
    lens = rng.integers(14, 301, 3000)
    lens[rng.random(3000) < 0.5] = 14
    lens[1000:1700] = 14
    return lens_to_frames(lens, 2)


@pytest.fixture(scope="module")
def random3000(ctx):
    data, off = random3000_frames()
    fb = uploaded(ctx, data, off=off)
    yield fb, split(data, off), off
    fb.free()


@pytest.mark.parametrize("name", list(MODES))
def test_variable_random_lengths(ctx, random3000, name):
    fb, frames, _ = random3000
    check_encap(ctx, fb, frames, *MODES[name])


VAR_CASES = {
    # a record end exactly on byte 4096, followed by more frames
    "vxlan_page_edge": ("vxlan", [206] * 16 + [14, 206, 33, 206]),
    "vlan_page_edge": ("vlan", [60] * 64 + [14, 60, 61, 62]),
    "vxlan_long_among_short": ("vxlan", [14, 20, 65485, 14, 15, 300, 14]),
    "vlan_long_among_short": ("vlan", [14, 20, 65531, 14, 15, 300, 14]),
    # the masked source-port hash: every length that ends inside bytes 26..37
    "vxlan_hash_masked": ("vxlan", list(range(14, 39)) * 3),
    "vlan_short": ("vlan", list(range(14, 39)) * 3),
}


@pytest.mark.parametrize("case", list(VAR_CASES))
def test_variable_cases(ctx, case):
    name, lens = VAR_CASES[case]
    data, off = lens_to_frames(lens, 7)
    if "page_edge" in case:
        P = P_OF[MODES[name][0]]
        k = 16 if name == "vxlan" else 64
        assert int(off[k]) + k * P == 4096
    fb = uploaded(ctx, data, off=off)
    try:
        check_encap(ctx, fb, split(data, off), *MODES[name])
    finally:
        fb.free()


# ------------------------------------------------------------------ 3. sub-ranges
@pytest.mark.parametrize("name", list(MODES))
def test_subrange_every_source_alignment(ctx, name):
    """61-B frames from first_frame 0..16: the range's first source byte at every alignment mod 16."""
    data = np.random.default_rng(5).integers(0, 256, 61 * 120, dtype=np.uint8)
    fb = uploaded(ctx, data, flen=61)
    frames = fixed_frames(data, 61)
    try:
        assert {(61 * f) % 16 for f in range(17)} == set(range(16))
        for first in range(17):
            check_encap(ctx, fb, frames, *MODES[name], first=first, n=90)
    finally:
        fb.free()


@pytest.mark.parametrize("name", list(MODES))
def test_subrange_variable(ctx, random3000, name):
    fb, frames, off = random3000
    for first in range(17):
        check_encap(ctx, fb, frames, *MODES[name], first=first, n=700)
    check_encap(ctx, fb, frames, *MODES[name], first=2999, n=1)
    check_encap(ctx, fb, frames, *MODES[name], first=900, n=1500)


# ------------------------------------------------------------------ 4. built on the GPU
@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("cfg", ["c2_udp_64", "c4_tcp_syn", "c5_icmp_echo", "c3_udp_var"])
def test_built_on_the_gpu(ctx, cfg, name):
    seq = Sequence.from_config(pc.get(cfg))
    ctx.load_sequence(0, seq, pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, 4096))
    try:
        ctx.build(0, 777, 4096, fb)
        ctx.sync()
        frames = fb.frames()
        assert len(frames) >= 4096
        check_encap(ctx, fb, frames, *MODES[name])
    finally:
        fb.free()


# ------------------------------------------------------------------ 5. fields
@pytest.fixture(scope="module")
def udp64(ctx):
    data, off = ob.build(Sequence.from_config(pc.get("c2_udp_64")), 0, 12345, 300, pc.SEED_BASE)
    fb = uploaded(ctx, data, flen=64)
    yield fb, split(data, off)
    fb.free()


@pytest.mark.parametrize("fields", [
    dict(VX, src_port=4242),
    dict(VX, src_port=65535, dst_port=8472, ttl=1, tos=0xB8),
    dict(VX, dst_port=1, ttl=255, tos=1, vni=0xFFFFFF),
    dict(VX, vni=0, src_ip=bytes([255, 255, 255, 255]), dst_ip=bytes([255, 255, 255, 255]), tos=255, ttl=255),
], ids=["sport", "all", "hashed", "checksum_carry"])
def test_vxlan_fields(ctx, udp64, random3000, fields):
    check_encap(ctx, udp64[0], udp64[1], ENCAP_VXLAN, fields)
    check_encap(ctx, random3000[0], random3000[1], ENCAP_VXLAN, fields, first=100, n=300)


@pytest.mark.parametrize("fields", [dict(tci=0x0FFF, tpid=0x88A8), dict(tci=0), dict(tci=0xFFFF, tpid=0x9100)])
def test_vlan_fields(ctx, udp64, random3000, fields):
    check_encap(ctx, udp64[0], udp64[1], ENCAP_VLAN, fields)
    check_encap(ctx, random3000[0], random3000[1], ENCAP_VLAN, fields, first=100, n=300)


# ------------------------------------------------------------------ 6. composition
@pytest.mark.parametrize("src", ["fixed", "variable"])
def test_composition(ctx, udp64, random3000, src):
    fb, frames = (udp64[0], udp64[1]) if src == "fixed" else (random3000[0], random3000[1][:1200])
    n = len(frames)
    refs, vx = check_encap(ctx, fb, frames, ENCAP_VXLAN, VX, n=n, keep=True)
    try:
        # the outer header is Ethernet + IPv4 + UDP
        res = vx.verify(checks=pbgpu.VERIFY_IP_CSUM | pbgpu.VERIFY_TOT_LEN)
        assert (int(res.n_checked), int(res.n_bad)) == (n, 0)
        assert vx.frames() == refs
        # landed in slots
        slot = 512
        umem = np.zeros(slot * n, dtype=np.uint8)
        lens = vx.to_umem(umem, slot, 0, n)
        assert [bytes(umem[i * slot:i * slot + int(lens[i])]) for i in range(n)] == refs
        # packed into a pcap stream
        assert vx.pcap_bytes(t0_ns=10**18, step_ps=6_720_000).tobytes() == pypcap.pcap_stream(refs, 10**18, 6_720_000)
        # encapsulated again
        check_encap(ctx, vx, refs, ENCAP_VLAN, dict(tci=0x2005))
    finally:
        vx.free()
    refs, vl = check_encap(ctx, fb, frames, ENCAP_VLAN, dict(tci=100), n=n, keep=True)
    try:
        check_encap(ctx, vl, refs, ENCAP_VLAN, dict(tci=200, tpid=0x88A8))
        lens = vl.to_umem(umem, slot, 0, n)
        assert [bytes(umem[i * slot:i * slot + int(lens[i])]) for i in range(n)] == refs
    finally:
        vl.free()


# ------------------------------------------------------------------ 7. the empty range
@pytest.mark.parametrize("name", list(MODES))
def test_empty_range(ctx, udp64, random3000, name):
    for fb, frames, first in ((udp64[0], udp64[1], 0), (udp64[0], udp64[1], 300), (random3000[0], random3000[1], 5)):
        assert check_encap(ctx, fb, frames, *MODES[name], first=first, n=0) == []


# ------------------------------------------------------------------ 8. refusals
def _encap(ctx, src, dst, first, n, opts):
    return ctx.lib.pbgpu_encap(ctx.h, src, first, n, opts, dst, None)


def _size(ctx, src, first, n, opts):
    a, b = C.c_uint64(), C.c_uint64()
    return ctx.lib.pbgpu_encap_size(ctx.h, src, first, n, opts, C.byref(a), C.byref(b))


def _state(ctx, dst, cap):
    return (int(dst.f.n_frames), int(dst.f.fixed_len), int(dst.f.total_bytes), dst.stream(cap).tobytes())


def test_refusals(ctx, udp64):
    fb, _ = udp64  # 300 frames of 64 B
    never = ctx.alloc_frames(16, 1024)
    dst, cap = fresh_dst(ctx, 114 * 300, 300)
    state = _state(ctx, dst, cap)
    ok = EncapOpts.make(ENCAP_VXLAN, **VX)
    okv = EncapOpts.make(ENCAP_VLAN, tci=5)

    def refused(rc, src, first, n, opts, d=dst, sized=True):
        assert _encap(ctx, src, d.ptr if d is not None else None, first, n, opts) == rc
        if sized and rc == EINVAL:
            assert _size(ctx, src, first, n, opts) == rc
        assert _state(ctx, dst, cap) == state

    try:
        # NULL arguments
        refused(EINVAL, None, 0, 300, C.byref(ok))
        refused(EINVAL, fb.ptr, 0, 300, None)
        refused(EINVAL, fb.ptr, 0, 300, C.byref(ok), d=None, sized=False)
        assert ctx.lib.pbgpu_encap(None, fb.ptr, 0, 300, C.byref(ok), dst.ptr, None) == EINVAL
        a = C.c_uint64()
        assert ctx.lib.pbgpu_encap_size(ctx.h, fb.ptr, 0, 300, C.byref(ok), None, C.byref(a)) == EINVAL
        assert ctx.lib.pbgpu_encap_size(ctx.h, fb.ptr, 0, 300, C.byref(ok), C.byref(a), None) == EINVAL
        # a source never built or uploaded
        refused(EINVAL, never.ptr, 0, 0, C.byref(ok))
        # a range past n_frames
        refused(EINVAL, fb.ptr, 1, 300, C.byref(ok))
        refused(EINVAL, fb.ptr, 301, 0, C.byref(okv))
        # src == dst, overlapping allocations
        assert _encap(ctx, fb.ptr, fb.ptr, 0, 1, C.byref(ok)) == EINVAL
        alias = pbgpu.Frames.from_buffer_copy(dst.f)
        alias.data = fb.f.data + 4096
        alias.capacity_bytes = 1024
        assert _encap(ctx, fb.ptr, C.byref(alias), 0, 1, C.byref(ok)) == EINVAL
        # unknown mode, flags, reserved, vni
        for bad in (dict(mode=0), dict(mode=3), dict(flags=1), dict(reserved=1), dict(vni=1 << 24)):
            o = EncapOpts.make(ENCAP_VXLAN, **VX)
            for k, v in bad.items():
                setattr(o, k, v)
            refused(EINVAL, fb.ptr, 0, 300, C.byref(o))
        o = EncapOpts.make(ENCAP_VLAN, tci=1, flags=2)
        refused(EINVAL, fb.ptr, 0, 300, C.byref(o))
        # a destination too small: frames, bytes
        few = pbgpu.Frames.from_buffer_copy(dst.f)
        few.capacity_frames = 299
        assert _encap(ctx, fb.ptr, C.byref(few), 0, 300, C.byref(ok)) == ENOSPC
        short = pbgpu.Frames.from_buffer_copy(dst.f)
        need = 114 * 300  # 34200, 8 mod 16
        short.capacity_bytes = ((need + 15) & ~15) - 1
        assert _encap(ctx, fb.ptr, C.byref(short), 0, 300, C.byref(ok)) == ENOSPC
        assert _state(ctx, dst, cap) == state
        with pytest.raises(PbError) as e:
            small = ctx.alloc_frames(300, 1024)
            try:
                fb.encap(small, mode=ENCAP_VXLAN, **VX)
            finally:
                small.free()
        assert e.value.code == ENOSPC
        short.capacity_bytes = (need + 15) & ~15
        assert _encap(ctx, fb.ptr, C.byref(short), 0, 300, C.byref(ok)) == 0
    finally:
        dst.free()
        never.free()


@pytest.mark.parametrize("name", list(MODES))
def test_refused_frame_lengths(ctx, name):
    """A 13-B fixed upload, an upload holding one 13-B frame, a frame one byte too long."""
    mode, fields = MODES[name]
    opts = EncapOpts.make(mode, **fields)
    too_long = 65535 - P_OF[mode] + 1
    dst, cap = fresh_dst(ctx, 3 * 65536, 64)
    state = _state(ctx, dst, cap)
    cases = [
        uploaded(ctx, np.zeros(13 * 8, dtype=np.uint8), flen=13),
        uploaded(ctx, *lens_to_frames([60, 14, 13, 60], 3)),
        uploaded(ctx, np.zeros(too_long * 2, dtype=np.uint8), flen=too_long),
        uploaded(ctx, *lens_to_frames([60, too_long, 60], 3)),
    ]
    try:
        for fb in cases:
            n = int(fb.f.n_frames)
            assert _encap(ctx, fb.ptr, dst.ptr, 0, n, C.byref(opts)) == EINVAL
            assert _encap(ctx, fb.ptr, dst.ptr, 0, 1, C.byref(opts)) == EINVAL  # the buffer's frames, not the range's
            assert _size(ctx, fb.ptr, 0, n, C.byref(opts)) == EINVAL
            assert _state(ctx, dst, cap) == state
        # the longest frame that fits does
        fits = uploaded(ctx, *lens_to_frames([14, too_long - 1], 4))
        try:
            assert _encap(ctx, fits.ptr, dst.ptr, 0, 2, C.byref(opts)) == 0
        finally:
            fits.free()
    finally:
        for fb in cases:
            fb.free()
        dst.free()


# ------------------------------------------------------------------ 9. past 2^32 output bytes
def test_output_past_4_gib(ctx):
    """1500-B frames built on the GPU, VXLAN, 1550-B records past byte 2^32 of the output; a window
    of 384 KiB around byte 2^32 and the last 64 KiB against the oracle's frames for those iterations."""
    rec = 1550
    n, first_iter = (1 << 32) // rec + 2000, 1000
    seq = Sequence.from_config(pc.get("c2_udp_1500"))
    ctx.load_sequence(0, seq, pc.SEED_BASE)
    total = rec * n
    assert total > (1 << 32) + (1 << 20)
    try:
        fb = ctx.alloc_frames(*ctx.build_size(0, n))
    except PbError as e:
        pytest.skip("cannot allocate the 4.2-GB frame buffer: %s" % e)
    try:
        try:
            dst = ctx.alloc_frames(n, total)
        except PbError as e:
            pytest.skip("cannot allocate the 4.3-GB output buffer: %s" % e)
        try:
            ctx.build(0, first_iter, n, fb)
            ctx.sync()
            assert int(fb.f.fixed_len) == 1500
            fb.encap(dst, mode=ENCAP_VXLAN, **VX)
            assert (int(dst.f.n_frames), int(dst.f.fixed_len), int(dst.f.total_bytes)) == (n, rec, total)
            for a, win in (((1 << 32) - (192 << 10), 384 << 10), (total - (64 << 10), 64 << 10), (0, 64 << 10)):
                b = a + win
                j_lo, j_hi = a // rec, (b - 1) // rec
                data, off = ob.build(seq, 0, first_iter + j_lo, j_hi - j_lo + 1, pc.SEED_BASE)
                ref = b"".join(pyencap.vxlan(f, **VX) for f in split(data, off))
                assert dst.stream(win, a).tobytes() == ref[a - rec * j_lo:b - rec * j_lo], a
        finally:
            dst.free()
    finally:
        fb.free()
