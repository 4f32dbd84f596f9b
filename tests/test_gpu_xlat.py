"""pbgpu_xlat46 on the GPU: every output byte against tests/pyxlat.py, which writes the translated
frames from their definition with `struct` and Python integers, and every output frame through
pyxlat's from-scratch IPv6 checksum checker.

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
import pyland
import pypcap
import pyxlat
from pbgpu import ENCAP_VLAN, ENCAP_VXLAN, EncapOpts, GpuContext, PbError, Sequence, XlatOpts, XlatResult

pytestmark = pytest.mark.gpu

SLACK = 4096 + 64  # bytes of the destination past the frames, watched for stray writes
EINVAL, ENOSPC = -22, -28
NONE = 2**64 - 1
PFX = {
    "carry": pyxlat.prefix96("2001:db8:ffff:ffff:ffff:ffff::/96"),
    "zero": pyxlat.prefix96("::/96"),
    "neutral": pyxlat.prefix96("64:ff9b::/96"),
}
DSTP = pyxlat.prefix96("2001:db8:1:2:3:4::/96")
VX = dict(dst_mac=bytes.fromhex("0200000000a2"), src_mac=bytes.fromhex("0200000000a1"), src_ip=bytes([192, 0, 2, 1]),
          dst_ip=bytes([198, 51, 100, 2]), vni=0x123456)
# the option sets the cases run under: (src_prefix, dst_prefix, flow_label, hash_flow)
OPTS = {
    "label": (PFX["carry"], DSTP, 0xABCDE, False),
    "hash": (PFX["neutral"], None, 0, True),
}


def mkopts(o):
    return XlatOpts.make(o[0], o[1], flow_label=o[2], hash_flow=o[3])


def ref_frames(frames, o):
    return [pyxlat.xlat46(f, o[0], o[1], flow_label=o[2], hash_flow=o[3]) for f in frames]


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


def upload_frames(ctx, frames, fixed=False):
    data = np.frombuffer(b"".join(frames), dtype=np.uint8)
    if fixed:
        return uploaded(ctx, data, flen=len(frames[0]))
    off = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.uint64)
    return uploaded(ctx, data, off=off)


def fresh_dst(ctx, nbytes, frames=0):
    """A destination of nbytes rounded up to 16 plus SLACK, every byte 0xA5."""
    cap = ((nbytes + 15) & ~15) + SLACK
    dst = ctx.alloc_frames(max(cap // 16, frames), cap)
    dst.upload(np.full(cap, 0xA5, dtype=np.uint8), fixed_len=16)
    return dst, cap


def check_xlat(ctx, fb, frames, o, first=0, n=None, keep=False, scratch=True):
    """Translates fb's frames [first, first + n) and compares the whole destination; `frames` are
    the buffer's frames as bytes.  Returns the reference frames (and with keep the destination)."""
    n = len(frames) - first if n is None else n
    refs = ref_frames(frames[first:first + n], o)
    assert None not in refs
    ref = b"".join(refs)
    opts = mkopts(o)
    assert ctx.xlat46_size(fb, first, n, opts) == (n, len(ref))
    before = fb.packed().copy()
    meta_before = (int(fb.f.n_frames), int(fb.f.fixed_len))
    dst, cap = fresh_dst(ctx, len(ref), n)
    try:
        res = fb.xlat46(dst, first, n, opts)
        kinds = [pyxlat.classify(f) for f in frames[first:first + n]]
        assert (int(res.n_in), int(res.n_udp), int(res.n_tcp), int(res.n_icmp), int(res.n_other), int(res.first_other)) == \
            (n, kinds.count("udp"), kinds.count("tcp"), kinds.count("icmp"), 0, NONE)
        assert res.device_ms >= 0
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
        assert (int(dst.f.n_frames), int(dst.f.fixed_len), int(dst.f.total_bytes)) == (n, flen + 20 if flen else 0, total)
        if not flen and n:
            want_off = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.uint64)
            assert np.array_equal(dst.offsets(), want_off)
        assert (int(fb.f.n_frames), int(fb.f.fixed_len)) == meta_before and np.array_equal(fb.packed(), before)
        if scratch:
            assert all(pyxlat.check6(r) for r in refs)
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
    for kind, lens in (("udp", (42, 43, 44, 45, 57, 58, 60, 61, 64, 98, 1500, 4076, 4077)), ("tcp", (54, 55, 60, 74)),
                       ("icmp", (42, 43, 98))):
        for L in lens:
            ns = {1, 2, 257}
            if L in (42, 60, 64):  # either side of the first output page edge
                k = 4096 // (L + 20)
                ns |= {k - 1, k, k + 1}
            out += [(kind, L, n) for n in sorted(ns)]
    return out


@pytest.mark.parametrize("kind,L,n", _fixed_cases())
def test_fixed_uploaded(ctx, kind, L, n):
    rng = np.random.default_rng(L * 1000 + n)
    frames = [pyxlat.frame4(kind, L, rng, icmp_type=8 * (i & 1)) for i in range(n)]
    fb = upload_frames(ctx, frames, fixed=True)
    try:
        check_xlat(ctx, fb, frames, OPTS["label" if n & 1 else "hash"])
    finally:
        fb.free()


# ------------------------------------------------------------------ 2. variable lengths, uploaded
def mixed_frames(lens, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i, L in enumerate(lens):
        kind = ("udp", "tcp", "icmp")[int(rng.integers(0, 3))]
        if kind == "tcp" and L < 54:
            kind = "udp"
        out.append(pyxlat.frame4(kind, int(L), rng, icmp_type=8 * (i & 1)))
    return out


def mixed1000_frames():
    """1,000 frames of mixed protocols, 42..1600 B: more records than one LDS window."""
    lens = np.random.default_rng(99).integers(42, 1601, 1000)
    return mixed_frames(lens, 2)


@pytest.fixture(scope="module")
def mixed1000(ctx):
    frames = mixed1000_frames()
    fb = upload_frames(ctx, frames)
    yield fb, frames
    fb.free()


@pytest.mark.parametrize("oname", list(OPTS))
def test_variable_mixed(ctx, mixed1000, oname):
    fb, frames = mixed1000
    check_xlat(ctx, fb, frames, OPTS[oname])


VAR_CASES = {
    "all_42": [42] * 300,  # 62-B records: the most a page can hold
    "long_among_short": [42, 54, 65515, 42, 43, 300, 42],
    # a record end exactly on byte 4096 (65 records of 62 B and one of 66), followed by more
    "page_edge": [42] * 65 + [46, 42, 43, 44, 42],
}


@pytest.mark.parametrize("case", list(VAR_CASES))
def test_variable_cases(ctx, case):
    lens = VAR_CASES[case]
    if case == "page_edge":
        assert sum(L + 20 for L in lens[:66]) == 4096
    frames = mixed_frames(lens, 7)
    fb = upload_frames(ctx, frames)
    try:
        check_xlat(ctx, fb, frames, OPTS["label"])
        check_xlat(ctx, fb, frames, OPTS["hash"])
    finally:
        fb.free()


# ------------------------------------------------------------------ 3. sub-ranges
def test_subrange_every_source_alignment(ctx):
    """61-B frames from first_frame 0..16: the range's first source byte at every alignment mod 16,
    1, 2 and 3 mod 4 among them."""
    rng = np.random.default_rng(5)
    frames = [pyxlat.frame4(("udp", "tcp", "icmp")[i % 3], 61, rng) for i in range(120)]
    fb = upload_frames(ctx, frames, fixed=True)
    try:
        assert {(61 * f) % 4 for f in range(1, 4)} == {1, 2, 3}
        for first in range(17):
            check_xlat(ctx, fb, frames, OPTS["label"], first=first, n=90, scratch=False)
    finally:
        fb.free()


def test_subrange_variable(ctx, mixed1000):
    fb, frames = mixed1000
    off = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
    firsts = [next(i for i in range(1, 1000) if off[i] % 4 == m) for m in (1, 2, 3)]
    for first in firsts + [0, 7]:
        check_xlat(ctx, fb, frames, OPTS["hash"], first=first, n=400, scratch=False)
    check_xlat(ctx, fb, frames, OPTS["label"], first=999, n=1)
    check_xlat(ctx, fb, frames, OPTS["label"], first=300, n=700, scratch=False)


def test_empty_range(ctx, mixed1000):
    fb, frames = mixed1000
    for first in (0, 5, 1000):
        assert check_xlat(ctx, fb, frames, OPTS["label"], first=first, n=0) == []


# ------------------------------------------------------------------ 4. built on the GPU
@pytest.mark.parametrize("oname", list(OPTS))
@pytest.mark.parametrize("cfg", ["c2_udp_64", "c3_udp_var", "c4_tcp_syn", "c5_icmp_echo"])
def test_built_on_the_gpu(ctx, cfg, oname):
    """The output equals pyxlat of the oracle's frames, and every output frame checks good from scratch."""
    seq = Sequence.from_config(pc.get(cfg))
    n = 2048
    ctx.load_sequence(0, seq, pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n))
    try:
        ctx.build(0, 777, n, fb)
        ctx.sync()
        data, off = ob.build(seq, 0, 777, n, pc.SEED_BASE)
        frames = [bytes(data[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]
        assert len(frames) >= n
        check_xlat(ctx, fb, frames, OPTS[oname])
    finally:
        fb.free()


# ------------------------------------------------------------------ 5. checksum corners
def corner_frames(prefix):
    """UDP and TCP frames whose stored checksum makes the translated one 0x0000 (UDP: stored as 0xFFFF),
    stored checksums 0x0000 and 0xFFFF, ICMP types 8 and 0; the stored checksums are forced, so
    these frames are compared with pyxlat alone."""
    rng = np.random.default_rng(11)
    K = pyxlat.fold(2 * pyxlat.words(prefix))
    c0 = K  # ~C + K = 0xFFFF: the result is 0x0000
    out = []
    for kind, L in (("udp", 64), ("tcp", 60)):
        for c in (c0, 0x0000, 0xFFFF, 0x1234):
            out.append(pyxlat.frame4(kind, L, rng, l4_csum=c))
    for t in (8, 0):
        out.append(pyxlat.frame4("icmp", 98, rng, icmp_type=t))
        out.append(pyxlat.frame4("icmp", 43, rng, icmp_type=t, l4_csum=0xFFFF))
    return out, c0


@pytest.mark.parametrize("pname", list(PFX))
def test_checksum_corners(ctx, pname):
    prefix = PFX[pname]
    frames, c0 = corner_frames(prefix)
    o = (prefix, None, 5, False)
    refs = ref_frames(frames, o)
    if c0 != 0 or pname == "zero":
        assert refs[0][60:62] == b"\xff\xff"  # UDP: never 0x0000
        assert refs[4][70:72] == b"\x00\x00"  # TCP: kept
    fb = upload_frames(ctx, frames)
    try:
        assert check_xlat(ctx, fb, frames, o, scratch=False) == refs
    finally:
        fb.free()


def test_udp_zero_result_still_checks_good(ctx):
    """A good UDP frame whose translated checksum comes out 0x0000: stored as 0xFFFF, good from scratch."""
    prefix = PFX["carry"]
    K = pyxlat.fold(2 * pyxlat.words(prefix))
    rng = np.random.default_rng(3)
    f = None
    for _ in range(10):
        f = bytearray(pyxlat.frame4("udp", 64, rng))
        # move the good checksum to K by changing a payload word with it
        c = int.from_bytes(f[40:42], "big")
        w = int.from_bytes(f[62:64], "big")
        # ~c' + w' = ~c + w (mod 0xFFFF): the sum over the segment stays 0xFFFF
        w2 = (w + (c - K)) % 0xFFFF
        f[40:42] = K.to_bytes(2, "big")
        f[62:64] = w2.to_bytes(2, "big")
        g = pyxlat.xlat46(bytes(f), prefix)
        if pyxlat.check6(g) and g[60:62] == b"\xff\xff":
            break
    else:
        raise AssertionError("no frame found")
    frames = [bytes(f)] * 3
    fb = upload_frames(ctx, frames, fixed=True)
    try:
        refs = check_xlat(ctx, fb, frames, (prefix, None, 0, False))
        assert refs[0][60:62] == b"\xff\xff"
    finally:
        fb.free()


# ------------------------------------------------------------------ 6. refusals
def _xlat(ctx, src, dst, first, n, opts, res=None):
    return ctx.lib.pbgpu_xlat46(ctx.h, src, first, n, opts, dst, res)


def _size(ctx, src, first, n, opts):
    a, b = C.c_uint64(), C.c_uint64()
    return ctx.lib.pbgpu_xlat46_size(ctx.h, src, first, n, opts, C.byref(a), C.byref(b))


def _state(ctx, dst, cap):
    return (int(dst.f.n_frames), int(dst.f.fixed_len), int(dst.f.total_bytes), dst.stream(cap).tobytes())


def other_frames():
    rng = np.random.default_rng(21)
    good = pyxlat.frame4("udp", 64, rng)

    def mut(at, val, base=good):
        b = bytearray(base)
        b[at:at + len(val)] = val
        return bytes(b)

    return {
        "short": good[:33],
        "arp": mut(12, b"\x08\x06"),
        "ihl6": mut(14, b"\x46"),
        "fragment": mut(20, b"\x20\x00"),
        "frag_offset": mut(20, b"\x00\x01"),
        "proto47": mut(23, b"\x2f"),
        "icmp_type3": mut(34, b"\x03", pyxlat.frame4("icmp", 64, rng)),
        "udp41": good[:41],
        "tcp53": pyxlat.frame4("tcp", 54, rng)[:53],
        "icmp41": pyxlat.frame4("icmp", 42, rng)[:41],
    }


@pytest.mark.parametrize("what", list(other_frames()))
def test_one_other_frame_refuses_the_call(ctx, what):
    bad = other_frames()[what]
    assert pyxlat.classify(bad) == pyxlat.OTHER
    rng = np.random.default_rng(22)
    good = [pyxlat.frame4(("udp", "tcp", "icmp")[i % 3], 64, rng) for i in range(300)]
    opts = mkopts(OPTS["label"])
    dst, cap = fresh_dst(ctx, 84 * 300, 300)
    state = _state(ctx, dst, cap)
    try:
        for places in ([0], [150], [299], [40, 200]):
            frames = list(good)
            for p in places:
                frames[p] = bad
            fb = upload_frames(ctx, frames)
            try:
                res = XlatResult()
                assert _xlat(ctx, fb.ptr, dst.ptr, 0, 300, C.byref(opts), C.byref(res)) == EINVAL
                assert _state(ctx, dst, cap) == state
                kinds = [pyxlat.classify(f) for f in frames]
                assert (int(res.n_in), int(res.n_udp), int(res.n_tcp), int(res.n_icmp), int(res.n_other),
                        int(res.first_other)) == (300, kinds.count("udp"), kinds.count("tcp"), kinds.count("icmp"),
                                                  len(places), places[0])
                assert _xlat(ctx, fb.ptr, dst.ptr, 0, 300, C.byref(opts), None) == EINVAL
                assert _state(ctx, dst, cap) == state
                # the size call does not look at the frames
                assert _size(ctx, fb.ptr, 0, 300, C.byref(opts)) == 0
                # an `other` frame outside the range does not matter
                if places == [150]:
                    check_xlat(ctx, fb, frames, OPTS["label"], first=0, n=150, scratch=False)
                    check_xlat(ctx, fb, frames, OPTS["label"], first=151, n=149, scratch=False)
                    res = XlatResult()
                    assert _xlat(ctx, fb.ptr, dst.ptr, 100, 100, C.byref(opts), C.byref(res)) == EINVAL
                    assert (int(res.n_other), int(res.first_other)) == (1, 150)
                    assert _state(ctx, dst, cap) == state
            finally:
                fb.free()
    finally:
        dst.free()


def test_argument_errors(ctx):
    rng = np.random.default_rng(23)
    frames = [pyxlat.frame4("udp", 64, rng) for _ in range(300)]
    fb = upload_frames(ctx, frames, fixed=True)
    never = ctx.alloc_frames(16, 1024)
    dst, cap = fresh_dst(ctx, 84 * 300, 300)
    state = _state(ctx, dst, cap)
    ok = mkopts(OPTS["label"])

    def refused(rc, src, first, n, opts, d=dst, sized=True):
        assert _xlat(ctx, src, d.ptr if d is not None else None, first, n, opts) == rc
        if sized and rc == EINVAL:
            assert _size(ctx, src, first, n, opts) == rc
        assert _state(ctx, dst, cap) == state

    try:
        # NULL arguments
        refused(EINVAL, None, 0, 300, C.byref(ok))
        refused(EINVAL, fb.ptr, 0, 300, None)
        refused(EINVAL, fb.ptr, 0, 300, C.byref(ok), d=None, sized=False)
        assert ctx.lib.pbgpu_xlat46(None, fb.ptr, 0, 300, C.byref(ok), dst.ptr, None) == EINVAL
        a = C.c_uint64()
        assert ctx.lib.pbgpu_xlat46_size(ctx.h, fb.ptr, 0, 300, C.byref(ok), None, C.byref(a)) == EINVAL
        assert ctx.lib.pbgpu_xlat46_size(ctx.h, fb.ptr, 0, 300, C.byref(ok), C.byref(a), None) == EINVAL
        # a source never built or uploaded
        refused(EINVAL, never.ptr, 0, 0, C.byref(ok))
        # a range past n_frames
        refused(EINVAL, fb.ptr, 1, 300, C.byref(ok))
        refused(EINVAL, fb.ptr, 301, 0, C.byref(ok))
        # src == dst, overlapping allocations
        assert _xlat(ctx, fb.ptr, fb.ptr, 0, 1, C.byref(ok)) == EINVAL
        alias = pbgpu.Frames.from_buffer_copy(dst.f)
        alias.data = fb.f.data + 4096
        alias.capacity_bytes = 1024
        assert _xlat(ctx, fb.ptr, C.byref(alias), 0, 1, C.byref(ok)) == EINVAL
        # flow label, flags, reserved
        for bad in (dict(flow_label=1 << 20), dict(flags=2), dict(flags=3), dict(reserved=1)):
            o = mkopts(OPTS["label"])
            for k, v in bad.items():
                setattr(o, k, v)
            refused(EINVAL, fb.ptr, 0, 300, C.byref(o))
        # a destination too small: frames, bytes
        few = pbgpu.Frames.from_buffer_copy(dst.f)
        few.capacity_frames = 299
        assert _xlat(ctx, fb.ptr, C.byref(few), 0, 300, C.byref(ok)) == ENOSPC
        short = pbgpu.Frames.from_buffer_copy(dst.f)
        need = 84 * 300  # 25200, a multiple of 16
        assert need % 16 == 0
        short.capacity_bytes = need - 16
        assert _xlat(ctx, fb.ptr, C.byref(short), 0, 300, C.byref(ok)) == ENOSPC
        assert _state(ctx, dst, cap) == state
        with pytest.raises(PbError) as e:
            small = ctx.alloc_frames(300, 1024)
            try:
                fb.xlat46(small, opts=ok)
            finally:
                small.free()
        assert e.value.code == ENOSPC
        short.capacity_bytes = need
        short.capacity_frames = 300
        assert _xlat(ctx, fb.ptr, C.byref(short), 0, 300, C.byref(ok)) == 0
    finally:
        dst.free()
        never.free()
        fb.free()


def test_longest_frame(ctx):
    """65516 B is one byte too long for a 16-bit frame length after translation; 65515 B is taken."""
    opts = mkopts(OPTS["label"])
    rng = np.random.default_rng(24)
    dst, cap = fresh_dst(ctx, 3 * 65536, 64)
    state = _state(ctx, dst, cap)
    too = upload_frames(ctx, [pyxlat.frame4("udp", 64, rng), pyxlat.frame4("udp", 65516, rng)])
    try:
        assert _xlat(ctx, too.ptr, dst.ptr, 0, 2, C.byref(opts)) == EINVAL
        assert _xlat(ctx, too.ptr, dst.ptr, 0, 1, C.byref(opts)) == EINVAL  # the buffer's frames, not the range's
        assert _size(ctx, too.ptr, 0, 2, C.byref(opts)) == EINVAL
        assert _state(ctx, dst, cap) == state
    finally:
        too.free()
        dst.free()


# ------------------------------------------------------------------ 7. composition
@pytest.mark.parametrize("src", ["fixed", "variable"])
def test_composition(ctx, mixed1000, src):
    if src == "fixed":
        rng = np.random.default_rng(31)
        frames = [pyxlat.frame4(("udp", "tcp", "icmp")[i % 3], 64, rng) for i in range(300)]
        fb = upload_frames(ctx, frames, fixed=True)
    else:
        fb, frames = mixed1000[0], mixed1000[1][:400]
    n = len(frames)
    o = OPTS["label"]
    refs, x6 = check_xlat(ctx, fb, frames, o, n=n, keep=True)
    total = sum(len(r) for r in refs)
    tmp, tcap = fresh_dst(ctx, total + 50 * n, n)
    try:
        assert x6.frames() == refs
        # packed into a pcap stream
        assert x6.pcap_bytes(t0_ns=10**18, step_ps=6_720_000).tobytes() == pypcap.pcap_stream(refs, 10**18, 6_720_000)
        # encapsulated
        x6.encap(tmp, mode=ENCAP_VLAN, tci=100)
        assert tmp.frames() == [pyencap.vlan(r, 100) for r in refs]
        x6.encap(tmp, mode=ENCAP_VXLAN, **VX)
        assert tmp.frames() == [pyencap.vxlan(r, **VX) for r in refs]
        # landed in slots
        slot = 2048
        before = np.full(slot * n, 0x5A, dtype=np.uint8)
        umem = before.copy()
        lens = x6.to_umem(umem, slot, 0, n)
        want, want_lens = pyland.land(before, [np.frombuffer(r, dtype=np.uint8) for r in refs], slot, 0, 0, n)
        assert np.array_equal(umem, want) and np.array_equal(np.asarray(lens, dtype=np.uint16), want_lens)
        # no IPv4 in it: the stamp takes none, the fragmenter copies all, a second translation refuses
        image = x6.packed().copy()
        res = x6.stamp(t0_ns=5, step_ps=1000)
        assert (int(res.n_in), int(res.n_stamped), int(res.n_short), int(res.n_other)) == (n, 0, 0, n)
        assert np.array_equal(x6.packed(), image)
        fr = x6.fragment(tmp, mtu=68)
        assert (int(fr.n_in), int(fr.n_out), int(fr.n_split)) == (n, n, 0)
        assert tmp.frames() == refs
        state = _state(ctx, tmp, tcap)
        xr = XlatResult()
        assert _xlat(ctx, x6.ptr, tmp.ptr, 0, n, C.byref(mkopts(o)), C.byref(xr)) == EINVAL
        assert (int(xr.n_other), int(xr.first_other)) == (n, 0)
        assert _state(ctx, tmp, tcap) == state
        # the destination reused for a shorter output: nothing past the new frames' pad is touched
        old = x6.stream(((total + 15) & ~15) + 64).copy()
        m = n // 3
        short_refs = ref_frames(frames[5:5 + m], OPTS["hash"])
        fb.xlat46(x6, 5, m, mkopts(OPTS["hash"]))
        t2 = sum(len(r) for r in short_refs)
        r16 = (t2 + 15) & ~15
        got = x6.stream(len(old))
        assert got[:t2].tobytes() == b"".join(short_refs) and not got[t2:r16].any()
        assert np.array_equal(got[r16:], old[r16:])
        assert (int(x6.f.n_frames), int(x6.f.total_bytes)) == (m, t2)
    finally:
        tmp.free()
        x6.free()
        if src == "fixed":
            fb.free()


def test_rebuild_of_the_source_queued_behind_the_call(ctx):
    """A build into src is queued right after the translation with no sync between: the translation
    read the old frames (it returns when its frames are in place), the build then gives the new ones."""
    seq = Sequence.from_config(pc.get("c2_udp_64"))
    n = 4096
    ctx.load_sequence(0, seq, pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n))
    dst = ctx.alloc_frames(n, 84 * n)
    try:
        o = OPTS["hash"]
        ctx.build(0, 0, n, fb)
        fb.xlat46(dst, opts=mkopts(o))
        ctx.build(0, n, n, fb)  # not waited for
        olds = ob.frames(seq, 0, 0, n, pc.SEED_BASE)
        assert dst.stream(84 * n).tobytes() == b"".join(ref_frames(olds, o))
        fb.xlat46(dst, opts=mkopts(o))  # follows the queued build
        news = ob.frames(seq, 0, n, n, pc.SEED_BASE)
        assert dst.stream(84 * n).tobytes() == b"".join(ref_frames(news, o))
    finally:
        dst.free()
        fb.free()


# ------------------------------------------------------------------ 8. several pages to a workgroup
def test_workgroups_that_own_several_pages(ctx):
    """An output above 64 MiB gives a workgroup more than one page, so the variable-length window is
    carried from page to page: 220,000 frames of configs[2], three windows of the output against
    pyxlat of the oracle's frames for those iterations."""
    seq = Sequence.from_config(pc.get("c3_udp_var"))
    n, first_iter = 220_000, 5000
    ctx.load_sequence(0, seq, pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n))
    o = OPTS["hash"]
    try:
        ctx.build(0, first_iter, n, fb)
        ctx.sync()
        total = fb.total_bytes() + 20 * n
        assert ((total + 4095) >> 12) // 16384 >= 2  # pages per workgroup
        dst = ctx.alloc_frames(n, total + 16)
        try:
            res = fb.xlat46(dst, opts=mkopts(o))
            assert (int(res.n_udp), int(res.n_other)) == (n, 0)
            assert (int(dst.f.n_frames), int(dst.f.fixed_len), int(dst.f.total_bytes)) == (n, 0, total)
            off = dst.offsets()
            assert int(off[n]) == total
            for j_lo, cnt in ((0, 300), (n // 2 - 150, 300), (n - 300, 300)):
                frames = ob.frames(seq, 0, first_iter + j_lo, cnt, pc.SEED_BASE)
                ref = b"".join(ref_frames(frames, o))
                a = int(off[j_lo])
                assert int(off[j_lo + cnt]) - a == len(ref)
                assert dst.stream(len(ref), a).tobytes() == ref, j_lo
        finally:
            dst.free()
    finally:
        fb.free()
