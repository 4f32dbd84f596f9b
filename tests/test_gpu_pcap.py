"""pbgpu_pcap_pack on the GPU: the packed stream byte for byte against tests/pypcap.py, which
writes the stream from its definition with `struct` and Python integers.

Sources are oracle frames (built by the CPU oracle and uploaded, or built by the GPU and compared
through the oracle's bytes).  Every destination buffer is first filled with 0xA5 by an upload, so a
stray write shows; every pack is checked over the whole buffer: the stream, zeros up to the next
multiple of 16, 0xA5 after that."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import pb_configs as pc
import pbgpu
import pypcap
from pbgpu import GpuContext, PbError, Sequence

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_123_456_789
STEP = 14_880_952  # ps: 67.2 kpps
SLACK = 4096 + 64  # bytes of the destination past the stream, watched for stray writes


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def oracle_frames(name, n, first=12345):
    return ob.build(Sequence.from_config(pc.get(name)), 0, first, n, pc.SEED_BASE)


def split(data, off):
    return [bytes(data[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def uploaded(ctx, data, off=None, flen=0):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = len(off) - 1 if off is not None else len(data) // flen
    fb = ctx.alloc_frames(max(n, 1), max(len(data), 16))
    fb.upload(data, offsets=off, fixed_len=flen)
    return fb


def fresh_dst(ctx, nbytes):
    """A destination of the stream's size rounded up to 16 plus SLACK, every byte 0xA5."""
    cap = ((nbytes + 15) & ~15) + SLACK
    dst = ctx.alloc_frames(cap // 16, cap)
    dst.upload(np.full(cap, 0xA5, dtype=np.uint8), fixed_len=16)
    assert int(dst.f.n_frames) == cap // 16
    return dst, cap


def check_pack(ctx, fb, frames, first=0, n=None, **kw):
    """Packs fb's frames [first, first + n) and compares the whole destination; `frames` are the
    buffer's frames as bytes.  Returns the stream."""
    n = len(frames) - first if n is None else n
    ref = pypcap.pcap_stream(frames[first:first + n], kw.get("t0_ns", 0), kw.get("step_ps", 0),
                             kw.get("first_index", 0), kw.get("file_header", True), kw.get("nsec", False))
    flags = (pbgpu.PCAP_FILE_HEADER if kw.get("file_header", True) else 0) | (pbgpu.PCAP_NSEC if kw.get("nsec") else 0)
    assert ctx.pcap_size(fb, first, n, flags) == len(ref)
    before = fb.packed().copy()
    n_frames_before = int(fb.f.n_frames)
    dst, cap = fresh_dst(ctx, len(ref))
    try:
        nbytes, ms = fb.pcap_pack(dst, first, n, **kw)
        assert nbytes == len(ref) and ms >= 0
        got = dst.stream(cap).tobytes()
        r16 = (nbytes + 15) & ~15
        bad = next((i for i in range(nbytes) if got[i] != ref[i]), None) if got[:nbytes] != ref else None
        assert bad is None, (bad, got[max(0, bad - 8):bad + 8].hex(), ref[max(0, bad - 8):bad + 8].hex())
        assert got[nbytes:r16] == bytes(r16 - nbytes)
        assert got[r16:] == b"\xa5" * (cap - r16)
        # dst is plain bytes now: no frames; src is untouched
        assert (int(dst.f.n_frames), int(dst.f.fixed_len), int(dst.f.total_bytes)) == (0, 0, nbytes)
        assert dst.verify().n_checked == 0
        assert int(fb.f.n_frames) == n_frames_before and np.array_equal(fb.packed(), before)
    finally:
        dst.free()
    return ref


# ------------------------------------------------------------------ 1. fixed lengths
@pytest.fixture(scope="module")
def udp64():
    data, off = oracle_frames("c2_udp_64", 512)
    return data, split(data, off)


@pytest.mark.parametrize("hdr", [True, False])
@pytest.mark.parametrize("n", [1, 2, 51, 52, 257])
def test_fixed_udp64(ctx, udp64, n, hdr):
    """80-B records: 51.2 per page, so 51 and 52 straddle the first page edge; with the header
    record k starts at 24 + 80 k, 8 mod 16."""
    data, frames = udp64
    fb = uploaded(ctx, data[:64 * n], flen=64)
    try:
        check_pack(ctx, fb, frames[:n], t0_ns=T0, step_ps=STEP, file_header=hdr)
    finally:
        fb.free()


@pytest.mark.parametrize("hdr", [True, False])
def test_fixed_tcp_syn_built_on_the_gpu(ctx, hdr):
    """60-B frames, 76-B records: every alignment mod 4 of source and destination."""
    seq = Sequence.from_config(pc.get("c4_tcp_syn"))
    ctx.load_sequence(0, seq, pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, 300))
    try:
        ctx.build(0, 777, 300, fb)
        ctx.sync()
        data, off = ob.build(seq, 0, 777, 300, pc.SEED_BASE)
        assert int(fb.f.fixed_len) == 60 and np.array_equal(fb.packed(), data)
        check_pack(ctx, fb, split(data, off), t0_ns=T0, step_ps=STEP, file_header=hdr)
    finally:
        fb.free()


@pytest.mark.parametrize("hdr", [True, False])
@pytest.mark.parametrize("flen,n", [(1, 500), (35, 500), (61, 500), (1500, 40), (65535, 3)])
def test_fixed_uploaded(ctx, flen, n, hdr):
    """Odd lengths for odd source and destination alignments; 1500 B; 65535 B: one record over 17
    pages."""
    rng = np.random.default_rng(flen)
    data = rng.integers(0, 256, flen * n, dtype=np.uint8)
    fb = uploaded(ctx, data, flen=flen)
    try:
        check_pack(ctx, fb, [bytes(data[i * flen:(i + 1) * flen]) for i in range(n)], t0_ns=T0, step_ps=STEP,
                   file_header=hdr)
    finally:
        fb.free()


# ------------------------------------------------------------------ 2. variable lengths
@pytest.mark.parametrize("how", ["built", "uploaded"])
def test_variable_config2(ctx, how):
    seq = Sequence.from_config(pc.get("c3_udp_var"))
    data, off = ob.build(seq, 0, 4242, 600, pc.SEED_BASE)
    if how == "built":
        ctx.load_sequence(0, seq, pc.SEED_BASE)
        fb = ctx.alloc_frames(*ctx.build_size(0, 600))
        ctx.build(0, 4242, 600, fb)
        ctx.sync()
    else:
        fb = uploaded(ctx, data, off=off)
    try:
        assert int(fb.f.fixed_len) == 0
        frames = split(data, off)
        check_pack(ctx, fb, frames, t0_ns=T0, step_ps=STEP)
        check_pack(ctx, fb, frames, t0_ns=T0, step_ps=STEP, file_header=False, nsec=True)
    finally:
        fb.free()


def lens_to_frames(lens, seed):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.uint64))]).astype(np.uint64)
    data = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    return data, off


EDGE_LENS = [0, 0, 1, 15, 16, 17, 4079, 4080, 4081, 0, 65535, 34]


@pytest.mark.parametrize("hdr", [True, False])
def test_variable_edge_lengths(ctx, hdr):
    """Empty frames, lengths around a chunk, 16 + 4080: a record ending exactly on a page edge."""
    data, off = lens_to_frames(EDGE_LENS, 1)
    fb = uploaded(ctx, data, off=off)
    try:
        check_pack(ctx, fb, split(data, off), t0_ns=T0, step_ps=STEP, file_header=hdr)
    finally:
        fb.free()


def random3000_frames():
    lens = np.random.default_rng(99).integers(0, 201, 3000)
    return lens_to_frames(lens, 2)


@pytest.fixture(scope="module")
def random3000(ctx):
    data, off = random3000_frames()
    fb = uploaded(ctx, data, off=off)
    yield fb, split(data, off), off
    fb.free()


@pytest.mark.parametrize("hdr", [True, False])
def test_variable_random_lengths(ctx, random3000, hdr):
    fb, frames, _ = random3000
    check_pack(ctx, fb, frames, t0_ns=T0, step_ps=STEP, file_header=hdr)


# ------------------------------------------------------------------ 3. sub-ranges
def test_subrange_fixed(ctx, udp64):
    data, frames = udp64
    fb = uploaded(ctx, data[:64 * 300], flen=64)
    try:
        check_pack(ctx, fb, frames[:300], first=7, n=100, t0_ns=T0, step_ps=STEP, first_index=7)
        check_pack(ctx, fb, frames[:300], first=299, n=1, file_header=False)
    finally:
        fb.free()


@pytest.mark.parametrize("align", [1, 2, 3])
def test_subrange_source_alignment(ctx, random3000, align):
    """A range whose first frame starts at byte alignment 1, 2, 3 mod 4 of the source."""
    fb, frames, off = random3000
    first = next(i for i in range(10, 3000) if int(off[i]) % 4 == align and len(frames[i]) > 0)
    check_pack(ctx, fb, frames, first=first, n=400, t0_ns=T0, step_ps=STEP, first_index=first)
    check_pack(ctx, fb, frames, first=first, n=400, file_header=False)


@pytest.mark.parametrize("flen", [35, 61])
def test_subrange_fixed_odd_alignment(ctx, flen):
    data = np.random.default_rng(5).integers(0, 256, flen * 64, dtype=np.uint8)
    fb = uploaded(ctx, data, flen=flen)
    frames = [bytes(data[i * flen:(i + 1) * flen]) for i in range(64)]
    try:
        for first in (1, 2, 3):
            check_pack(ctx, fb, frames, first=first, n=50, t0_ns=T0, step_ps=STEP)
    finally:
        fb.free()


@pytest.mark.parametrize("hdr", [True, False])
def test_zero_frames(ctx, random3000, udp64, hdr):
    """n = 0: the file header alone, or nothing."""
    fb, frames, _ = random3000
    assert check_pack(ctx, fb, frames, first=5, n=0, file_header=hdr) == (pypcap.pcap_file_header() if hdr else b"")
    assert check_pack(ctx, fb, frames, first=3000, n=0, file_header=hdr, nsec=True) == \
        (pypcap.pcap_file_header(True) if hdr else b"")
    fx = uploaded(ctx, udp64[0][:640], flen=64)
    try:
        assert len(check_pack(ctx, fx, udp64[1][:10], first=10, n=0, file_header=hdr)) == (24 if hdr else 0)
        assert np.array_equal(fx.pcap_bytes(n=0, file_header=hdr), np.frombuffer(
            pypcap.pcap_file_header() if hdr else b"", dtype=np.uint8))
    finally:
        fx.free()


# ------------------------------------------------------------------ 4. concatenation
@pytest.mark.parametrize("kind", ["fixed", "variable"])
@pytest.mark.parametrize("a", [1, 51, 255])
def test_batches_concatenate(ctx, udp64, random3000, kind, a):
    """[0, a) then [a, n) with first_index 0 / a, the second without the file header, is the pack of
    [0, n).  step 333333 ps: a t0 truncated per batch would differ."""
    if kind == "fixed":
        fb, frames = uploaded(ctx, udp64[0], flen=64), udp64[1]
    else:
        fb, frames = random3000[0], random3000[1]
    try:
        n, step = 512, 333_333
        whole = fb.pcap_bytes(0, n, T0, step, 0, True, True).tobytes()
        assert whole == pypcap.pcap_stream(frames[:n], T0, step, 0, True, True)
        head = fb.pcap_bytes(0, a, T0, step, 0, True, True).tobytes()
        tail = fb.pcap_bytes(a, n - a, T0, step, a, False, True).tobytes()
        assert head + tail == whole
        # a second batch started from a truncated t0 instead is really different on this step
        assert pypcap.pcap_stream(frames[a:n], T0 + (a * step) // 1000, step, 0, False, True) != tail
        us = fb.pcap_bytes(0, a, T0, step, 0, True, False).tobytes() + \
            fb.pcap_bytes(a, n - a, T0, step, a, False, False).tobytes()
        assert us == pypcap.pcap_stream(frames[:n], T0, step, 0, True, False)
    finally:
        if kind == "fixed":
            fb.free()


# ------------------------------------------------------------------ 5. timestamps
STAMP_CASES = {
    "second_rolls": dict(t0_ns=1_700_000_000 * 10**9 + 999_999_000, step_ps=7_000_000),  # 1 us left: at record 1
    "second_rolls_at_143": dict(t0_ns=1_700_000_000 * 10**9 + 999_000_000, step_ps=7_000_000),  # 1 ms left
    "step_0": dict(t0_ns=T0, step_ps=0),
    "step_1": dict(t0_ns=T0, step_ps=1, first_index=999),
    "past_2_32_seconds": dict(t0_ns=(2**32 + 17) * 10**9 + 999_999_999, step_ps=1_000_000),
    "large_first_index": dict(t0_ns=T0, step_ps=3, first_index=2**40),
    "huge_product": dict(t0_ns=5, step_ps=2**33 + 1, first_index=2**30),
}


@pytest.mark.parametrize("nsec", [False, True])
@pytest.mark.parametrize("case", list(STAMP_CASES))
def test_timestamps(ctx, udp64, case, nsec):
    data, frames = udp64
    fb = uploaded(ctx, data[:64 * 300], flen=64)
    try:
        ref = check_pack(ctx, fb, frames[:300], nsec=nsec, **STAMP_CASES[case])
        if case == "second_rolls":
            _, recs = pypcap.read_pcap(ref)
            assert recs[0][0] == 1_700_000_000 and recs[1][0] == 1_700_000_001
        if case == "second_rolls_at_143":
            _, recs = pypcap.read_pcap(ref)
            assert recs[142][0] == 1_700_000_000 and recs[143][0] == 1_700_000_001
        if case == "past_2_32_seconds":
            assert pypcap.read_pcap(ref)[1][0][0] == 17
    finally:
        fb.free()


def test_timestamps_variable(ctx, random3000):
    fb, frames, _ = random3000
    check_pack(ctx, fb, frames, nsec=True, **STAMP_CASES["second_rolls"])
    check_pack(ctx, fb, frames, **STAMP_CASES["large_first_index"])


# ------------------------------------------------------------------ 7. errors
def _pack(ctx, src, dst, first, n, opts):
    nbytes, ms = C.c_uint64(), C.c_double()
    return ctx.lib.pbgpu_pcap_pack(ctx.h, src, first, n, opts, dst, C.byref(nbytes), C.byref(ms))


def test_errors(ctx, udp64):
    data, _ = udp64
    fb = uploaded(ctx, data[:64 * 100], flen=64)
    never = ctx.alloc_frames(16, 1024)
    need = 24 + 80 * 100
    dst = ctx.alloc_frames(1, need)
    ok = pbgpu.PcapOpts(T0, STEP, 0, pbgpu.PCAP_FILE_HEADER, 0)
    nb = C.c_uint64()
    EINVAL, ENOSPC = -22, -28
    try:
        assert _pack(ctx, fb.ptr, dst.ptr, 0, 100, C.byref(ok)) == 0
        # NULL arguments
        assert _pack(ctx, None, dst.ptr, 0, 100, C.byref(ok)) == EINVAL
        assert _pack(ctx, fb.ptr, None, 0, 100, C.byref(ok)) == EINVAL
        assert _pack(ctx, fb.ptr, dst.ptr, 0, 100, None) == EINVAL
        assert ctx.lib.pbgpu_pcap_pack(ctx.h, fb.ptr, 0, 100, C.byref(ok), dst.ptr, None, None) == EINVAL
        assert ctx.lib.pbgpu_pcap_size(ctx.h, fb.ptr, 0, 100, 1, None) == EINVAL
        assert ctx.lib.pbgpu_pcap_size(ctx.h, None, 0, 100, 1, C.byref(nb)) == EINVAL
        # a source never built or uploaded
        assert _pack(ctx, never.ptr, dst.ptr, 0, 0, C.byref(ok)) == EINVAL
        assert ctx.lib.pbgpu_pcap_size(ctx.h, never.ptr, 0, 0, 1, C.byref(nb)) == EINVAL
        # a range past n_frames
        assert _pack(ctx, fb.ptr, dst.ptr, 1, 100, C.byref(ok)) == EINVAL
        assert _pack(ctx, fb.ptr, dst.ptr, 101, 0, C.byref(ok)) == EINVAL
        assert ctx.lib.pbgpu_pcap_size(ctx.h, fb.ptr, 0, 101, 1, C.byref(nb)) == EINVAL
        # src == dst, overlapping data
        assert _pack(ctx, fb.ptr, fb.ptr, 0, 1, C.byref(ok)) == EINVAL
        alias = pbgpu.Frames.from_buffer_copy(dst.f)
        alias.data = fb.f.data + 4096
        alias.capacity_bytes = 1024
        assert _pack(ctx, fb.ptr, C.byref(alias), 0, 1, C.byref(ok)) == EINVAL
        # unknown flag bits, reserved
        assert _pack(ctx, fb.ptr, dst.ptr, 0, 100, C.byref(pbgpu.PcapOpts(T0, STEP, 0, 4, 0))) == EINVAL
        assert _pack(ctx, fb.ptr, dst.ptr, 0, 100, C.byref(pbgpu.PcapOpts(T0, STEP, 0, 1, 1))) == EINVAL
        assert ctx.lib.pbgpu_pcap_size(ctx.h, fb.ptr, 0, 100, 8, C.byref(nb)) == EINVAL
        # (first_index + n - 1) * step_ps >= 2^64
        assert _pack(ctx, fb.ptr, dst.ptr, 0, 3, C.byref(pbgpu.PcapOpts(0, 2**63, 0, 1, 0))) == EINVAL
        assert _pack(ctx, fb.ptr, dst.ptr, 0, 2, C.byref(pbgpu.PcapOpts(0, 2**63, 0, 1, 0))) == 0
        assert _pack(ctx, fb.ptr, dst.ptr, 0, 2, C.byref(pbgpu.PcapOpts(0, 1, 2**64 - 1, 1, 0))) == EINVAL
        # a destination too small (an allocation's capacity is a whole multiple of 16)
        assert need % 16 == 8
        small = ctx.alloc_frames(1, need - 9)
        try:
            assert int(small.f.capacity_bytes) < ((need + 15) & ~15)
            assert _pack(ctx, fb.ptr, small.ptr, 0, 100, C.byref(ok)) == ENOSPC
            with pytest.raises(PbError) as e:
                fb.pcap_pack(small, t0_ns=T0)
            assert e.value.code == ENOSPC
        finally:
            small.free()
        exact = ctx.alloc_frames(1, (need + 15) & ~15)
        try:
            assert _pack(ctx, fb.ptr, exact.ptr, 0, 100, C.byref(ok)) == 0
            assert _pack(ctx, fb.ptr, exact.ptr, 0, 100, C.byref(pbgpu.PcapOpts(T0, STEP, 0, 0, 0))) == 0
        finally:
            exact.free()
    finally:
        dst.free()
        never.free()
        fb.free()


def test_one_byte_short(ctx):
    """A destination whose capacity is one byte below the stream rounded up to 16.  An allocation's
    capacity is itself rounded up to 16, so the byte is taken off in a copy of the descriptor."""
    data = np.arange(48 * 4, dtype=np.uint8)
    fb = uploaded(ctx, data, flen=48)  # 4 records of 64 B, no file header: 256 B
    dst = ctx.alloc_frames(1, 256)
    small = ctx.alloc_frames(1, 240)
    opts = pbgpu.PcapOpts(T0, STEP, 0, 0, 0)
    try:
        assert fb.pcap_pack(dst, file_header=False)[0] == 256
        short = pbgpu.Frames.from_buffer_copy(dst.f)
        short.capacity_bytes = 255
        assert _pack(ctx, fb.ptr, C.byref(short), 0, 4, C.byref(opts)) == -28
        # 3 records and the file header: 216 B, 224 rounded up; 223 is one byte short of that
        opts.flags = pbgpu.PCAP_FILE_HEADER
        short.capacity_bytes = 223
        assert _pack(ctx, fb.ptr, C.byref(short), 0, 3, C.byref(opts)) == -28
        short.capacity_bytes = 224
        assert _pack(ctx, fb.ptr, C.byref(short), 0, 3, C.byref(opts)) == 0
        with pytest.raises(PbError) as e:
            fb.pcap_pack(small, file_header=False)
        assert e.value.code == -28
        assert fb.pcap_pack(small, n=3, file_header=False)[0] == 192
    finally:
        small.free()
        dst.free()
        fb.free()


# ------------------------------------------------------------------ 8. past 2^32 bytes
def test_stream_past_4_gib(ctx):
    """2^26 64-B frames built on the GPU (4 GiB), packed into 5.4 GB; three 1-MiB windows (the
    start, around byte 2^32, the end) against the oracle's frames for just those iterations."""
    n, first_iter, win = 1 << 26, 1000, 1 << 20
    seq = Sequence.from_config(pc.get("c2_udp_64"))
    ctx.load_sequence(0, seq, pc.SEED_BASE)
    total = 24 + 80 * n
    try:
        fb = ctx.alloc_frames(*ctx.build_size(0, n))
    except PbError as e:
        pytest.skip("cannot allocate the 4-GiB frame buffer: %s" % e)
    try:
        try:
            dst = ctx.alloc_frames(1, total)
        except PbError as e:
            pytest.skip("cannot allocate the 5.4-GB stream buffer: %s" % e)
        try:
            ctx.build(0, first_iter, n, fb)
            ctx.sync()
            nbytes, _ = fb.pcap_pack(dst, t0_ns=T0, step_ps=6_720)
            assert nbytes == total == ctx.pcap_size(fb)
            for a in (0, (1 << 32) - win // 2, total - win):
                b = a + win
                j_lo, j_hi = max(a - 24, 0) // 80, (b - 24 - 1) // 80
                data, off = ob.build(seq, 0, first_iter + j_lo, j_hi - j_lo + 1, pc.SEED_BASE)
                ref = pypcap.pcap_stream(split(data, off), T0, 6_720, j_lo, a == 0, False)
                pos = 0 if a == 0 else 24 + 80 * j_lo  # stream position of ref[0]
                assert dst.stream(win, a).tobytes() == ref[a - pos:b - pos], a
        finally:
            dst.free()
    finally:
        fb.free()
