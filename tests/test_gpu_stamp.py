"""pbgpu_stamp on the GPU: every byte of the buffer's whole capacity and every field of the result
against tests/pystamp.py, which writes the stamp from its definition with `struct` and Python
integers.

A buffer is first filled with 0xA5 by an upload and then takes the frames, so the pad and the slack
behind the frames hold a known value; it is fetched whole before and after the stamp and the second
copy must equal pystamp applied to the first.  The buffer's metadata and device offsets are compared
as well."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import pb_configs as pc
import pbgpu
import pyencap
import pyfrag
import pypcap
import pystamp
import verify_ref as vr
from pbgpu import GpuContext, PbError, Sequence, StampOpts, StampResult
from stamp_frames import frame_ok, l4_frame, pack

pytestmark = pytest.mark.gpu

SLACK = 4096 + 64  # bytes of the buffer past the frames, watched for stray writes
EINVAL = -22
T0, STEP = 1_700_000_000_123_456_789, 672_000
POSITIONS = [(False, 0), (False, 1), (False, 5), (True, 0), (True, 1), (True, 5)]


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def prepared(ctx, frames, flen=0):
    """(buffer, capacity, offsets): the frames uploaded into a buffer whose every other byte is 0xA5."""
    data, off = pack(frames)
    cap = ((len(data) + 15) & ~15) + SLACK
    fb = ctx.alloc_frames(max(cap // 16, len(frames), 1), cap)
    fb.upload(np.full(cap, 0xA5, dtype=np.uint8), fixed_len=16)
    fb.upload(data, offsets=None if flen else off, fixed_len=flen)
    return fb, cap, off


def meta(fb):
    f = fb.f
    return int(f.n_frames), int(f.fixed_len), int(f.total_bytes), int(f.capacity_frames), int(f.capacity_bytes)


def check_stamp(ctx, fb, cap, off, first=0, n=None, t0_ns=T0, step_ps=STEP, first_index=0, offset=0, tail=False,
                csum=True):
    """Stamps fb's frames [first, first + n) and compares the whole capacity, the result, the
    metadata and the offsets.  Returns (the bytes after, the counts)."""
    n = len(off) - 1 - first if n is None else n
    before = fb.stream(cap).tobytes()
    m0 = meta(fb)
    want, cnt = pystamp.stamp_buffer(before, off, first, n, t0_ns, step_ps, first_index, offset, tail, csum)
    res = fb.stamp(first, n, t0_ns, step_ps, first_index, offset, tail, csum)
    got = fb.stream(cap).tobytes()
    if got != want:
        bad = next(i for i in range(cap) if got[i] != want[i])
        j = int(np.searchsorted(np.asarray(off, dtype=np.uint64), bad, side="right")) - 1
        raise AssertionError(("byte", bad, "frame", j, got[max(0, bad - 8):bad + 8].hex(),
                              want[max(0, bad - 8):bad + 8].hex()))
    assert (int(res.n_in), int(res.n_stamped), int(res.n_short), int(res.n_other)) == \
        (n, cnt["stamped"], cnt["short"], cnt["other"])
    assert res.device_ms >= 0
    assert meta(fb) == m0
    if not m0[1]:
        assert np.array_equal(fb.offsets(), np.asarray(off, dtype=np.uint64))
    return got, cnt


def verify_clean(fb):
    res = fb.verify()
    assert (int(res.n_checked), int(res.n_bad)) == (int(fb.f.n_frames), 0)


def codes_before(frames):
    """The reference's verify codes of the frames as made (a frame too short for its checksum field
    carries none): a stamp with the checksum update changes no frame's code."""
    return vr.ref_codes(*pack(frames))


def verify_same(fb, codes):
    res, got = fb.verify(codes=True)
    vr.expect(res, got, codes)


# ------------------------------------------------------------------ 1. fixed-length UDP, uploaded
FIXED = [(L, n) for L in (57, 58, 59, 60, 64, 65, 98, 1500, 4092) for n in (1, 2, 257)] + \
        [(64, n) for n in (63, 64, 65)]  # 64-B frames either side of a page edge


@pytest.mark.parametrize("L,n", FIXED)
def test_fixed_udp(ctx, L, n):
    frames = [l4_frame(17, L, 100 * L + j) for j in range(n)]
    for tail, offset in POSITIONS:
        fb, cap, off = prepared(ctx, frames, flen=L)
        try:
            _, cnt = check_stamp(ctx, fb, cap, off, first_index=1 << 40, offset=offset, tail=tail)
            fits = L - 42 - 16 - offset >= 0
            assert cnt == dict(stamped=n if fits else 0, short=0 if fits else n, other=0)
            verify_clean(fb)
        finally:
            fb.free()


# ------------------------------------------------------------------ 2. variable lengths, uploaded
def _var_frames():
    rng = np.random.default_rng(5)
    frames = []
    for j in range(900):
        L = int(rng.integers(34, 201))
        kind = j % 4
        if kind == 0 or kind == 3:
            frames.append(l4_frame(17, L, j))
        elif kind == 1:
            frames.append(l4_frame(6, L, j, doff=5 if j % 8 == 1 else 8))
        else:
            frames.append(l4_frame(1, L, j))
    return frames


@pytest.fixture(scope="module")
def var(ctx):
    frames = _var_frames()
    fb, cap, off = prepared(ctx, frames)
    yield fb, cap, off, frames
    fb.free()


def test_variable_every_alignment(ctx, var):
    """Lengths 34..200, UDP / TCP (data offset 5 and 8) / ICMP packed back to back: over the run the
    stamp's address takes every value mod 16, a both parities, and a tail stamp ends frames of odd L4
    length (the 9th word's missing byte).  Each stamp goes over the last one's bytes."""
    fb, cap, off, frames = var
    codes = codes_before(frames)
    assert 0 < np.count_nonzero(codes) < 100
    align, parity, ninth = set(), set(), 0
    for k, (tail, offset) in enumerate(POSITIONS):
        got, cnt = check_stamp(ctx, fb, cap, off, first_index=1000 * k, offset=offset, tail=tail)
        assert cnt["stamped"] > 200 and cnt["short"] > 50
        for j, f in enumerate(frames):
            cls, S, _ = pystamp.position(f, offset, tail)
            if cls == "stamped":
                align.add((int(off[j]) + S) % 16)
                parity.add((S - 34) & 1)
                ninth += int(tail and offset == 0 and (S - 34) & 1 == 1 and S + 16 == len(f))
        verify_same(fb, codes)
    assert align == set(range(16)) and parity == {0, 1} and ninth > 20


def test_tcp_data_offsets_and_icmp(ctx):
    frames = []
    for doff in (5, 8):
        H = 4 * doff
        for L in (46, 47, 34 + H + 15, 34 + H + 16, 34 + H + 17, 34 + H + 40):
            frames += [l4_frame(6, L, 10 * L + doff, doff=doff), l4_frame(1, L, 10 * L + doff + 1)]
    codes = codes_before(frames)
    fb, cap, off = prepared(ctx, frames)
    try:
        _, cnt = check_stamp(ctx, fb, cap, off)
        assert cnt["other"] == 0 and cnt["short"] >= 8 and cnt["stamped"] >= 8
        verify_same(fb, codes)
        _, cnt = check_stamp(ctx, fb, cap, off, offset=1, tail=True, first_index=77)
        verify_same(fb, codes)
    finally:
        fb.free()


def test_other_classes_stay_as_they_are(ctx):
    udp = l4_frame(17, 98, 1)
    others = [l4_frame(17, 98, 2, ethertype=b"\x86\xdd"), l4_frame(17, 98, 3, vihl=0x46), l4_frame(17, 98, 4, fo=0x2000),
              l4_frame(17, 98, 5, fo=0x00B9), l4_frame(47, 98, 6), l4_frame(6, 98, 7, doff=4), l4_frame(6, 47, 8, doff=0)]
    others += [udp[:L] for L in range(13, 34)]
    frames = []
    for f in others:  # each between two frames that are stamped
        frames += [l4_frame(17, 64, len(frames)), f]
    frames.append(l4_frame(1, 99, 9))
    fb, cap, off = prepared(ctx, frames)
    try:
        for tail in (False, True):
            _, cnt = check_stamp(ctx, fb, cap, off, tail=tail)
            assert cnt == dict(stamped=len(others) + 1, short=0, other=len(others))
    finally:
        fb.free()
    # a fixed length below 34 B: nothing is read, every frame is `other`
    short = [udp[:33]] * 70
    fb, cap, off = prepared(ctx, short, flen=33)
    try:
        assert check_stamp(ctx, fb, cap, off)[1] == dict(stamped=0, short=0, other=70)
    finally:
        fb.free()


# ------------------------------------------------------------------ 3. sub-ranges, the empty range
def test_subranges(ctx, var):
    fb, cap, off, frames = var
    for first, n in ((1, 1), (17, 300), (256, 257), (899, 1), (0, 899), (450, 450)):
        check_stamp(ctx, fb, cap, off, first=first, n=n, first_index=first * 3, offset=2)
    frames = [l4_frame(17, 65, j) for j in range(300)]
    fb, cap, off = prepared(ctx, frames, flen=65)
    try:
        for first in range(0, 17):  # the range's first byte at every alignment mod 16
            check_stamp(ctx, fb, cap, off, first=first, n=200, first_index=first, tail=True)
        verify_clean(fb)
    finally:
        fb.free()


def test_empty_range(ctx, var):
    fb, cap, off, _ = var
    for first in (0, 5, 900):
        assert check_stamp(ctx, fb, cap, off, first=first, n=0)[1] == dict(stamped=0, short=0, other=0)
    assert ctx.lib.pbgpu_stamp(ctx.h, fb.ptr, 0, 0, C.byref(StampOpts()), None) == 0


# ------------------------------------------------------------------ 4. refusals
def test_refusals(ctx):
    frames = [l4_frame(17, 98, j) for j in range(100)]
    fb, cap, off = prepared(ctx, frames, flen=98)
    never = ctx.alloc_frames(16, 1024)
    state = (meta(fb), fb.stream(cap).tobytes())
    ok = StampOpts(T0, STEP, 0, 0, 0)
    res = StampResult()

    def refused(frames_ptr, first, n, opts, h=ctx.h):
        assert ctx.lib.pbgpu_stamp(h, frames_ptr, first, n, opts, C.byref(res)) == EINVAL
        assert ctx.lib.pbgpu_stamp(h, frames_ptr, first, n, opts, None) == EINVAL
        assert (meta(fb), fb.stream(cap).tobytes()) == state

    try:
        refused(fb.ptr, 0, 100, C.byref(ok), h=None)
        refused(None, 0, 100, C.byref(ok))
        refused(fb.ptr, 0, 100, None)
        refused(never.ptr, 0, 0, C.byref(ok))  # never built or uploaded
        refused(fb.ptr, 1, 100, C.byref(ok))   # a range past n_frames
        refused(fb.ptr, 101, 0, C.byref(ok))
        refused(fb.ptr, 0, 1 << 63, C.byref(ok))
        for flags in (4, 8, 7, 1 << 31):
            refused(fb.ptr, 0, 100, C.byref(StampOpts(T0, STEP, 0, 0, flags)))
        refused(fb.ptr, 0, 100, C.byref(StampOpts(T0, STEP, 0, 65536, 0)))
        refused(fb.ptr, 0, 100, C.byref(StampOpts(T0, STEP, 0, 1 << 31, 1)))
        # the 64-bit rules of pbgpu_pcap_pack: the last index, its product with the step, the last timestamp
        refused(fb.ptr, 0, 2, C.byref(StampOpts(0, 0, 2**64 - 1, 0, 0)))
        refused(fb.ptr, 0, 100, C.byref(StampOpts(0, 1 << 40, (1 << 24) - 99, 0, 0)))
        refused(fb.ptr, 0, 2, C.byref(StampOpts(2**64 - 1, 1000, 0, 0, 0)))
        with pytest.raises(PbError) as e:
            fb.stamp(flags=4)
        assert e.value.code == EINVAL
        # the largest values that pass
        assert ctx.lib.pbgpu_stamp(ctx.h, fb.ptr, 0, 1, C.byref(StampOpts(0, 0, 2**64 - 1, 0, 0)), None) == 0
        assert ctx.lib.pbgpu_stamp(ctx.h, fb.ptr, 1, 2, C.byref(StampOpts(2**64 - 2, 1000, 0, 65535, 1)), C.byref(res)) == 0
        assert (res.n_in, res.n_stamped, res.n_short, res.n_other) == (2, 0, 2, 0)
        want = pystamp.stamp(frames[0], 2**64 - 1, 0)[0]
        assert fb.stream(98).tobytes() == want and fb.stream(cap - 98, 98).tobytes() == state[1][98:]
    finally:
        never.free()
        fb.free()


# ------------------------------------------------------------------ 5. built on the GPU
@pytest.mark.parametrize("cfg,n_iter", [("c2_udp_64", 4099), ("c4_tcp_syn", 4099), ("c5_icmp_echo", 1025),
                                        ("c3_udp_var", 3001)])
def test_built_on_the_gpu(ctx, cfg, n_iter):
    """A built buffer stamped (head, then tail over it), byte for byte against pystamp over the
    oracle's frames; the 60-B TCP SYN frames have no room and the buffer stays what it was."""
    seq = Sequence.from_config(pc.get(cfg))
    ctx.load_sequence(0, seq, pc.SEED_BASE)
    o_data, o_off = ob.build(seq, 0, 777, n_iter, pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n_iter))
    try:
        ctx.build(0, 777, n_iter, fb)
        m0 = meta(fb)
        res = fb.stamp(t0_ns=T0, step_ps=STEP, first_index=123456789)  # follows the build on the stream
        assert meta(fb) == m0
        want, cnt = pystamp.stamp_buffer(o_data.tobytes(), o_off, 0, None, T0, STEP, 123456789)
        assert fb.packed().tobytes() == want
        assert (int(res.n_stamped), int(res.n_short), int(res.n_other)) == (cnt["stamped"], cnt["short"], cnt["other"])
        n = len(o_off) - 1
        assert cnt == (dict(stamped=0, short=n, other=0) if cfg == "c4_tcp_syn" else dict(stamped=n, short=0, other=0))
        if cfg == "c4_tcp_syn":
            assert want == o_data.tobytes()
        assert np.array_equal(fb.offsets(), o_off)
        verify_clean(fb)
        res = fb.stamp(t0_ns=T0 + 1, step_ps=STEP, first_index=5, offset=3, tail=True)
        want2, cnt2 = pystamp.stamp_buffer(want, o_off, 0, None, T0 + 1, STEP, 5, 3, True)
        assert fb.packed().tobytes() == want2 and int(res.n_stamped) == cnt2["stamped"]
        verify_clean(fb)
    finally:
        fb.free()


# ------------------------------------------------------------------ 6. checksums
def test_no_csum_codes_follow_the_reference(ctx, var):
    """NO_CSUM leaves the checksum field: the GPU's verify codes then equal the reference's over the
    reference bytes, whatever share of the frames that makes bad."""
    _, _, _, frames = var
    fb, cap, off = prepared(ctx, frames)
    try:
        got, cnt = check_stamp(ctx, fb, cap, off, csum=False, first_index=0x010203040506)
        assert cnt["stamped"] > 200
        res, codes = fb.verify(codes=True)
        ref = vr.ref_codes(np.frombuffer(got, dtype=np.uint8), off)
        vr.expect(res, codes, ref)
        q = [pystamp.CSUM_AT[f[23]] for f in frames if pystamp.position(f)[0] == "stamped"]
        o = [int(off[j]) for j, f in enumerate(frames) if pystamp.position(f)[0] == "stamped"]
        before = b"".join(frames)
        assert all(got[a + b:a + b + 2] == before[a + b:a + b + 2] for a, b in zip(o, q))
    finally:
        fb.free()


def test_twice_with_different_options(ctx):
    frames = [l4_frame((17, 6, 1)[j % 3], 120 + j % 50, j) for j in range(600)]
    fb, cap, off = prepared(ctx, frames)
    try:
        check_stamp(ctx, fb, cap, off, first_index=10, offset=4)
        got, _ = check_stamp(ctx, fb, cap, off, t0_ns=5, step_ps=10**9, first_index=2**30, offset=9, tail=True)
        twice = pystamp.stamp_buffer(pystamp.stamp_buffer(b"".join(frames), off, 0, None, T0, STEP, 10, 4)[0], off, 0,
                                     None, 5, 10**9, 2**30, 9, True)[0]
        assert got[:len(twice)] == twice
        verify_clean(fb)
        assert all(frame_ok(got[int(off[j]):int(off[j + 1])]) for j in range(len(frames)))
    finally:
        fb.free()


# ------------------------------------------------------------------ 7. composition
def _stamped_frames(frames, **kw):
    data, off = pack(frames)
    out = pystamp.stamp_buffer(data.tobytes(), off, **kw)[0]
    return [out[int(off[j]):int(off[j + 1])] for j in range(len(frames))]


def test_then_fragment_encap_and_pcap(ctx):
    frames = [l4_frame(17, 3000 if j % 3 == 0 else 90 + j % 40, j) for j in range(300)]
    kw = dict(t0_ns=T0, step_ps=STEP, first_index=4242, offset=8)
    refs = _stamped_frames(frames, **kw)
    fb, cap, off = prepared(ctx, frames)
    dst = ctx.alloc_frames(1024, 1 << 20)
    try:
        check_stamp(ctx, fb, cap, off, **kw)
        # the fragments of one packet share one stamp: it is in the first
        fb.fragment(dst, mtu=1500)
        assert dst.frames() == pyfrag.fragment_all(refs, 1500)[0]
        fb.encap(dst, mode=pbgpu.ENCAP_VLAN, tci=0x2064)
        assert dst.frames() == [pyencap.vlan(f, 0x2064) for f in refs]
        # the pcap stream with the same three values: every record's timestamp is its frame's T
        raw = fb.pcap_bytes(t0_ns=T0, step_ps=STEP, first_index=4242, nsec=True).tobytes()
        assert raw == pypcap.pcap_stream(refs, T0, STEP, 4242, nsec=True)
        nsec, recs = pypcap.read_pcap(raw)
        assert nsec and len(recs) == 300
        for j, (sec, frac, f) in enumerate(recs):
            idx, T = np.frombuffer(f[50:66], dtype=">u8")
            assert int(idx) == 4242 + j and (int(T) // 10**9 % 2**32, int(T) % 10**9) == (sec, frac)
    finally:
        dst.free()
        fb.free()


def test_follows_a_queued_landing(ctx):
    """The stamp is a writer: a landing queued from the buffer gets the unstamped frames, one queued
    after the stamp the stamped ones."""
    n, L, slot = 4096, 98, 256
    frames = [l4_frame(17, L, j) for j in range(n)]
    refs = _stamped_frames(frames, t0_ns=T0, step_ps=STEP, first_index=9)
    lib = ctx.lib
    lib.pbgpu_copy_to_umem_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64,
                                             C.c_uint32, C.POINTER(C.c_uint16)]
    lib.pbgpu_land_wait.argtypes = [C.c_void_p, C.c_uint32]
    fb, cap, off = prepared(ctx, frames, flen=L)
    umem = np.zeros(slot * n, dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint16)
    assert lib.pbgpu_host_register(ctx.h, umem.ctypes.data, umem.nbytes) == 0
    try:
        assert lib.pbgpu_copy_to_umem_async(ctx.h, fb.ptr, umem.ctypes.data, slot, 0, 0, n,
                                            lens.ctypes.data_as(C.POINTER(C.c_uint16))) == 0
        res = fb.stamp(t0_ns=T0, step_ps=STEP, first_index=9)  # the landing is queued, not waited for
        assert int(res.n_stamped) == n
        assert lib.pbgpu_land_wait(ctx.h, 0) == 0
        assert (lens == L).all()
        assert umem.reshape(n, slot)[:, :L].tobytes() == b"".join(frames)
        lens2 = fb.to_umem(umem, slot, 0, n)
        assert (lens2 == L).all()
        assert umem.reshape(n, slot)[:, :L].tobytes() == b"".join(refs)
        assert fb.stream(n * L).tobytes() == b"".join(refs)
    finally:
        lib.pbgpu_host_unregister(ctx.h, umem.ctypes.data)
        fb.free()
