"""The UMEM landing (pbgpu_copy_to_umem[_async], pbgpu_land_wait) byte by byte against tests/pyland.py.

Every frame here is uploaded, so its length and bytes are the test's own (pyland.frame_bytes: a hash
of frame index and byte position).  The whole UMEM array is prefilled, landed into and compared whole
with the model: the guard slots in front of and behind the landed ones and the bytes in front of the
base included.  Every case runs with two prefill bytes, so a store that never happened cannot hide
behind a frame byte equal to the fill.  Every landing stays inside the array: `bounded` asserts it
before each call.  Run on the MI355X box: pytest -m gpu."""
import ctypes as C
import os
from contextlib import contextmanager

import numpy as np
import pytest

import pb_configs as pc
import pbgpu
import pyland as pl
from pbgpu import GpuContext, Sequence

pytestmark = pytest.mark.gpu

EINVAL = -22
FILLS = (0xEE, 0x11)
GUARD = 2  # untouched slots in front of the landed ones; as many behind


def _bind(lib):
    lib.pbgpu_copy_to_umem_async.restype = C.c_int
    lib.pbgpu_copy_to_umem_async.argtypes = [C.c_void_p, C.POINTER(pbgpu.Frames), C.c_void_p, C.c_uint32, C.c_uint32,
                                             C.c_uint64, C.c_uint32, C.c_void_p]
    lib.pbgpu_land_wait.restype = C.c_int
    lib.pbgpu_land_wait.argtypes = [C.c_void_p, C.c_uint32]
    return lib


@contextmanager
def opened(**env):
    """A context of its own, opened under the given environment (read at pbgpu_open only)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = GpuContext(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    _bind(c.lib)
    try:
        yield c
    finally:
        c.close()


@contextmanager
def registered(c, arr):
    assert c.lib.pbgpu_host_register(c.h, arr.ctypes.data, arr.nbytes) == 0
    try:
        yield arr
    finally:
        assert c.lib.pbgpu_host_unregister(c.h, arr.ctypes.data) == 0


@pytest.fixture(scope="module")
def ctx():
    with opened() as c:
        yield c


@pytest.fixture(scope="module")
def umem_reg(ctx):
    """8 MiB registered with the module's context; the tests land into views of it."""
    with registered(ctx, np.zeros(8 << 20, dtype=np.uint8)) as arr:
        yield arr


@pytest.fixture(scope="module")
def umem_plain():
    return np.zeros(8 << 20, dtype=np.uint8)


def bounded(umem, stride, first_slot, n, base):
    """The landing's slots lie inside the array it was given."""
    assert base >= 0 and first_slot >= 0 and base + (first_slot + n) * stride <= umem.nbytes


def land_rc(c, fb, umem, stride, first_slot, first_frame, n, base=0, lens=None, sync=True):
    bounded(umem, stride, first_slot, n, base)
    fn = c.lib.pbgpu_copy_to_umem if sync else c.lib.pbgpu_copy_to_umem_async
    p = C.cast(lens.ctypes.data, C.POINTER(C.c_uint16) if sync else C.c_void_p) if lens is not None else None
    return fn(c.h, fb.ptr, umem.ctypes.data + base, stride, first_slot, first_frame, n, p)


def upload_var(c, lengths, capacity_bytes=None):
    frames = [pl.frame_bytes(j, ln) for j, ln in enumerate(lengths)]
    data = np.concatenate(frames) if frames else np.zeros(0, dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    fb = c.alloc_frames(len(lengths), len(data) if capacity_bytes is None else capacity_bytes)
    fb.upload(data, offsets=off)
    return fb, frames, data


def upload_fixed(c, flen, n, capacity_bytes=None):
    frames = [pl.frame_bytes(j, flen) for j in range(n)]
    data = np.concatenate(frames)
    fb = c.alloc_frames(n, len(data) + 64 if capacity_bytes is None else capacity_bytes)
    fb.upload(data, fixed_len=flen)
    return fb, frames, data


# ---- a. variable length: every length against every source and destination alignment ----

@pytest.fixture(scope="module")
def var_set():
    lengths, blocks = pl.var_blocks()
    return lengths, blocks, [pl.frame_bytes(j, ln) for j, ln in enumerate(lengths)]


def run_var(c, umem_all, var_set, stride):
    lengths, blocks, frames = var_set
    fb, _, _ = upload_var(c, lengths)
    n_slots = GUARD + len(lengths) + GUARD
    cases = 0
    try:
        for base in (0, 1, 2, 3):
            umem = umem_all[:base + n_slots * stride]
            for fill in FILLS:
                umem[:] = fill
                want = umem.copy()
                for first, n in blocks:  # block k into the slots of its frames: sub-ranges, first_frame > 0
                    lens = np.full(n, 0xFFFF, dtype=np.uint16)
                    assert land_rc(c, fb, umem, stride, GUARD + first, first, n, base, lens) == 0
                    want, want_lens = pl.land(want, frames, stride, GUARD + first, first, n, base=base)
                    assert np.array_equal(lens, want_lens)
                    cases += n
                assert np.array_equal(umem, want), (stride, base, fill, np.flatnonzero(umem != want)[:8])
    finally:
        fb.free()
    return cases


@pytest.mark.parametrize("stride", pl.VAR_STRIDES)
def test_variable_lengths_registered(ctx, umem_reg, var_set, stride):
    """pb_scatter_slots over the host link: lengths 0..80 and the long ones at every source offset
    mod 16, slots at every destination offset mod 4 (base, and strides that are no multiple of 4)."""
    assert run_var(ctx, umem_reg, var_set, stride) == 2 * 4 * 16 * 89


@pytest.mark.parametrize("stride", pl.VAR_STRIDES)
def test_variable_lengths_unregistered(ctx, umem_plain, var_set, stride):
    """land_unmapped's staging copy, every landing with first_frame > 0."""
    assert run_var(ctx, umem_plain, var_set, stride) == 2 * 4 * 16 * 89


def test_variable_lengths_umem_dma(umem_plain, var_set):
    """PBGPU_UMEM_DMA=1: registered memory lands through the staging copy too."""
    with opened(PBGPU_UMEM_DMA="1") as c, registered(c, umem_plain):
        for stride in pl.VAR_STRIDES:
            assert run_var(c, umem_plain, var_set, stride) == 2 * 4 * 16 * 89


# ---- b, c. fixed length: odd lengths, every stride class, the three paths ----

def run_fixed(c, umem_all, flen, whole_path):
    """Every (capacity, stride, range, base, fill) of the fixed-length set for one frame length; whole_path:
    tight slots are written whole (registered memory, scatter kernel).  -> landings made.
    Of a whole slot only filler at or past the buffer's total is unspecified (pyland.check_cap: at most
    stride - flen <= 63 bytes of a slot), and even that is held to the buffer's own byte or zero."""
    n = pl.FIXED_N
    total = n * flen
    landings = 0
    for cap in (None, total):  # roomy, then capacity_bytes == round16(total) exactly
        fb, frames, stream = upload_fixed(c, flen, n, cap)
        try:
            cap_bytes = int(fb.f.capacity_bytes)
            assert cap is None or cap_bytes == (total + 15) & ~15
            pad = fb.stream(cap_bytes - total, total)  # what lies behind the frames in the buffer
            for stride in pl.fixed_strides(flen):
                whole = whole_path and pl.is_tight(flen, stride)
                for first, cnt in pl.fixed_ranges(n):
                    for base in pl.FIXED_BASES:
                        umem = umem_all[:base + (GUARD + cnt + GUARD) * stride]
                        for fill in FILLS:
                            umem[:] = fill
                            lens = np.full(cnt, 0xFFFF, dtype=np.uint16)
                            assert land_rc(c, fb, umem, stride, GUARD, first, cnt, base, lens) == 0
                            landings += 1
                            assert (lens == flen).all()
                            m = pl.land(np.full(umem.nbytes, fill, dtype=np.uint8), frames, stride, GUARD, first, cnt,
                                        base=base, whole=whole, stream=stream)
                            where = (flen, cap, stride, first, cnt, base, fill)
                            if not whole:
                                assert np.array_equal(umem, m[0]), (where, np.flatnonzero(umem != m[0])[:8])
                                continue
                            want, _, mask = m
                            pl.check_cap(mask, flen, stride, GUARD, first, cnt, base, total)
                            assert np.array_equal(umem[~mask], want[~mask]), \
                                (where, np.flatnonzero((umem != want) & ~mask)[:8])
                            # filler past the frames: the buffer's own byte there, or zero; zero past the
                            # buffer; so never the prefill left standing
                            at = np.flatnonzero(mask)
                            pos = pl.stream_pos(at, flen, stride, GUARD, first, base) - total
                            got = umem[at]
                            inside = pos < len(pad)
                            ok = got == 0
                            ok[inside] |= got[inside] == pad[pos[inside]]
                            assert ok.all(), (where, at[~ok][:8], got[~ok][:8])
        finally:
            fb.free()
    return landings


N_FIXED_LANDINGS = {flen: 2 * len(pl.fixed_strides(flen)) * 3 * 2 * 2 for flen in pl.FIXED_LENS}


@pytest.mark.parametrize("flen", pl.FIXED_LENS)
def test_fixed_lengths_scatter_kernel(ctx, umem_reg, flen):
    """pb_scatter_fixed into registered memory: the byte tail with flen % 4 of 1, 2 and 3, strides and
    bases that are no multiple of 4, tight slots up to round64(flen) whole and round64(flen) + 1 not,
    and the end of the stream in a buffer of exactly round16(total) bytes."""
    assert run_fixed(ctx, umem_reg, flen, True) == N_FIXED_LANDINGS[flen]


@pytest.fixture(scope="module")
def dma_ctx():
    with opened(PBGPU_LAND_DMA_MIN="1") as c:
        yield c


@pytest.mark.parametrize("flen", pl.FIXED_LENS)
def test_fixed_lengths_dma_engine(dma_ctx, umem_plain, flen):
    """PBGPU_LAND_DMA_MIN=1: registered memory through the strided DMA, which writes the frame only."""
    with registered(dma_ctx, umem_plain):
        assert run_fixed(dma_ctx, umem_plain, flen, False) == N_FIXED_LANDINGS[flen]


@pytest.mark.parametrize("flen", pl.FIXED_LENS)
def test_fixed_lengths_unregistered(ctx, umem_plain, flen):
    assert run_fixed(ctx, umem_plain, flen, False) == N_FIXED_LANDINGS[flen]


# ---- d. the queue and the lens ring ----

def test_queue_and_lens_ring(umem_reg):
    """One context's lens ring through its wrap at 65536 entries with landings queued, fixed-length
    landings (some without lens_out) in between, land_wait(keep) with keep = 3, and the ring
    regrown for a 70000-frame landing while two landings are queued."""
    with opened() as c:
        L = c.lib
        rng = np.random.default_rng(5)
        v_len = rng.integers(40, 91, 3200).tolist()
        vb, v_frames, _ = upload_var(c, v_len)
        xb, x_frames, _ = upload_fixed(c, 60, 500)  # 60 B in 128-B slots: not tight
        big_len = rng.integers(60, 81, 70000).tolist()
        bb, b_frames, _ = upload_var(c, big_len)
        stride = 128
        umem = umem_reg[:(29 * 1000 + 3200 + GUARD) * stride]
        umem[:] = 0xEE
        want = umem.copy()
        try:
            queued = []  # (lens_out or None, expected lens), oldest first

            def queue(fb, frames, first_slot, first, n, with_lens=True, um=umem, st=stride):
                lens = np.full(n, 0xFFFF, dtype=np.uint16) if with_lens else None
                assert land_rc(c, fb, um, st, first_slot, first, n, 0, lens, sync=False) == 0
                queued.append((lens, frames, st, first_slot, first, n))

            def check_done(upto):
                for lens, frames, st, first_slot, first, n in queued[:max(0, upto)]:
                    if lens is not None:
                        assert np.array_equal(lens, [len(f) for f in frames[first:first + n]])

            entries = 0
            for i in range(30):
                first, n = (i * 37) % 180, 3000 + (i % 5) * 5 - 10
                queue(vb, v_frames, GUARD + i * 1000, first, n)
                entries += n
                if i % 3 == 1:
                    queue(xb, x_frames, GUARD + i * 1000 + 17, i, 400 + i, with_lens=i % 2 == 0)
                assert L.pbgpu_land_wait(c.h, 3) == 0
                check_done(len(queued) - 3)
            assert entries >= 90000 - 30 * 10 > 65536
            assert L.pbgpu_land_wait(c.h, 0) == 0
            check_done(len(queued))
            for lens, frames, st, first_slot, first, n in queued:  # one stream: they landed in this order
                want, _ = pl.land(want, frames, st, first_slot, first, n)
            assert np.array_equal(umem, want), np.flatnonzero(umem != want)[:8]

            # regrow: n > the ring's capacity with two landings queued
            del queued[:]
            small = umem_reg[:1 << 20]
            big = umem_reg[1 << 20:(1 << 20) + (GUARD + 70000 + GUARD) * 80]  # 80-B slots: Lmax
            small[:] = 0x11
            big[:] = 0x11
            queue(vb, v_frames, GUARD, 5, 3000, um=small)
            queue(vb, v_frames, GUARD + 3100, 100, 3100, um=small)
            queue(bb, b_frames, GUARD, 0, 70000, um=big, st=80)
            assert L.pbgpu_land_wait(c.h, 0) == 0
            check_done(3)
            want = np.full(small.nbytes, 0x11, dtype=np.uint8)
            for lens, frames, st, first_slot, first, n in queued[:2]:
                want, _ = pl.land(want, frames, st, first_slot, first, n)
            assert np.array_equal(small, want)
            want, _ = pl.land(np.full(big.nbytes, 0x11, dtype=np.uint8), b_frames, 80, GUARD, 0, 70000)
            assert np.array_equal(big, want), np.flatnonzero(big != want)[:8]
        finally:
            assert L.pbgpu_land_wait(c.h, 0) == 0
            for fb in (vb, xb, bb):
                fb.free()


# ---- e. refusals ----

def test_refusals_leave_the_umem_alone(ctx, umem_reg, umem_plain):
    L = ctx.lib
    vb, _, _ = upload_var(ctx, [40, 90, 64, 1, 0, 77])  # Lmax = 90
    xb, _, _ = upload_fixed(ctx, 61, 10)
    try:
        for umem_all in (umem_reg, umem_plain):
            umem = umem_all[:1 << 16]
            umem[:] = 0xEE
            lens = np.full(16, 0xFFFF, dtype=np.uint16)
            lp = C.cast(lens.ctypes.data, C.POINTER(C.c_uint16))
            u = umem.ctypes.data
            assert L.pbgpu_copy_to_umem(None, vb.ptr, u, 128, 0, 0, 6, lp) == EINVAL
            assert L.pbgpu_copy_to_umem(ctx.h, None, u, 128, 0, 0, 6, lp) == EINVAL
            assert L.pbgpu_copy_to_umem(ctx.h, vb.ptr, None, 128, 0, 0, 6, lp) == EINVAL
            assert L.pbgpu_copy_to_umem_async(None, vb.ptr, u, 128, 0, 0, 6, lens.ctypes.data) == EINVAL
            for fb, n_frames, too_short in ((vb, 6, 89), (xb, 10, 60)):
                assert land_rc(ctx, fb, umem, 0, 0, 0, n_frames, 0, lens) == EINVAL       # slot_stride == 0
                assert land_rc(ctx, fb, umem, 128, 0, 1, n_frames, 0, lens) == EINVAL     # a range past n_frames
                assert land_rc(ctx, fb, umem, 128, 0, n_frames + 1, 0, 0, lens) == EINVAL
                assert land_rc(ctx, fb, umem, too_short, 0, 0, n_frames, 0, lens) == EINVAL  # Lmax - 1, flen - 1
                assert land_rc(ctx, fb, umem, too_short, 0, 0, n_frames, 0, lens, sync=False) == EINVAL
                # the short frames of a refused buffer do not land either
                assert land_rc(ctx, fb, umem, too_short, 0, 0, 1, 0, lens) == EINVAL
                assert land_rc(ctx, fb, umem, 128, 3, 2, 0, 0, lens) == 0                 # n == 0: nothing to do
                assert land_rc(ctx, fb, umem, 128, 3, n_frames, 0, 0, lens) == 0
            assert L.pbgpu_land_wait(ctx.h, 0) == 0
            assert L.pbgpu_land_wait(None, 0) == EINVAL
            assert (umem == 0xEE).all() and (lens == 0xFFFF).all()
            # and the slot that just fits is taken
            assert land_rc(ctx, vb, umem, 90, 1, 0, 6, 0, lens) == 0
            assert lens[:6].tolist() == [40, 90, 64, 1, 0, 77]
    finally:
        vb.free()
        xb.free()


# ---- f. the slot check uses the buffer's own lengths, not the sequence slot's ----

def var_cfg(lo, hi):
    """c3_udp_var with payloads of lo..hi bytes: frames of 42 + lo .. 42 + hi."""
    c = pc.get("c3_udp_var")
    c["payloads"] = [{"length": {"min": lo, "max": hi}}]
    return c


@pytest.mark.parametrize("is_registered", [True, False], ids=["registered", "unregistered"])
def test_reloading_the_sequence_slot_does_not_change_the_check(ctx, umem_reg, umem_plain, is_registered):
    """Frames of 106..300 B (c3_udp_var with 64..258-B payloads) built from sequence slot 12, the slot
    then reloaded with c2_udp_64: 128-B slots are still refused, with nothing written.  The other way
    round, 42..64-B frames still land in 64-B slots after c2_udp_1500 took the sequence slot.  The
    array is 8 MiB, at least 8 * 128 + 4096 bytes, and the landing starts at slot 0: eight 300-B frames
    in 128-B slots would end at byte 7 * 128 + 300."""
    s = 12
    umem = (umem_reg if is_registered else umem_plain)[:1 << 16]
    assert umem.nbytes >= 8 * 128 + 4096
    ctx.load_sequence(s, Sequence.from_config(var_cfg(64, 258)), pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(s, 64))
    sb = ctx.alloc_frames(*ctx.build_size(s, 64))
    eb = ctx.alloc_frames(64, 64 * 304 + 16)
    try:
        ctx.build(s, 3, 64, fb)
        ctx.sync()
        long_frames = [np.frombuffer(f, dtype=np.uint8) for f in fb.frames()]
        assert 128 < max(len(f) for f in long_frames[:8]) <= 300
        fb.encap(eb, mode=pbgpu.ENCAP_VLAN, tci=5)
        tagged = [np.frombuffer(f, dtype=np.uint8) for f in eb.frames()]
        assert [len(f) for f in tagged] == [len(f) + 4 for f in long_frames]

        ctx.load_sequence(s, Sequence.from_config(pc.get("c2_udp_64")), pc.SEED_BASE)
        for fill in FILLS:
            umem[:] = fill
            lens = np.full(8, 0xFFFF, dtype=np.uint16)
            for sync in (True, False):
                assert land_rc(ctx, fb, umem, 128, 0, 0, 8, 0, lens, sync=sync) == EINVAL
                assert ctx.lib.pbgpu_land_wait(ctx.h, 0) == 0
                assert (umem == fill).all() and (lens == 0xFFFF).all()
            # the encapsulated copy carries its own lengths: refused below its longest frame, taken at it
            assert land_rc(ctx, eb, umem, 128, 0, 0, 8, 0, lens) == EINVAL
            assert (umem == fill).all() and (lens == 0xFFFF).all()
            lens = np.full(64, 0xFFFF, dtype=np.uint16)
            assert land_rc(ctx, eb, umem, 304, GUARD, 0, 64, 1, lens) == 0
            want, want_lens = pl.land(np.full(umem.nbytes, fill, dtype=np.uint8), tagged, 304, GUARD, 0, 64, base=1)
            assert np.array_equal(lens, want_lens) and np.array_equal(umem, want)
            # and the built buffer still lands where its frames fit
            umem[:] = fill
            assert land_rc(ctx, fb, umem, 300, GUARD, 0, 64, 0, lens) == 0
            want, want_lens = pl.land(np.full(umem.nbytes, fill, dtype=np.uint8), long_frames, 300, GUARD, 0, 64)
            assert np.array_equal(lens, want_lens) and np.array_equal(umem, want)

        # the reverse: short frames, the slot reloaded with a longer sequence
        ctx.load_sequence(s, Sequence.from_config(var_cfg(0, 22)), pc.SEED_BASE)
        ctx.build(s, 9, 64, sb)
        ctx.sync()
        short_frames = [np.frombuffer(f, dtype=np.uint8) for f in sb.frames()]
        assert max(len(f) for f in short_frames) <= 64
        ctx.load_sequence(s, Sequence.from_config(pc.get("c2_udp_1500")), pc.SEED_BASE)
        for fill in FILLS:
            umem[:] = fill
            lens = np.full(64, 0xFFFF, dtype=np.uint16)
            assert land_rc(ctx, sb, umem, 64, GUARD, 0, 64, 0, lens) == 0
            want, want_lens = pl.land(np.full(umem.nbytes, fill, dtype=np.uint8), short_frames, 64, GUARD, 0, 64)
            assert np.array_equal(lens, want_lens) and np.array_equal(umem, want)
    finally:
        for b in (fb, sb, eb):
            b.free()
