"""Taking over a destination buffer (take_dst in pbgpu.cpp): an upload, a pcap pack, an encapsulation
and a fragmentation into a buffer that another stream is still building, or that a queued landing is
still reading.  Span timing with per-sequence streams: sequence 1 (c4_tcp_syn) builds on a stream of
its own, the four transforms run on the context's.

What this is: it runs the hop from the buffer's last writer and the wait for the queued landing, and
checks every byte that comes out against the Python references and a build into a fresh buffer.
What it is not: a proof of the ordering.  A missing wait could still pass by timing; the test pins
that the path works."""
import ctypes as C

import numpy as np
import pytest

import pb_configs as pc
import pyencap
import pyfrag
import pypcap
from pbgpu import ENCAP_VXLAN, EncapOpts, GpuContext, Sequence

pytestmark = pytest.mark.gpu

N = 4096
VX = dict(dst_mac=bytes.fromhex("0200000000a2"), src_mac=bytes.fromhex("0200000000a1"), src_ip=bytes([192, 0, 2, 1]),
          dst_ip=bytes([198, 51, 100, 2]), vni=0x123456)
SLOTS = {0: "c2_udp_64", 1: "c4_tcp_syn", 4: "udp_jumbo_fixed_odd"}  # 0 and 4 share a stream, 1 has another


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    c.set_timing(c.TIMING_SPAN)
    for slot, name in SLOTS.items():
        c.load_sequence(slot, Sequence.from_config(pc.get(name)), pc.SEED_BASE)
    yield c
    c.close()


def _frames(fb):
    data, flen = fb.packed(), int(fb.f.fixed_len)
    return [bytes(data[i * flen:(i + 1) * flen]) for i in range(int(fb.f.n_frames))]


@pytest.fixture(scope="module")
def world(ctx):
    """The two sources, sequence 1's frames from a build into a fresh buffer, the destination D and
    the four transforms with their reference bytes; computed once."""
    src = ctx.alloc_frames(*ctx.build_size(0, N))
    ctx.build(0, 0, N, src)
    jumbo = ctx.alloc_frames(*ctx.build_size(4, 64))
    ctx.build(4, 0, 64, jumbo)
    fresh = ctx.alloc_frames(*ctx.build_size(1, N))
    ctx.build(1, 0, N, fresh)
    ctx.sync()
    f64, fj, syn = _frames(src), _frames(jumbo), _frames(fresh)
    fresh.free()
    raw = b"".join(f64)
    opts = EncapOpts.make(ENCAP_VXLAN, **VX)
    D = ctx.alloc_frames(16384, 4 << 20)
    runs = {
        "upload": (lambda: D.upload(raw, fixed_len=64), raw),
        "pcap": (lambda: src.pcap_pack(D, t0_ns=5, step_ps=672000), bytes(pypcap.pcap_stream(f64, 5, 672000))),
        "encap": (lambda: src.encap(D, opts=opts), b"".join(pyencap.vxlan(f, **VX) for f in f64)),
        "fragment": (lambda: jumbo.fragment(D, mtu=1500), b"".join(pyfrag.fragment_all(fj, 1500)[0])),
    }
    yield dict(D=D, syn=syn, runs=runs)
    for fb in (src, jumbo, D):
        fb.free()


def _same(got, want):
    return np.array_equal(got, np.frombuffer(want, dtype=np.uint8))


CASES = ["upload", "pcap", "encap", "fragment"]


@pytest.mark.parametrize("what", CASES)
def test_transform_follows_a_build_on_another_stream(ctx, world, what):
    D, (run, ref), syn = world["D"], world["runs"][what], b"".join(world["syn"])
    ctx.build(1, 0, N, D)  # on sequence 1's stream, not waited for
    run()
    assert _same(D.stream(len(ref)), ref)
    ctx.build(1, 0, N, D)  # and back: the build follows the transform
    ctx.sync()
    assert _same(D.stream(len(syn)), syn)


@pytest.mark.parametrize("what", CASES)
def test_transform_waits_for_the_queued_landing(ctx, world, what):
    D, (run, ref), syn = world["D"], world["runs"][what], world["syn"]
    lib = ctx.lib
    lib.pbgpu_copy_to_umem_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64,
                                             C.c_uint32, C.POINTER(C.c_uint16)]
    lib.pbgpu_land_wait.argtypes = [C.c_void_p, C.c_uint32]
    umem = np.zeros(4096 * N, dtype=np.uint8)
    lens = np.zeros(N, dtype=np.uint16)
    assert lib.pbgpu_host_register(ctx.h, umem.ctypes.data, umem.nbytes) == 0
    try:
        ctx.build(1, 0, N, D)
        assert lib.pbgpu_copy_to_umem_async(ctx.h, D.ptr, umem.ctypes.data, 4096, 0, 0, N,
                                            lens.ctypes.data_as(C.POINTER(C.c_uint16))) == 0
        run()  # the landing is queued, not waited for
        assert lib.pbgpu_land_wait(ctx.h, 0) == 0
        L = len(syn[0])
        assert (lens == L).all()
        assert _same(umem.reshape(N, 4096)[:, :L].reshape(-1), b"".join(syn))  # D's old frames
        assert _same(D.stream(len(ref)), ref)
    finally:
        lib.pbgpu_host_unregister(ctx.h, umem.ctypes.data)
