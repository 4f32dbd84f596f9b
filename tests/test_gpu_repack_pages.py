"""The five repack writers (pcap pack, encap, fragment, segment, xlat46) with several 4-KiB pages per
workgroup.  page_grid() gives a workgroup more than one page only from 32,768 output pages (128 MiB)
on, so every other byte-exact test of these writers runs their page loops exactly once.  Here
PBGPU_RP_PER forces 2, 3 and 32 pages per workgroup at outputs of a few MB, and each writer's own
check helper compares the whole destination as it does in its own test file: every byte against the
Python definition, the pad, the slack, the counters, the metadata, the offsets and the source.

The cases are repack_cases.CASES; test_repack_pages_cpu.py shows without a GPU that they reach the
window moves, the carried pages, the pages without a record start and the ragged ends.  One run per
writer at the smallest natural size with 2 pages per workgroup ties the forced shape to the rule."""
import ctypes as C

import numpy as np
import pytest

import pb_configs as pc
import pyfrag
import pypcap
import pyseg
import repack_cases as rc
import test_gpu_encap as tge
import test_gpu_frag as tgf
import test_gpu_pcap as tgp
import test_gpu_seg as tgs
import test_gpu_xlat as tgx
from pbgpu import EncapOpts, GpuContext, Sequence
from repack_cases import CASES, PAGE, PERS, case_geometry, case_id, source

pytestmark = pytest.mark.gpu

FORCED = (1, 2, 3, 4, 5, 8, 13, 16, 31, 32)
IGNORED = ("0", "33", "64", "-3", "x", "")


def rule(npages, forced=0):
    """page_grid() as pbgpu.cpp states it: npages / 16384 clamped to 1..32, or the forced value; more
    where the grid would pass 2^24."""
    per = forced or min(max(npages // 16384, 1), 32)
    if -(-npages // per) > 1 << 24:
        per = (npages + (1 << 24) - 1) >> 24
    return per, -(-npages // per)


def opened(mp, value):
    """A context opened with PBGPU_RP_PER = value (None: unset); the options are read at pbgpu_open."""
    if value is None:
        mp.delenv("PBGPU_RP_PER", raising=False)
    else:
        mp.setenv("PBGPU_RP_PER", str(value))
    return GpuContext(0)


@pytest.fixture(scope="module")
def ctxs():
    """A context per pages-per-workgroup value, the default one under None; the environment is put
    back before the first test runs."""
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        for per in (None, 1) + PERS:
            out[per] = opened(mp, per)
    yield out
    for c in out.values():
        c.close()


def _memo(fn, key):
    cache = {}

    def wrapped(*a, **kw):
        k = key(*a) + tuple(sorted(kw.items()))
        if k not in cache:
            cache[k] = fn(*a, **kw)
        return cache[k]

    return wrapped


@pytest.fixture(scope="module", autouse=True)
def references_once():
    """The check helpers compute their reference on every call; here each is computed once per (frames,
    options) and shared by the runs at 2, 3 and 32 pages per workgroup."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(pyseg, "segment_all", _memo(pyseg.segment_all, lambda fr, *a: (tuple(fr),) + a))
        mp.setattr(pyfrag, "fragment_all", _memo(pyfrag.fragment_all, lambda fr, *a: (tuple(fr),) + a))
        mp.setattr(pypcap, "pcap_stream", _memo(pypcap.pcap_stream, lambda fr, *a: (tuple(fr),) + a))
        mp.setattr(tge, "ref_frame", _memo(tge.ref_frame, lambda f, mode, fields: (f, mode, tuple(sorted(fields.items())))))
        mp.setattr(tgx, "ref_frames", _memo(tgx.ref_frames, lambda fr, o: (tuple(fr), o)))
        yield


# ------------------------------------------------------------------ 1. the launch shape
def test_page_grid_follows_the_rule(ctxs):
    ctx = ctxs[None]
    table = [(1, 1), (16383, 1), (32767, 1), (32768, 2), (49151, 2), (49152, 3), (524288, 32), (1 << 29, 32),
             ((1 << 29) + 1, 33)]
    for npages, per in table:
        got = ctx.page_grid(npages)
        assert got == (per, -(-npages // per)) == rule(npages), npages
    assert ctx.page_grid(1 << 29)[1] == 1 << 24 and ctx.page_grid((1 << 29) + 1)[1] <= 1 << 24
    for npages in (0, 2, 16384, 65535, 65536, 524287, (1 << 29) - 1, 1 << 40, 1 << 55):
        assert ctx.page_grid(npages) == rule(npages), npages
    per, grid = C.c_uint32(), C.c_uint32()
    assert ctx.lib.pbgpu_page_grid(ctx.h, 1 << 57, C.byref(per), C.byref(grid)) == -22  # per would pass 32 bits
    assert ctx.lib.pbgpu_page_grid(None, 1, C.byref(per), C.byref(grid)) == -22
    assert ctx.lib.pbgpu_page_grid(ctx.h, 1, None, C.byref(grid)) == -22
    assert ctx.lib.pbgpu_page_grid(ctx.h, 1, C.byref(per), None) == -22


def test_page_grid_forced(ctxs, monkeypatch):
    sizes = (1, 2, 31, 33, 1000, 16384, 32768, 524288, 1 << 24, (1 << 24) + 1, 1 << 29, (1 << 29) + 1)
    for k in (1,) + PERS:
        for npages in sizes:
            assert ctxs[k].page_grid(npages) == rule(npages, k), (k, npages)
    assert ctxs[1].page_grid((1 << 24) + 1) == (2, (1 << 23) + 1)  # the grid cap on top of a forced value
    for k in FORCED:
        ctx = opened(monkeypatch, k)
        try:
            assert [ctx.page_grid(n) for n in sizes] == [rule(n, k) for n in sizes], k
            assert ctx.page_grid(100 * k)[0] == k
        finally:
            ctx.close()
    for v in IGNORED:
        ctx = opened(monkeypatch, v)
        try:
            assert [ctx.page_grid(n) for n in sizes] == [rule(n) for n in sizes], v
        finally:
            ctx.close()
    # read at pbgpu_open: a context already open keeps what it read
    monkeypatch.setenv("PBGPU_RP_PER", "7")
    assert ctxs[None].page_grid(1000) == (1, 1000) and ctxs[32].page_grid(1000) == (32, 32)


# ------------------------------------------------------------------ 2. whole outputs at 2, 3 and 32 pages
def check(ctx, c, fb, frames, first, n):
    o = rc.OPTS[c.writer][c.oname]
    if c.writer == "pcap":
        tgp.check_pack(ctx, fb, frames, first, n, **o)
    elif c.writer == "encap":
        tge.check_encap(ctx, fb, frames, *o, first=first, n=n)
    elif c.writer == "frag":
        tgf.check_frag(ctx, fb, frames, *o, first=first, n=n)
    elif c.writer == "seg":
        tgs.check_seg(ctx, fb, frames, *o, first=first, n=n)
    else:
        tgx.check_xlat(ctx, fb, frames, o, first=first, n=n, scratch=False)  # check6: test_repack_pages_cpu.py


@pytest.mark.parametrize("case,per", [(c, per) for c in CASES for per in c.pers],
                         ids=lambda v: case_id(v) if isinstance(v, rc.Case) else "per%d" % v)
def test_whole_output(ctxs, case, per):
    ctx = ctxs[per]
    frames, flen, first, n = source(case)
    g = case_geometry(case, per)
    assert ctx.page_grid(g.npages) == (per, g.grid) and g.grid >= 2
    data, off = tgs.pack(frames)
    fb = tgs.uploaded(ctx, data, flen=flen) if flen else tgs.uploaded(ctx, data, off=off)
    try:
        check(ctx, case, fb, frames, first, n)
    finally:
        fb.free()


# ------------------------------------------------------------------ 3. the natural size
N_BUILT = 170_000  # frames of 824 B on average: 128 MiB are about 160,000 of them
VX = EncapOpts.make(tge.MODES["vxlan"][0], **tge.MODES["vxlan"][1])
XO = tgx.mkopts(tgx.OPTS["hash"])
# writer: (its size call's output bytes of frames [0, n), the call itself returning its counters)
NATURAL = {
    "pcap": (lambda ctx, fb, n: ctx.pcap_size(fb, 0, n),
             lambda fb, dst, n: {"nbytes": fb.pcap_pack(dst, 0, n, t0_ns=tgp.T0, step_ps=tgp.STEP)[0]}),
    "encap": (lambda ctx, fb, n: ctx.encap_size(fb, 0, n, VX)[1],
              lambda fb, dst, n: {"ms_is_a_number": fb.encap(dst, 0, n, opts=VX) >= 0}),
    "frag": (lambda ctx, fb, n: ctx.fragment_size(fb, 0, n, 576, True)[1],
             lambda fb, dst, n: fb.fragment(dst, 0, n, 576, True)),
    "seg": (lambda ctx, fb, n: ctx.segment_size(fb, 0, n, 536, False, False)[1],
            lambda fb, dst, n: fb.segment(dst, 0, n, 536)),
    "xlat": (lambda ctx, fb, n: ctx.xlat46_size(fb, 0, n, XO)[1],
             lambda fb, dst, n: fb.xlat46(dst, 0, n, XO)),
}


def counters(res):
    if isinstance(res, dict):
        return res
    return {name: int(getattr(res, name)) for name, _ in res._fields_ if name != "device_ms"}


@pytest.fixture(scope="module")
def built(ctxs):
    """configs[2] built on the GPU, the same frames in the default context and in the one that keeps
    one page per workgroup."""
    seq = Sequence.from_config(pc.get("c3_udp_var"))
    out = {}
    try:
        for k in (None, 1):
            ctx = ctxs[k]
            ctx.load_sequence(0, seq, pc.SEED_BASE)
            out[k] = ctx.alloc_frames(*ctx.build_size(0, N_BUILT))
            ctx.build(0, 5000, N_BUILT, out[k])
            ctx.sync()
        yield out
    finally:
        for fb in out.values():
            fb.free()


@pytest.mark.parametrize("writer", rc.WRITERS)
def test_natural_size_against_one_page_per_workgroup(ctxs, built, writer):
    """The smallest range of the built frames whose output the rule itself gives 2 pages per
    workgroup (32,768 pages, 128 MiB), repacked in the default context and under PBGPU_RP_PER=1: the
    same bytes (pad and slack included), offsets, metadata and counters."""
    size, call = NATURAL[writer]
    pages = lambda n: (((size(ctxs[None], built[None], n) + 15) & ~15) + PAGE - 1) // PAGE
    lo, hi = 1, N_BUILT
    assert pages(hi) >= 32768
    while lo < hi:  # the smallest n with 32,768 pages
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pages(mid) >= 32768 else (mid + 1, hi)
    n, npages = lo, pages(lo)
    assert npages == 32768 and pages(n - 1) == 32767
    assert ctxs[None].page_grid(npages) == (2, 16384) and ctxs[1].page_grid(npages) == (1, 32768)
    got = {}
    for k in (None, 1):
        ctx, fb = ctxs[k], built[k]
        total = size(ctx, fb, n)
        dst, cap = tgs.fresh_dst(ctx, total, N_BUILT * 4)
        try:
            res = counters(call(fb, dst, n))
            meta = (int(dst.f.n_frames), int(dst.f.fixed_len), int(dst.f.total_bytes))
            assert meta[2] == total
            got[k] = (res, meta, dst.offsets() if meta[0] else None, dst.stream(cap))
        finally:
            dst.free()
    (res_a, meta_a, off_a, bytes_a), (res_b, meta_b, off_b, bytes_b) = got[None], got[1]
    assert res_a == res_b and meta_a == meta_b
    assert (off_a is None and off_b is None) or np.array_equal(off_a, off_b)
    assert np.array_equal(bytes_a, bytes_b)
    r16 = (meta_a[2] + 15) & ~15
    assert not bytes_a[meta_a[2]:r16].any() and (bytes_a[r16:] == 0xA5).all() and bytes_a[:meta_a[2]].any()
