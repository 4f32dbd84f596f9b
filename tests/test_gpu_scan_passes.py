"""pb_scan_blocks past its first pass of 8192 entries, through every caller that can get there at a
size a test can afford (tests/scan_cases.py; test_scan_cases_cpu.py holds its arithmetic and its
references without a GPU): the length pass of pb_vline_kernel and pb_vstage_kernel at 32 frames per
workgroup, pb_vstage_kernel's 3-pass scan, and the fragmenter's and the segmenter's row scans over a
source of 9,217 rows.  Each case has 1,025 entries in the second pass and a ragged last one.

Every reference is numpy on the host: all offsets are compared, and the bytes of three windows of 64
frames (the first, the ones around the second pass's first frame, the last) against the oracle, pyfrag
and pyseg; the device verifiers walk the whole buffers.  No buffer's data comes to the host whole."""
import numpy as np
import pytest

import oracle_binding as ob
import pb_configs as pc
import pbgpu
import pyfrag
import pyseg
import scan_cases as sc
from pbgpu import GpuContext, PbError, Sequence

gpu = pytest.mark.gpu
SLOT = sc.SLOT


def r16(x):
    return (x + 15) & ~15


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def _alloc(ctx, frames, nbytes, what):
    try:
        return ctx.alloc_frames(frames, nbytes)
    except PbError as e:
        pytest.skip("cannot allocate the %.1f-GB %s: %s" % (nbytes / 1e9, what, e))


def _build(ctx, case, seq):
    """Loads seq (under the environment of the moment), builds the case's frames and holds the whole
    buffer against the numpy lengths and, in the windows, the oracle's bytes.  Returns the buffer."""
    ctx.load_sequence(SLOT, seq, pc.SEED_BASE)
    assert ctx.kernel_name(SLOT).startswith(case.kernel + "<"), ctx.kernel_name(SLOT)
    off = sc.offsets_of(sc.build_lengths(case))
    total = int(off[-1])
    assert ctx.build_size(SLOT, case.frames) == (case.frames, r16(case.frames * (42 + case.hi)) + 16)
    fb = _alloc(ctx, *ctx.build_size(SLOT, case.frames), what="frame buffer")
    try:
        p0, b0 = ctx.counters(SLOT + 1)
        ctx.build(SLOT, sc.FIRST_ITER, case.frames, fb)
        ctx.sync()
        assert (int(fb.f.n_frames), int(fb.f.fixed_len)) == (case.frames, 0)
        assert fb.total_bytes() == total
        sc.assert_offsets(fb.offsets(), off, case.id)
        for f0, n in sc.windows(case):
            o_data, o_off = ob.build(seq, SLOT, sc.FIRST_ITER + f0, n, pc.SEED_BASE)
            sc.assert_offsets(off[f0:f0 + n + 1] - off[f0], o_off, "%s: the reference at frame %d" % (case.id, f0))
            got = fb.stream(len(o_data), int(off[f0]))
            if not np.array_equal(got, o_data):
                pytest.fail("%s: frames %d..%d: first mismatch at byte %d of the window" %
                            (case.id, f0, f0 + n, int(np.nonzero(got != o_data)[0][0])))
        res = fb.verify()
        assert (int(res.n_checked), int(res.n_bad)) == (case.frames, 0), int(res.first_bad)
        p1, b1 = ctx.counters(SLOT + 1)
        assert (int(p1[SLOT] - p0[SLOT]), int(b1[SLOT] - b0[SLOT])) == (case.frames, total)
    except BaseException:
        fb.free()
        raise
    return fb


@gpu
@pytest.mark.parametrize("case", sc.BUILDS, ids=[b.id for b in sc.BUILDS])
def test_build_scans_past_one_pass(ctx, monkeypatch, case):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)  # read when the sequence is loaded
    assert sc.entries(case) > sc.constants()["PASS"]
    _build(ctx, case, Sequence.from_config(sc.config(case))).free()


@pytest.fixture(scope="module")
def source(ctx):
    """The cut source, built once: (buffer, sequence)."""
    seq = Sequence.from_config(sc.config(sc.SRC))
    fb = _build(ctx, sc.SRC, seq)
    yield fb, seq
    fb.free()


def _cut_one(case, frame):
    return pyfrag.fragment(frame, case.opt) if case.kind == "frag" else pyseg.segment(frame, case.opt)


@gpu
@pytest.mark.parametrize("case", sc.CUTS, ids=[c.id for c in sc.CUTS])
def test_cut_scans_past_one_pass(ctx, source, case):
    src, seq = source
    assert sc.entries(case) > sc.constants()["PASS"]
    ref = sc.cut_case_reference(case)
    cnt = ref.counts
    frag = case.kind == "frag"
    # the count and scan stages alone
    if frag:
        size = ctx.fragment_size(src, case.first, case.n, mtu=case.opt)
    else:
        size = ctx.segment_size(src, case.first, case.n, mss=case.opt)
    assert size == (cnt["n_out"], cnt["out_bytes"])
    # room for exactly the reference's output: a device that counts more gets -ENOSPC
    dst = _alloc(ctx, cnt["n_out"], r16(cnt["out_bytes"]), what="output buffer")
    try:
        if frag:
            res = src.fragment(dst, case.first, case.n, mtu=case.opt)
        else:
            res = src.segment(dst, case.first, case.n, mss=case.opt)
        assert {k: int(getattr(res, k)) for k in cnt} == cnt
        assert (int(dst.f.n_frames), int(dst.f.fixed_len), dst.total_bytes()) == (cnt["n_out"], 0, cnt["out_bytes"])
        sc.assert_offsets(dst.offsets(), ref.off, case.id)
        for f0, n in sc.windows(case):
            frames = ob.frames(seq, SLOT, sc.FIRST_ITER + case.first + f0, n, pc.SEED_BASE)
            recs = [r for f in frames for r in _cut_one(case, f)]
            k0, k1 = int(ref.first_rec[f0]), int(ref.first_rec[f0 + n])
            assert [len(r) for r in recs] == ref.out_len[k0:k1].tolist(), (case.id, f0)
            want = b"".join(recs)
            got = dst.stream(len(want), int(ref.off[k0])).tobytes()
            assert got == want, "%s: source frames %d..%d (records %d..%d)" % (case.id, f0, f0 + n, k0, k1)
        if frag:  # (a fragment's L4 checksum cannot be evaluated)
            v = dst.verify(checks=pbgpu.VERIFY_IP_CSUM | pbgpu.VERIFY_TOT_LEN)
            assert (int(v.n_checked), int(v.n_bad)) == (cnt["n_out"], 0), int(v.first_bad)
        else:  # the built source carries valid checksums, so every segment's hold
            v = dst.verify(checks=pbgpu.VERIFY_ALL)
            assert (int(v.n_checked), int(v.n_bad)) == (cnt["n_out"], 0), int(v.first_bad)
            w = dst.verify_wire(checks=pbgpu.WIRE_ALL)
            assert (int(w.n_checked), int(w.n_bad)) == (cnt["n_out"], 0), int(w.first_bad)
    finally:
        dst.free()
