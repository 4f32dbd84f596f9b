"""pbgpu_verify / pbgpu_frames_upload on the GPU: every frame's verdict against the CPU checker.

The reference is the oracle's checker, `oracle_binding.verify_frames`, called on one frame at a
time (n = 1): it says whether a frame is bad.  It stops at the first failing check, so which
checks failed comes from `ref_code` (verify_ref.py), a plain restatement of the same rules (RFC 1071 over
the frame's big-endian words); `ref_codes` asserts for every frame it is given that the two agree
(oracle says bad <=> ref_code != 0).  Neither is the code under test."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_binding as ob
import pb_configs as pc
import pbgpu
from pbgpu import GpuContext, PbError, Sequence
from verify_ref import expect, ref_code, ref_codes, ref_one  # noqa: F401

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NONE = pbgpu.NO_BAD_FRAME


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def uploaded(ctx, data, off=None, flen=0, fb=None):
    """The frames in a buffer of their own (or again in fb)."""
    n = len(off) - 1 if off is not None else len(data) // flen
    if fb is None:
        fb = ctx.alloc_frames(n, len(data))
    fb.upload(data, offsets=off, fixed_len=flen)
    return fb


def oracle_frames(cfg, n, first=12345, rule=0, fold=0):
    return ob.build(Sequence.from_config(cfg), 0, first, n, pc.SEED_BASE, payload_rule=rule, iph_fold=fold)


def cfg_mask(cfg):
    m = 0
    if cfg.get("ip", {}).get("csum", 1):
        m |= pbgpu.VERIFY_IP_CSUM | pbgpu.VERIFY_TOT_LEN
    if cfg.get("l4csum", 1):
        m |= pbgpu.VERIFY_L4_CSUM
    return m


# ------------------------------------------------------------------ 1. every config
CASES = [(n, 0, 0) for n in pc.ALL] + list(pc.RULE_CASES)


@pytest.mark.parametrize("name,rule,fold", CASES)
def test_every_config_builds_clean(ctx, name, rule, fold):
    """601 iterations at first_iter 12345: clean under the config's own checks; under every check
    the counts, first_bad and codes are the reference's (udp_no_csums: every frame bad; the
    single-fold cases: whatever the reference says, under the config's checks too)."""
    cfg = pc.get(name)
    seq = Sequence.from_config(cfg)
    ctx.load_sequence(0, seq, pc.SEED_BASE, payload_rule=rule, iph_fold=fold)
    fb = ctx.alloc_frames(*ctx.build_size(0, 601))
    try:
        ctx.build(0, 12345, 601, fb)
        n = int(fb.f.n_frames)
        assert n == 601 * seq.frames_per_iter
        ref = ref_codes(fb.packed(), fb.offsets())
        mask = cfg_mask(cfg)
        res = fb.verify(checks=mask)
        # a short frame is bad under any mask
        want = np.where(ref & 8, ref, ref & mask)
        print(f"{name}: {n} frames, bad under own checks {res.n_bad}, under all {np.count_nonzero(ref)}")
        assert res.n_checked == n
        assert res.n_bad == int(np.count_nonzero(want))
        if not fold:
            assert res.n_bad == 0 and res.first_bad == NONE
        res, codes = fb.verify(codes=True)
        expect(res, codes, ref)
        if name == "udp_no_csums":
            assert res.n_bad == n
    finally:
        fb.free()


# ------------------------------------------------------------------ 2. alignment and length sweep
def _sweep_cases():
    out = []
    for flen in (42, 43, 45, 60, 61, 64, 98, 127, 128, 129, 1499, 1500, 1514):
        c = pc.c2_udp_64()
        c["payloads"] = [{"length": {"min": flen - 42, "max": flen - 42}}]
        out.append((f"udp{flen}", c, flen))
    out.append(("tcp60", pc.c4_tcp_syn(), 60))
    out.append(("icmp98", pc.c5_icmp_echo(), 98))
    return out


SWEEP = _sweep_cases()


@pytest.mark.parametrize("label,cfg,flen", SWEEP, ids=[s[0] for s in SWEEP])
def test_alignment_and_length_sweep(ctx, label, cfg, flen):
    """67 oracle frames per length (starts on every alignment the length gives): clean; then one
    bit flipped in frame 0 / 33 / 66 at byte 3 (Ethernet: stays good), 17, 22, 23, 24, 26, 34, the
    first payload byte and the last byte: a one-bit flip inside a summed region always changes a
    one's-complement sum, so each flips its check's verdict, as the reference says."""
    data, off = oracle_frames(cfg, 67)
    assert len(off) == 68 and np.all(np.diff(off.astype(np.int64)) == flen)
    hl = 54 if label == "tcp60" else 42
    base = ref_codes(data, off)
    assert not base.any()
    fb = uploaded(ctx, data, flen=flen)
    try:
        assert int(fb.f.fixed_len) == flen and int(fb.f.n_frames) == 67
        res, codes = fb.verify(codes=True)
        expect(res, codes, base)
        for fr in (0, 33, 66):
            for pos in sorted({3, 17, 22, 23, 24, 26, 34, min(hl, flen - 1), flen - 1}):
                d = data.copy()
                d[fr * flen + pos] ^= 0x01
                ref = base.copy()
                ref[fr] = ref_one(d[fr * flen:(fr + 1) * flen])
                assert (ref[fr] != 0) == (pos != 3), (fr, pos)
                uploaded(ctx, d, flen=flen, fb=fb)
                res, codes = fb.verify(codes=True)
                expect(res, codes, ref)
                assert fb.verify().n_bad == res.n_bad  # the variant without codes
    finally:
        fb.free()


# ------------------------------------------------------------------ 3. packed odd offsets
@pytest.fixture(scope="module")
def var_frames():
    """257 oracle frames each of c3_udp_var and tcp_all_flags_var, with their reference codes."""
    out = {}
    for name in ("c3_udp_var", "tcp_all_flags_var"):
        data, off = oracle_frames(pc.get(name), 257)
        starts = off[:-1].astype(np.int64)
        assert (starts & 1).any() and not (starts & 1).all()  # odd and even starts
        base = ref_codes(data, off)
        assert not base.any()
        out[name] = (data, off, base)
    return out


@pytest.mark.parametrize("name", ["c3_udp_var", "tcp_all_flags_var"])
def test_packed_odd_offsets(ctx, var_frames, name):
    data, off, base = var_frames[name]
    fb = uploaded(ctx, data, off)
    try:
        assert int(fb.f.fixed_len) == 0
        res, codes = fb.verify(codes=True)
        expect(res, codes, base)
        victims = (0, 1, 63, 64, 255, 256)
        for group in [(v,) for v in victims] + [victims]:
            d = data.copy()
            ref = base.copy()
            for v in group:
                d[int(off[v + 1]) - 1] ^= 0x01
                ref[v] = ref_one(d[int(off[v]):int(off[v + 1])])
                assert ref[v]
            uploaded(ctx, d, off, fb=fb)
            res, codes = fb.verify(codes=True)
            expect(res, codes, ref)
            assert res.first_bad == group[0]
    finally:
        fb.free()


# ------------------------------------------------------------------ 4. short and degenerate frames
def test_short_and_degenerate_frames(ctx):
    good, goff = oracle_frames(pc.c1_udp_static_106(), 8)
    g = [good[int(goff[i]):int(goff[i + 1])] for i in range(8)]
    assert all(len(x) == 106 for x in g)
    parts = [g[0], g[1][:0], g[1], g[2][:1], g[2], g[3][:33], g[3], g[4][:34], g[4], g[5][:35], g[5], g[6][:0],
             g[6][:0], g[7], g[7][:33]]
    data = np.concatenate(parts)
    off = np.concatenate(([0], np.cumsum([len(p) for p in parts]))).astype(np.uint64)
    ref = ref_codes(data, off)
    assert int(np.count_nonzero(ref & 8)) == 6 and ref[-1] == 8
    fb = uploaded(ctx, data, off)
    try:
        res, codes = fb.verify(codes=True)
        expect(res, codes, ref)
        # a short frame is bad whatever the mask
        res = fb.verify(checks=0)
        assert res.n_bad == res.bad_short == 6 and res.first_bad == 1
        res, codes = fb.verify(first=3, n=0, codes=True)
        assert (res.n_checked, res.n_bad, res.bad_short, res.bad_ip_csum, res.bad_tot_len, res.bad_l4_csum) == (0,) * 6
        assert res.first_bad == NONE and len(codes) == 0
    finally:
        fb.free()
    # fixed length below 34: every frame short
    fb = uploaded(ctx, good[:33 * 5].copy(), flen=33)
    try:
        res, codes = fb.verify(codes=True)
        expect(res, codes, np.full(5, 8, np.uint8))
    finally:
        fb.free()


# ------------------------------------------------------------------ 5. sub-range
def test_sub_range(ctx, var_frames):
    data, off, base = var_frames["c3_udp_var"]
    d = data.copy()
    ref = base.copy()
    for v in (3, 200):
        d[int(off[v + 1]) - 1] ^= 0x01
        ref[v] = ref_one(d[int(off[v]):int(off[v + 1])])
    r = pbgpu.VerifyResult()
    fb = uploaded(ctx, d, off)
    try:
        res, codes = fb.verify(first=5, n=100, codes=True)
        expect(res, codes, ref[5:105], first=5)
        assert res.n_bad == 0
        res, codes = fb.verify(first=150, n=107, codes=True)
        expect(res, codes, ref[150:257], first=150)
        assert res.n_bad == 1 and res.first_bad == 200
        for first, n in ((0, 258), (257, 1), (258, 0), (200, 58), (2**64 - 1, 2)):
            with pytest.raises(PbError) as e:
                fb.verify(first=first, n=n)
            assert e.value.code == -22
        assert ctx.lib.pbgpu_verify(ctx.h, fb.ptr, 0, 1, 7, None, None) == -22
    finally:
        fb.free()
    fb = ctx.alloc_frames(16, 4096)  # never built or uploaded
    try:
        assert ctx.lib.pbgpu_verify(ctx.h, fb.ptr, 0, 0, 7, C.byref(r), None) == -22
    finally:
        fb.free()


# ------------------------------------------------------------------ 6. reference-captured frames
def test_reference_captured_frames(ctx):
    with open(os.path.join(GOLD, "kat_test1_gif.json")) as f:
        kat = json.load(f)
    frames = [np.frombuffer(bytes.fromhex(fr["hex"].replace(" ", "")), dtype=np.uint8) for fr in kat["frames"]]
    assert len(frames) == 2
    data = np.concatenate(frames)
    off = np.concatenate(([0], np.cumsum([len(x) for x in frames]))).astype(np.uint64)
    fb = uploaded(ctx, data, off)
    try:
        res, codes = fb.verify(codes=True)
        expect(res, codes, ref_codes(data, off))
        assert res.n_bad == 0 and res.n_checked == 2
    finally:
        fb.free()


# ------------------------------------------------------------------ 7. upload round trip
def test_upload_round_trip(ctx, var_frames):
    data, off, _ = var_frames["tcp_all_flags_var"]
    fb = uploaded(ctx, data, off + np.uint64(1000))  # offsets are taken relative to the first
    try:
        assert np.array_equal(fb.offsets(), off)
        assert np.array_equal(fb.packed(), data)
        assert fb.total_bytes() == len(data)
        umem = np.zeros(257 * 2048, dtype=np.uint8)
        lens = fb.to_umem(umem, 2048, 0, 257)
        assert np.array_equal(lens, np.diff(off.astype(np.int64)).astype(np.uint16))
        for i in (0, 1, 128, 256):
            assert np.array_equal(umem[i * 2048:i * 2048 + int(lens[i])], data[int(off[i]):int(off[i + 1])])
        dec = off.copy()
        dec[100] = dec[99] - np.uint64(1)
        with pytest.raises(PbError) as e:
            fb.upload(data, offsets=dec)
        assert e.value.code == -22
        # a refused upload leaves the buffer as it was
        assert np.array_equal(fb.offsets(), off)
    finally:
        fb.free()
    fixed = data[:64 * 100].copy()
    fb = uploaded(ctx, fixed, flen=64)
    try:
        assert int(fb.f.n_frames) == 100 and int(fb.f.fixed_len) == 64
        assert np.array_equal(fb.packed(), fixed)
        assert np.array_equal(fb.offsets(), np.arange(101, dtype=np.uint64) * np.uint64(64))
    finally:
        fb.free()
    small = ctx.alloc_frames(256, len(data))  # too few frames
    tight = ctx.alloc_frames(257, len(data) - 64)  # too few bytes
    try:
        for fb in (small, tight):
            with pytest.raises(PbError) as e:
                fb.upload(data, offsets=off)
            assert e.value.code == -28
    finally:
        small.free()
        tight.free()


# ------------------------------------------------------------------ 8. 64-bit offsets
def test_offsets_past_4_gib(ctx):
    """2^23 configs[2] frames cross 2^32 bytes: a truncated byte offset would read mid-frame."""
    n = 1 << 23
    ctx.load_sequence(0, Sequence.from_config(pc.get("c3_udp_var")), pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n))
    try:
        ctx.build(0, 12345, n, fb)
        res = fb.verify()
        assert (res.n_checked, res.n_bad, res.first_bad) == (n, 0, NONE)
        off = fb.offsets()
        assert int(off[-1]) > 1 << 32
        for m in range(1, int(off[-1] >> np.uint64(32)) + 1):
            f = int(np.searchsorted(off, np.uint64(m << 32), side="right")) - 1
            assert int(off[f]) <= m << 32 < int(off[f + 1])
            res, codes = fb.verify(first=f - 16, n=32, codes=True)
            assert res.n_checked == 32 and res.n_bad == 0 and not codes.any()
    finally:
        fb.free()


# ------------------------------------------------------------------ 9. full size
@pytest.mark.parametrize("name,n", [("c2_udp_64", 1 << 25), ("c2_udp_1500", 1 << 22), ("c3_udp_var", 1 << 22)])
def test_full_size(ctx, name, n):
    ctx.load_sequence(0, Sequence.from_config(pc.get(name)), pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n))
    try:
        ctx.build(0, 0, n, fb)
        flen = int(fb.f.fixed_len)
        w0 = n // 2 - 2048
        if flen:
            b0, b1 = w0 * flen, (w0 + 4096) * flen
        else:
            off = fb.offsets()
            b0, b1 = int(off[w0]), int(off[w0 + 4096])
        before, after = np.empty(b1 - b0, np.uint8), np.empty(b1 - b0, np.uint8)
        assert ctx.lib.pbgpu_copy_packed(ctx.h, fb.ptr, before.ctypes.data, b0, b1 - b0) == 0
        res = fb.verify()
        print(f"{name}: {n} frames verified in {res.device_ms:.3f} ms on the device")
        assert (res.n_checked, res.n_bad, res.first_bad) == (n, 0, NONE)
        assert res.device_ms > 0
        assert ctx.lib.pbgpu_copy_packed(ctx.h, fb.ptr, after.ctypes.data, b0, b1 - b0) == 0
        assert np.array_equal(before, after)
        assert ctx.read_probe_at(fb, (b1 + 15) & ~15, 2) > 0
    finally:
        fb.free()
