"""pbgpu_verify against false inputs: one mutant per byte position on every kernel path, packed
mixtures with empty, short and jumbo frames, changes a one's-complement sum cannot see, sub-ranges,
masks, and the loops inside a wave / workgroup with bad frames in them.

Every comparison is `expect(res, codes, ref, first)`: the codes, all five counts and the absolute
first_bad, exactly.  The reference (verify_ref.py) is `ref_code`, a restatement of the rules in
Python integers, tied frame by frame to the oracle's C checker.  Which kernel path a case takes is
asserted from the launch arithmetic restated in verify_ref.py (test_verify_ref_cpu.py holds the table)."""
import numpy as np
import pytest

import oracle_binding as ob
import pb_configs as pc
import pbgpu
import verify_ref as vr
from pbgpu import GpuContext, Sequence
from verify_ref import clean_code, expect, good_frame, ref_one

pytestmark = pytest.mark.gpu
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


def check(fb, ref, first=0, n=None, checks=pbgpu.VERIFY_ALL):
    """One verify with codes against the reference's slice; the variant without codes agrees."""
    n = len(ref) - first if n is None else n
    want = ref[first:first + n]
    res, codes = fb.verify(first=first, n=n, checks=checks, codes=True)
    expect(res, codes, want, first)
    plain = fb.verify(first=first, n=n, checks=checks)
    assert (plain.n_checked, plain.n_bad, plain.first_bad) == (res.n_checked, res.n_bad, res.first_bad)
    assert (plain.bad_short, plain.bad_ip_csum, plain.bad_tot_len, plain.bad_l4_csum) == (
        res.bad_short, res.bad_ip_csum, res.bad_tot_len, res.bad_l4_csum)
    return res, codes


# ------------------------------------------------------------------ 1. one mutant per byte position
def _byte_cases():
    out = []
    for want, lengths in vr.LENGTH_CLASSES:
        for i, L in enumerate(lengths):
            protos = (17, 6, 1) if want == "vpg" or i == 0 else (17,)
            out += [(L, p, None) for p in protos]
    out += [(9043, 17, None), (65535, 17, None)]
    out += [(L, 17, 0xFF) for L in (1500, 9043, 65535)]
    return out


BYTE_CASES = _byte_cases()


def _positions(L):
    if L <= 4097:
        return np.arange(L)
    mid = np.random.default_rng(L).choice(np.arange(96, L - 96), 256, replace=False)
    return np.concatenate((np.arange(96), np.sort(mid), np.arange(L - 96, L)))


@pytest.mark.parametrize("L,proto,fill", BYTE_CASES, ids=[f"{L}-p{p}" + ("-ff" if f else "") for L, p, f in BYTE_CASES])
def test_one_mutant_per_byte(ctx, L, proto, fill):
    """Copies of one clean frame of L bytes back to back (an odd L starts them on every byte
    alignment), copy k with one byte changed (all positions; at 9043 and 65535 B the first 96, the
    last 96 and 256 drawn), the last copy untouched: bad exactly from byte 14 on.  At 34 and 35 B
    a kernel that lets the next copy's bytes into the segment calls the clean copy bad."""
    base = good_frame(L, proto, 21, fill)
    pos = _positions(L)
    n = len(pos) + 1
    clean = clean_code(L, proto)
    assert clean == (4 if L < 36 and proto == 1 else 0)
    assert ref_one(base) == clean
    table = {x: c for c, ls in vr.LENGTH_CLASSES for x in ls}
    assert vr.shape_class(L, n) == table.get(L, (64, "unstaged"))
    fb = ctx.alloc_frames(n, n * L)
    try:
        for xor in ("bit", 0xFF):
            data = np.tile(base, n).reshape(n, L)
            x = (1 << (pos % 8)).astype(np.uint8) if xor == "bit" else np.uint8(0xFF)
            data[np.arange(len(pos)), pos] ^= x
            ref = np.array([ref_one(data[k]) for k in range(n)], dtype=np.uint8)
            uploaded(ctx, data.reshape(-1), flen=L, fb=fb)
            assert int(fb.f.fixed_len) == L and int(fb.f.n_frames) == n
            res, codes = check(fb, ref)
            # the kernel's answer itself, not only through the reference
            assert np.all(codes[:-1][pos >= 14] != 0)
            assert np.all(codes[:-1][pos < 14] == clean) and codes[-1] == clean
            if clean == 0:
                assert res.n_bad == int(np.count_nonzero(pos >= 14)) and res.first_bad == 14
                assert fb.verify().n_bad == res.n_bad
    finally:
        fb.free()


# ------------------------------------------------------------------ 2. packed, mixed
@pytest.fixture(scope="module")
def mixes():
    """The two packed mixtures (G = 8 and G = 16), their bytes, offsets and reference codes."""
    out = {}
    for G, n_small in ((8, 2400), (16, 300)):
        frames, jumbo, near = vr.packed_mix(n_small)
        data, off = vr.pack(frames)
        out[G] = (frames, jumbo, near, data, off, vr.ref_codes(data, off))
    return out


def _mix_shape(G, data, off):
    n, mean = len(off) - 1, len(data) // (len(off) - 1)
    assert mean <= 192 if G == 8 else 193 <= mean <= 768
    assert vr.shape_class(0, n, mean, off) == (G, "both")  # unstaged windows among the staged ones
    return vr.verify_shape(0, 0, n, mean)


@pytest.mark.parametrize("G", [8, 16])
def test_packed_mixed(ctx, mixes, G):
    """Clean; then every jumbo frame changed at one of the places where the kernel changes hands
    (jumbo_positions), place by place; then the short frames next to the jumbo ones, at their last byte."""
    frames, jumbo, near, data, off, base = mixes[G]
    sh = _mix_shape(G, data, off)
    lens = np.diff(off.astype(np.int64))
    assert sorted(lens[jumbo]) == [9043] * 6 + [65535] * 4
    for L in (9043, 65535):  # odd and even offsets of both
        assert {int(off[j]) & 1 for j in jumbo if lens[j] == L} == {0, 1}
    run = int(np.nonzero(lens[jumbo[-1]:] == 0)[0][0]) + jumbo[-1]
    assert not lens[run:run + 512].any() and 2 * sh["bf"] <= 512 and lens[-1] == 0  # whole windows of empty frames
    for L in (1, 13, 33, 34, 35):
        assert L in lens
    assert set(np.unique(base)) == {0, 8}
    fb = uploaded(ctx, data, off)
    try:
        assert int(fb.f.fixed_len) == 0
        check(fb, base)
        places = [vr.jumbo_positions(int(off[j]), int(lens[j])) for j in jumbo]
        assert all(6 <= len(p) <= 8 for p in places)
        for k in range(8):
            d, ref = data.copy(), base.copy()
            for j, p in zip(jumbo, places):
                at = p[k % len(p)]
                d[int(off[j]) + at] ^= 1 << (at % 8)
                ref[j] = ref_one(d[int(off[j]):int(off[j + 1])])
            uploaded(ctx, d, off, fb=fb)
            res, codes = check(fb, ref)
            assert np.all(codes[jumbo] != 0) and res.n_bad == len(jumbo) + int(np.count_nonzero(base))
        d, ref = data.copy(), base.copy()
        for v in near:
            assert 60 <= lens[v] <= 120
            d[int(off[v + 1]) - 1] ^= 0x80
            ref[v] = ref_one(d[int(off[v]):int(off[v + 1])])
        uploaded(ctx, d, off, fb=fb)
        res, codes = check(fb, ref)
        assert np.all(codes[near] != 0) and not codes[jumbo].any()
    finally:
        fb.free()


def test_five_empty_frames(ctx):
    fb = uploaded(ctx, np.zeros(0, np.uint8), np.zeros(6, np.uint64))
    try:
        assert fb.total_bytes() == 0 and int(fb.f.n_frames) == 5
        res, codes = check(fb, np.full(5, 8, np.uint8))
        assert (res.n_bad, res.bad_short, res.first_bad) == (5, 5, 0)
        check(fb, np.full(5, 8, np.uint8), first=2, n=3, checks=0)
    finally:
        fb.free()


# ------------------------------------------------------------------ 3. what a sum cannot tell
def _blind_frames(L, proto):
    """13 frames: 0, 4, 8, 12 changed in ways the sums cannot see (two word swaps, 00 00 -> FF FF in
    the segment and in the IPv4 id), 2, 6, 10 true mutants, the rest clean."""
    frames = [good_frame(L, proto, 300 + k) for k in range(13)]
    frames[0] = vr.swap_words(frames[0], 1)
    frames[4] = vr.zero_word_frame(L, proto, 4, 34 + 2 * ((L - 34) // 4))[1]
    frames[8] = vr.swap_words(frames[8], 2)
    frames[12] = vr.zero_word_frame(L, proto, 12, 18)[1]
    for k, j in ((2, 34), (6, L - 1), (10, 20)):
        frames[k][j] ^= 0x10
    return frames


@pytest.mark.parametrize("L,proto,packed", [(98, 1, False), (1500, 17, False), (4097, 6, False), (9043, 17, True)],
                         ids=["98", "1500", "4097", "packed9043"])
def test_same_verdict_where_the_sum_is_blind(ctx, L, proto, packed):
    frames = _blind_frames(L, proto)
    if packed:  # a 35-B frame first: frames 0, 4, 8, 12 at odd offsets
        frames = [good_frame(35, 17, 1)] + frames
    data, off = vr.pack(frames)
    ref = vr.ref_codes(data, off)
    s = 1 if packed else 0
    assert [int(i) - s for i in np.nonzero(ref)[0]] == [2, 6, 10]
    if packed:
        assert all(int(off[s + k]) & 1 for k in (0, 4, 8, 12))
    fb = uploaded(ctx, data, off) if packed else uploaded(ctx, data, flen=L)
    try:
        res, codes = check(fb, ref)
        assert not codes[[s, s + 4, s + 8, s + 12]].any() and res.n_bad == 3
    finally:
        fb.free()


# ------------------------------------------------------------------ 4. sub-ranges
def _sub_ranges(off, mutants):
    """(first, n) pairs: first in {0, 1, the first frame starting in page 1, the one before, a mutant,
    the frame after it}; n in {1, 2, up to the next page edges, to the last frame}."""
    n_frames = len(off) - 1
    starts = off[:-1].astype(np.int64)
    p1 = int(np.searchsorted(starts, 4096, side="left"))  # first frame starting in page 1
    out = set()
    for first in (0, 1, p1, p1 - 1, mutants[3], mutants[3] + 1):
        page = int(starts[first]) >> 12
        ends = [int(np.searchsorted(starts, (page + k) << 12, side="left")) for k in (1, 2)]
        for n in [1, 2, n_frames - first] + [e - first for e in ends]:
            if 0 < n <= n_frames - first:
                out.add((first, n))
    return sorted(out), p1


def _sub_range_run(ctx, data, off, base, flen):
    n = len(off) - 1
    starts = off[:-1].astype(np.int64)
    p1 = int(np.searchsorted(starts, 4096, side="left"))
    s = p1 - 1  # the frame holding byte 4095: it straddles the page edge, or ends at it
    usable = [i for i in range(n) if base[i] == 0 and int(off[i + 1]) - int(off[i]) >= 60]
    near = lambda i: min(usable, key=lambda u: abs(u - i))  # noqa: E731
    mutants = sorted({near(0), near(s), near(s + 1), near(s + 3), near(n // 3), near(n // 3 + 1), near(n // 2),
                      near(n - 1)})
    d, ref = data.copy(), base.copy()
    for k, m in enumerate(mutants):
        L = int(off[m + 1]) - int(off[m])
        j = (17, 34, L - 1, 22, 41)[k % 5]
        d[int(off[m]) + j] ^= 1 << (k % 8)
        ref[m] = ref_one(d[int(off[m]):int(off[m + 1])])
        assert ref[m]
    ranges, p1 = _sub_ranges(off, mutants)
    assert len(ranges) >= 12
    fb = uploaded(ctx, d, flen=flen) if flen else uploaded(ctx, d, off)
    try:
        quiet = 0
        for first, cnt in ranges:
            res, codes = check(fb, ref, first, cnt)
            if not ref[first:first + cnt].any():
                assert res.n_bad == 0 and res.first_bad == NONE
                quiet += 1
            else:
                assert res.first_bad == first + int(np.nonzero(ref[first:first + cnt])[0][0])
        assert quiet >= 1
        # mutants just outside on both sides of a clean range
        a, b = near(s + 1), near(s + 3)
        if b - a >= 2:
            res, codes = check(fb, ref, a + 1, b - a - 1)
            assert res.n_bad == 0 and res.first_bad == NONE and ref[a] and ref[b]
        if flen == 64:  # up to a page edge exactly
            res, codes = check(fb, ref, 64, 64)
            assert res.n_checked == 64
    finally:
        fb.free()


@pytest.mark.parametrize("flen,n", [(60, 400), (64, 400), (98, 400), (127, 400), (129, 400), (1500, 100), (2049, 100)])
def test_sub_ranges_fixed(ctx, flen, n):
    """pb_vpg_kernel (60 .. 127 B) with first_frame != 0 and n < n_frames: its fcur clamp, the index
    into codes, the absolute first_bad and the load limit; pb_vst_kernel staged and unstaged."""
    frames = [good_frame(flen, (17, 6, 1)[k % 3], 400 + k) for k in range(n)]
    data, off = vr.pack(frames)
    assert vr.verify_shape(flen, 0, n, flen)["kernel"] == ("vpg" if flen <= 128 else "vst")
    _sub_range_run(ctx, data, off, np.zeros(n, np.uint8), flen)


def test_sub_ranges_packed(ctx, mixes):
    frames, jumbo, near, data, off, base = mixes[8]
    _sub_range_run(ctx, data, off, base, 0)


# ------------------------------------------------------------------ 5. masks
def _coded(f, code):
    """A clean frame made to fail exactly the checks of `code` (1 IP checksum, 2 tot_len, 4 L4)."""
    f = f.copy()
    if code & 2:  # a wrong tot_len under a checksum that covers it
        f[17] ^= 0x04
        f[24] = f[25] = 0
        c = 0xFFFF - vr._fold(vr._sum16(f[14:34]))
        f[24], f[25] = c >> 8, c & 0xFF
    if code & 1:
        f[22] ^= 0x20
    if code & 4:
        f[len(f) - 1] ^= 0x02
    return f


def _mask_run(ctx, data, off, ref, flen):
    fb = uploaded(ctx, data, flen=flen) if flen else uploaded(ctx, data, off)
    try:
        for checks in range(8):
            want = np.where(ref & 8, ref, ref & checks).astype(np.uint8)
            for c in (checks, 0xF8 | checks, 0xFFFFFF00 | checks):  # bits above 7 are ignored
                check(fb, want, checks=c)
    finally:
        fb.free()


def test_masks_fixed(ctx):
    frames = [_coded(good_frame(98, (17, 6, 1)[k % 3], 500 + k), (k * 3) % 8) for k in range(80)]
    data, off = vr.pack(frames)
    ref = vr.ref_codes(data, off)
    assert np.array_equal(ref, (np.arange(80) * 3) % 8)
    _mask_run(ctx, data, off, ref, 98)


def test_masks_packed(ctx):
    frames = []
    for k in range(90):
        f = good_frame(60 + (k * 11) % 200, (17, 6, 1)[k % 3], 600 + k)
        frames.append(f[:(0, 1, 33)[k % 3]] if k % 9 == 8 else _coded(f, k % 9))
    data, off = vr.pack(frames)
    ref = vr.ref_codes(data, off)
    assert np.array_equal(ref, np.arange(90) % 9)
    _mask_run(ctx, data, off, ref, 0)


# ------------------------------------------------------------------ 6. loops inside a wave / workgroup
def _loop_places(n, flen, sh):
    """Frames at the edges of what one wave or workgroup takes in each turn of its loop."""
    out = {0, n - 1, n - 2, n // 2, n // 2 + 1}
    if sh["kernel"] == "vpg":
        per, grid = sh["per"], sh["grid"]
        for w in (0, 1, 2, 7, 8, grid // 4, grid // 2, grid // 2 + 1, grid - 2, grid - 1):
            for p in range(w * per, min((w + 1) * per, sh["npages"])):
                a = -(-(p << 12) // flen)             # first frame starting in page p
                b = -(-((p + 1) << 12) // flen) - 1   # the last one: it straddles into the next page (or wave)
                out |= {a, a + 1, min(b, n - 1)}
    else:
        wgf, bf, grid = sh["wgf"], sh["bf"], sh["grid"]
        per = grid >> 3
        # regions at both ends of the workgroup numbering: workgroup b takes region (b & 7) * per + (b >> 3)
        for r in (0, 1, per - 1, per, per + 1, 2 * per, 4 * per - 1, 7 * per, 8 * per - 1, 8 * per, grid // 2,
                  grid - 2, grid - 1):
            for k in range(0, wgf, bf):
                out |= {r * wgf + k, r * wgf + k + bf - 1}
        out |= set(range(n - (n % wgf), n))  # the ragged tail
    return sorted(i for i in out if 0 <= i < n)


LOOPS = [("c4_tcp_syn", (1 << 21) + (1 << 18)), ("c2_udp_1500", 2 * 8 * 16384 + 43), ("c3_udp_var", (1 << 18) + 29)]


@pytest.mark.parametrize("name,n", LOOPS, ids=[x[0] for x in LOOPS])
def test_loops_with_bad_frames(ctx, name, n):
    """Built on the GPU at the smallest size where a wave takes two pages (60 B) or a workgroup two
    windows (1500 B, packed); fetched, about 64 frames changed by one byte at the edges of every turn
    of those loops, put back into the same buffer: the codes are the reference's on the mutants and
    0 elsewhere (the C checker counts as many bad frames in the whole buffer as there are mutants).
    Then the mutants of the first half are taken out again: first_bad moves to the second half, also
    in a sub-range that starts at frame 5."""
    ctx.load_sequence(0, Sequence.from_config(pc.get(name)), pc.SEED_BASE)
    fb = ctx.alloc_frames(*ctx.build_size(0, n))
    try:
        ctx.build(0, 0, n, fb)
        assert int(fb.f.n_frames) == n
        flen = int(fb.f.fixed_len)
        data = fb.packed()
        off = fb.offsets() if not flen else None
        start = (lambda i: i * flen) if flen else (lambda i: int(off[i]))
        mean = flen if flen else len(data) // n
        sh = vr.verify_shape(flen, 0, n, mean)
        if name == "c4_tcp_syn":
            assert flen == 60 and (sh["kernel"], sh["npages"], sh["per"]) == ("vpg", 34560, 2)
        else:
            assert (sh["G"], sh["bf"], sh["nw"]) == (32, 8, 2) and (flen == 1500) == (name == "c2_udp_1500")
            assert n % sh["wgf"] not in (0, sh["bf"])  # a ragged last window
        places = _loop_places(n, flen, sh)
        assert 56 <= len(places) <= 72
        want = np.zeros(n, np.uint8)
        saved = {}
        for k, m in enumerate(places):
            a, b = start(m), start(m + 1)
            assert ref_one(data[a:b]) == 0
            j = a + (14, 17, 33, 34, 41, b - a - 1)[k % 6]
            saved[m] = (j, data[j])
            data[j] ^= 1 << (k % 8)
            want[m] = ref_one(data[a:b])
            assert want[m]
        assert ob.verify_frames(data, off, flen, n, 16) == len(places)
        fb.upload(data, offsets=off, fixed_len=flen)
        res, codes = fb.verify(codes=True)
        expect(res, codes, want)
        assert res.first_bad == 0 and res.n_bad == len(places)
        assert fb.verify().n_bad == len(places)
        # without the first half's mutants
        for m in places:
            if m < n // 2:
                data[saved[m][0]] = saved[m][1]
                want[m] = 0
        assert ob.verify_frames(data, off, flen, n, 16) == int(np.count_nonzero(want)) > 8
        fb.upload(data, offsets=off, fixed_len=flen)
        res, codes = fb.verify(codes=True)
        expect(res, codes, want)
        assert res.first_bad == n // 2
        # a sub-range that still takes two turns of the loop
        first, cnt = 5, n - 8
        sub = vr.verify_shape(flen, first, cnt, mean)
        assert sub.get("per") == 2 or sub.get("nw") == 2
        res, codes = fb.verify(first=first, n=cnt, codes=True)
        expect(res, codes, want[first:first + cnt], first)
        assert res.first_bad == n // 2 and want[n - 1] and res.n_bad < int(np.count_nonzero(want))  # mutants past its end
    finally:
        fb.free()
