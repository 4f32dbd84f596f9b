"""What the verify tests share: the reference, a maker of clean frames, the mutants a checksum can
and cannot see, and pbgpu_verify's launch shapes restated.

The reference is the oracle's checker, `oracle_binding.verify_frames`, called on one frame at a
time (n = 1): it says whether a frame is bad.  It stops at the first failing check, so which
checks failed comes from `ref_code`, a plain restatement of the same rules (RFC 1071 over the
frame's big-endian words); `ref_one` asserts for every frame it is given that the two agree
(oracle says bad <=> ref_code != 0).  Neither is the code under test."""
import os
import re

import numpy as np

import oracle_binding as ob
import pbgpu

NONE = pbgpu.NO_BAD_FRAME
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ reference
def _sum16(b):
    b = np.asarray(b, dtype=np.uint8)
    if len(b) & 1:
        b = np.append(b, np.uint8(0))
    w = b.reshape(-1, 2).astype(np.uint64)
    return int(((w[:, 0] << np.uint64(8)) | w[:, 1]).sum())


def _fold(s):
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def ref_code(f):
    n = len(f)
    if n < 34:
        return pbgpu.VERIFY_SHORT
    code = 0
    if _fold(_sum16(f[14:34])) != 0xFFFF:
        code |= pbgpu.VERIFY_IP_CSUM
    if (int(f[16]) << 8 | int(f[17])) != n - 14:
        code |= pbgpu.VERIFY_TOT_LEN
    s, proto = _sum16(f[34:]), int(f[23])
    if proto in (6, 17):
        s += _sum16(f[26:34]) + proto + (n - 34)
    if _fold(s) != 0xFFFF:
        code |= pbgpu.VERIFY_L4_CSUM
    return code


def ref_one(f):
    """One frame's code, tied to the oracle's verdict."""
    f = np.ascontiguousarray(f, dtype=np.uint8)
    code = ref_code(f)
    # a one-byte buffer for an empty frame: the checker reads nothing of a short frame
    oracle_bad = ob.verify_frames(f if len(f) else np.zeros(1, np.uint8), None, len(f), 1, 1)
    assert oracle_bad == (1 if code else 0), (len(f), code)
    return code


def ref_codes(data, off):
    return np.array([ref_one(data[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)], dtype=np.uint8)


def expect(res, codes, ref, first=0):
    """A VerifyResult and its codes against reference codes of the same range."""
    assert np.array_equal(codes, ref), np.nonzero(codes != ref)[0][:8]
    assert res.n_checked == len(ref)
    assert res.n_bad == int(np.count_nonzero(ref))
    assert res.bad_short == int(np.count_nonzero(ref & 8))
    assert res.bad_ip_csum == int(np.count_nonzero(ref & 1))
    assert res.bad_tot_len == int(np.count_nonzero(ref & 2))
    assert res.bad_l4_csum == int(np.count_nonzero(ref & 4))
    bad = np.nonzero(ref)[0]
    assert res.first_bad == (first + int(bad[0]) if len(bad) else NONE)


# ------------------------------------------------------------------ clean frames
def _put16(f, pos, v):
    f[pos], f[pos + 1] = v >> 8, v & 0xFF


def fix_sums(f, proto):
    """Patches f (>= 34 bytes) in place into a frame of protocol `proto` that every check passes:
    Ethertype, version / IHL, tot_len, the protocol byte; then the L4 sum (with the pseudo header for
    protocols 6 and 17) is made to fold to 0xFFFF through the word at bytes 34..35 (the checker does
    not care where the checksum field lives), or, for a segment shorter than two bytes under
    protocols 6 / 17, through the last two address bytes; then the IPv4 checksum.  A segment shorter
    than two bytes without a pseudo header cannot be made to fold to 0xFFFF: L4_CSUM by definition."""
    n = len(f)
    assert n >= 34
    f[12], f[13], f[14], f[23] = 0x08, 0x00, 0x45, proto
    _put16(f, 16, n - 14)
    pseudo = proto in (6, 17)
    pos = 34 if n >= 36 else (32 if pseudo else None)
    if pos is not None:
        _put16(f, pos, 0)
        s = _sum16(f[34:])
        if pseudo:
            s += _sum16(f[26:34]) + proto + (n - 34)
        _put16(f, pos, 0xFFFF - _fold(s))
    _put16(f, 24, 0)
    _put16(f, 24, 0xFFFF - _fold(_sum16(f[14:34])))
    return f


def good_frame(L, proto, seed, fill=None):
    """L bytes, random (seeded) or all `fill`, patched into a clean frame (fix_sums)."""
    if fill is None:
        f = np.random.default_rng([int(seed), int(L), int(proto)]).integers(0, 256, L, dtype=np.uint8)
    else:
        f = np.full(L, fill, dtype=np.uint8)
    return fix_sums(f, proto)


def clean_code(L, proto):
    """What good_frame's result is by definition."""
    if L < 34:
        return pbgpu.VERIFY_SHORT
    return pbgpu.VERIFY_L4_CSUM if L < 36 and proto not in (6, 17) else 0


# ------------------------------------------------------------------ what a one's-complement sum cannot tell
def swap_words(f, seed):
    """A copy of f (>= 40 bytes) with two unequal 16-bit words of the segment swapped, both at even
    distances from byte 34: the sum's words are the same words."""
    n = len(f)
    nw = (n - 34) // 2
    rng = np.random.default_rng([int(seed), n])
    for _ in range(64):
        a, b = (34 + 2 * int(k) for k in rng.integers(0, nw, 2))
        if f[a] != f[b] or f[a + 1] != f[b + 1]:
            g = f.copy()
            g[a:a + 2], g[b:b + 2] = f[b:b + 2], f[a:a + 2]
            assert not np.array_equal(g, f)
            return g
    raise AssertionError("no two unequal words")


def zero_word_frame(L, proto, seed, at):
    """(clean frame with 00 00 at bytes at..at+1, the same frame with FF FF there); `at` is in the
    segment at an even distance from 34 (not the patched word at 34), or 18 (the IPv4 id).  The
    frame's sums are nonzero (they fold to 0xFFFF), so +0 and -0 are one value to them."""
    assert at == 18 or (at >= 36 and (at - 34) % 2 == 0 and at + 1 < L)
    f = np.random.default_rng([int(seed), int(L), int(proto), int(at)]).integers(0, 256, L, dtype=np.uint8)
    f[at] = f[at + 1] = 0
    fix_sums(f, proto)
    assert f[at] == 0 and f[at + 1] == 0
    g = f.copy()
    g[at] = g[at + 1] = 0xFF
    return f, g


# ------------------------------------------------------------------ the launch shapes, restated
def shape_constants():
    """PB_VS_STAGE, PB_VS_BF_MAX and PB_VST_WT as pb_device.h defines them."""
    src = open(os.path.join(ROOT, "pb-af-xdp_amd", "csrc", "pb_device.h")).read()
    out = {}
    for name in ("PB_VS_STAGE", "PB_VS_BF_MAX", "PB_VST_WT"):
        m = re.findall(r"^#define\s+%s\s+(\d+)u?\b" % name, src, re.M)
        assert len(m) == 1, name
        out[name] = int(m[0])
    return out


def page_grid(npages):
    """pbgpu.cpp's page_grid below its grid cap: (pages per wave, waves)."""
    per = min(max(npages // 16384, 1), 32)
    assert (npages + per - 1) // per <= 1 << 24
    return per, (npages + per - 1) // per


def verify_shape(fixed_len, first, n, mean):
    """pbgpu.cpp's verify_shape: the kernel and the sizing of a verify of frames [first, first + n)."""
    k = shape_constants()
    if fixed_len and fixed_len <= 128:
        page0 = first * fixed_len >> 12
        npages = (((first + n) * fixed_len - 1) >> 12) - page0 + 1
        per, grid = page_grid(npages)
        return {"kernel": "vpg", "page0": page0, "npages": npages, "per": per, "grid": grid}
    G = 8 if mean <= 192 else (16 if mean <= 768 else (32 if mean <= 3072 else 64))
    ng = k["PB_VST_WT"] // G
    target = k["PB_VS_STAGE"] - 16 if fixed_len else k["PB_VS_STAGE"] * 3 // 4
    bf = target // max(mean, 1) // ng * ng
    bf = min(max(bf, ng), k["PB_VS_BF_MAX"])
    nw = min(max(n // (bf * 16384), 1), 64)
    wgf = bf * nw
    return {"kernel": "vst", "G": G, "bf": bf, "nw": nw, "wgf": wgf, "grid": (n + wgf - 1) // wgf}


def window_flags(off, first, n, bf):
    """Per window of bf frames of [first, first + n): (frames, staged).  off: the buffer's n_frames + 1
    byte offsets (a callable frame -> byte for a fixed length works too).  A workgroup's frames are
    a multiple of bf, so the windows of a launch are the range cut every bf frames."""
    stage = shape_constants()["PB_VS_STAGE"]
    at = off if callable(off) else (lambda i: int(off[i]))
    out = []
    for w0 in range(0, n, bf):
        wn = min(bf, n - w0)
        sb, eb = at(first + w0), at(first + w0 + wn)
        out.append((wn, eb - (sb & ~15) <= stage))
    return out


def shape_class(fixed_len, n, mean=None, off=None):
    """The row of the case table a whole-buffer verify belongs to: 'vpg', or (G, staging) with staging
    'staged' / 'unstaged' / 'both' judged on the full windows (a ragged last window of fewer frames may
    fit where the full ones do not)."""
    sh = verify_shape(fixed_len, 0, n, fixed_len if fixed_len else mean)
    if sh["kernel"] == "vpg":
        return "vpg"
    fl = window_flags(off if off is not None else (lambda i: i * fixed_len), 0, n, sh["bf"])
    full = {s for wn, s in fl if wn == sh["bf"]}
    assert full
    return sh["G"], ("both" if len(full) == 2 else ("staged" if True in full else "unstaged"))


# The lengths of the per-byte mutant test by the path they take (fixed-length uploads of L + 1 frames)
LENGTH_CLASSES = [
    ("vpg", (34, 35, 36, 37, 41, 42, 59, 60, 61, 64, 98, 127, 128)),
    ((8, "staged"), (129, 192)),
    ((16, "staged"), (193, 768)),
    ((32, "staged"), (769, 1500, 2048)),
    ((32, "unstaged"), (2049, 3072)),
    ((64, "staged"), (3073, 4096)),
    ((64, "both"), (4095,)),
    ((64, "unstaged"), (4097,)),
]


# ------------------------------------------------------------------ the packed, mixed upload
def pack(frames):
    """(data, offsets) of frames back to back."""
    off = np.concatenate(([0], np.cumsum([len(x) for x in frames]))).astype(np.uint64)
    data = np.concatenate([np.asarray(x, dtype=np.uint8) for x in frames]) if int(off[-1]) else np.zeros(0, np.uint8)
    return data, off


def packed_mix(n_small):
    """The frames of the packed, mixed test: mostly clean frames of 60..120 B (UDP, TCP and protocol 1
    in turn), and among them runs of empty frames (512 in a row: whole windows of them; one as the
    last frame), lengths 1, 13, 33, 34, 35, four 65535-B frames each between two short ones, and six
    9043-B ones in pairs with one short frame between (two in a window do not fit the stage).
    n_small sets the mean: 2400 short frames keep it under 192 (G = 8), 300 put it in 193..768
    (G = 16).  Returns (frames, indices of the jumbo frames, indices of the short frames next to them)."""
    protos = (17, 6, 1)
    frames, jumbo, near = [], [], []
    count = [0]

    def small(k=1):
        for _ in range(k):
            i = count[0]
            count[0] += 1
            frames.append(good_frame(60 + (i * 7) % 61, protos[i % 3], 1000 + i))

    def empty(k):
        frames.extend(np.zeros(0, np.uint8) for _ in range(k))

    base = good_frame(106, 17, 1)
    run = max((n_small - 100) // 8, 1)
    small(40)
    empty(3)
    small(10)
    frames.extend([base[:1], base[:13], base[:33], good_frame(34, 17, 2), good_frame(35, 6, 3)])
    small(20)
    for j in range(4):
        near.append(len(frames))
        small()
        jumbo.append(len(frames))
        frames.append(good_frame(65535, protos[j % 2], 50 + j, 0xFF if j == 3 else None))
        near.append(len(frames))
        small()
        empty(j)
        frames.append(base[:1 + (j & 1)])  # moves the next one's parity
        small(run)
    for j in range(3):
        near.append(len(frames))
        small()
        for t in range(2):
            jumbo.append(len(frames))
            frames.append(good_frame(9043, protos[(j + t) % 3], 60 + 2 * j + t))
            near.append(len(frames))
            small()
        frames.append(base[:j])
        small(run)
    empty(512)
    small(max(n_small - count[0], 1))
    empty(1)
    return frames, jumbo, near


def jumbo_positions(p, L):
    """Byte positions inside a frame of L bytes at buffer offset p where a summing kernel changes
    hands: 14, 33, 34, both ends of the first and of the last 16-B buffer chunk the segment touches
    (and the byte on the other side of each inner edge), and the last byte."""
    e0 = ((p + 34) | 15) - p       # last byte of the first chunk
    s1 = ((p + L - 1) & ~15) - p   # first byte of the last chunk
    return sorted({14, 33, 34, e0, e0 + 1, s1 - 1, s1, L - 1})
