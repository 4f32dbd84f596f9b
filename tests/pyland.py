"""Reference model of the UMEM landing (pbgpu_copy_to_umem[_async], include/pbgpu.h), in numpy.

land() says what a landing leaves in the UMEM bytes: frame first_frame + j at
base + (first_slot + j) * stride, its length in lens[j], every other byte as it was.  The one
exception is the tight slot (fixed length, stride no longer than the frame rounded up to 64 B,
registered UMEM, scatter kernel), which is written whole: model it with whole=True."""
import numpy as np


def frame_bytes(j: int, length: int) -> np.ndarray:
    """Byte p of test frame j: a hash of (j, p), so that no shift, repeat or drop maps onto itself."""
    x = (np.arange(length, dtype=np.uint64) * np.uint64(40503) + np.uint64(j) * np.uint64(2654435761)
         + np.uint64(0x9E37)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(12)
    return (x & np.uint64(0xFF)).astype(np.uint8)


def round64(x: int) -> int:
    return (x + 63) & ~63


def is_tight(flen: int, stride: int) -> bool:
    return stride <= round64(flen)


def land(umem_before, frames, stride, first_slot, first_frame, n, base=0, whole=False, stream=None):
    """-> (umem_after, lens), and with whole=True -> (umem_after, lens, unspecified).

    frames: the buffer's frames (uint8 arrays).  whole=True: the rest of each slot holds the bytes
    that follow the frame in `stream`, the buffer's packed bytes (all its frames back to back);
    where the stream has none left, `unspecified` (bool, one per UMEM byte) is set and umem_after
    keeps the old byte."""
    out = np.array(umem_before, dtype=np.uint8, copy=True)
    lens = np.empty(n, dtype=np.uint16)
    unspecified = np.zeros(len(out), dtype=bool)
    pos = sum(len(f) for f in frames[:first_frame]) if whole else 0
    for j in range(n):
        f = frames[first_frame + j]
        at = base + (first_slot + j) * stride
        assert len(f) <= stride and at >= 0 and at + stride <= len(out)
        out[at:at + len(f)] = f
        lens[j] = len(f)
        if whole:
            pos += len(f)
            k = min(stride - len(f), max(0, len(stream) - pos))
            out[at + len(f):at + len(f) + k] = stream[pos:pos + k]
            unspecified[at + len(f) + k:at + stride] = True
    return (out, lens, unspecified) if whole else (out, lens)


def stream_pos(at, flen, stride, first_slot, first_frame, base):
    """The packed-stream position that UMEM byte `at` (array) of a whole-written fixed-length slot holds."""
    rel = at - base - first_slot * stride
    return (first_frame + rel // stride) * flen + rel % stride


def check_cap(unspecified, flen, stride, first_slot, first_frame, n, base, total):
    """The cap on what a comparison may leave out: only filler of the n landed slots whose stream
    position is at or past `total`, so fewer than stride - flen <= 63 positions behind it, and at most
    that many bytes of any slot."""
    at = np.flatnonzero(unspecified)
    if len(at) == 0:
        return
    assert is_tight(flen, stride) and stride - flen <= 63
    assert at.min() >= base + first_slot * stride and at.max() < base + (first_slot + n) * stride
    assert ((at - base) % stride >= flen).all()
    pos = stream_pos(at, flen, stride, first_slot, first_frame, base)
    assert pos.min() >= total and pos.max() < total + stride - flen
    assert np.bincount((at - base) // stride).max() <= stride - flen


# ---- the input sets of tests/test_gpu_landing.py (checked on the CPU by tests/test_land_cpu.py) ----

VAR_SHORT = list(range(81))
VAR_LONG = [255, 256, 257, 1499, 1500, 1501, 4095, 4096]
VAR_LMAX = 4096
VAR_STRIDES = sorted({4096, VAR_LMAX, VAR_LMAX + 1, VAR_LMAX + 2, VAR_LMAX + 3})


def var_blocks():
    """-> (lengths, blocks): 16 blocks, block k a prefix frame of 0..15 bytes that puts the next frame at a
    source offset of k mod 16, then one frame of every length of VAR_SHORT and VAR_LONG; blocks[k] =
    (first_frame, n) of block k without its prefix frame.  Each length meets every offset mod 16."""
    lengths, blocks, at = [], [], 0
    for k in range(16):
        p = (k - at) % 16
        lengths.append(p)
        at += p
        blocks.append((len(lengths), len(VAR_SHORT) + len(VAR_LONG)))
        lengths += VAR_SHORT + VAR_LONG
        at += sum(VAR_SHORT) + sum(VAR_LONG)
    return lengths, blocks


FIXED_LENS = [1, 2, 3, 4, 5, 59, 60, 61, 62, 63, 64, 65, 98, 127, 128, 129, 1500, 1501]
FIXED_N = 300
FIXED_BASES = [0, 2]


def fixed_strides(flen: int):
    return sorted({flen, flen + 1, flen + 3, round64(flen), round64(flen) + 1, 4096})


def fixed_ranges(n: int = FIXED_N):
    return [(0, n), (1, n - 1), (n - 3, 3)]
