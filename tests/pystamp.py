"""The stamp in plain Python, straight from the definition in include/pbgpu.h (pbgpu_stamp): the
reference the stamp tests compare against byte for byte.  `struct` and Python integers only."""
import struct

STAMP_LEN = 16
CSUM_AT = {17: 40, 6: 50, 1: 36}


def stamp_time(index, t0_ns, step_ps):
    """T of the frame with global index `index` (as pypcap.stamp, before the split into fields)."""
    return t0_ns + (index * step_ps) // 1000


def position(frame, offset=0, tail=False):
    """('stamped', S, Q) where the 16 bytes go and where the L4 checksum is, or ('short' | 'other',
    None, None) for a frame that stays as it is."""
    L = len(frame)
    if L < 34 or frame[12:14] != b"\x08\x00" or frame[14] != 0x45:
        return "other", None, None
    if struct.unpack("!H", frame[20:22])[0] & 0x3FFF:
        return "other", None, None
    proto = frame[23]
    if proto not in CSUM_AT:
        return "other", None, None
    if proto == 6:
        if L < 47:
            return "short", None, None
        H = 4 * (frame[46] >> 4)
        if H < 20:
            return "other", None, None
    else:
        H = 8
    P0 = 34 + H
    S = L - STAMP_LEN - offset if tail else P0 + offset
    if not (P0 <= S and S + STAMP_LEN <= L):
        return "short", None, None
    return "stamped", S, CSUM_AT[proto]


def _words(frame, a):
    """The big-endian 16-bit words of the L4 segment at even segment offsets that intersect
    [a, a + 16); a byte at or past the frame's end counts as 0."""
    seg = frame[34:]
    out = []
    for w in range(a & ~1, a + STAMP_LEN, 2):
        hi = seg[w] if w < len(seg) else 0
        lo = seg[w + 1] if w + 1 < len(seg) else 0
        out.append((hi << 8) | lo)
    return out


def stamp(frame, index, T, offset=0, tail=False, csum=True):
    """-> (bytes, 'stamped' | 'short' | 'other')."""
    frame = bytes(frame)
    cls, S, Q = position(frame, offset, tail)
    if cls != "stamped":
        return frame, cls
    out = bytearray(frame)
    out[S:S + STAMP_LEN] = struct.pack("!QQ", index & (2**64 - 1), T & (2**64 - 1))
    if csum:
        a = S - 34
        old, new = _words(frame, a), _words(bytes(out), a)
        assert len(old) == (9 if a & 1 else 8)
        C = struct.unpack("!H", frame[Q:Q + 2])[0]
        s = (~C & 0xFFFF) + sum(~w & 0xFFFF for w in old) + sum(new)
        while s >> 16:
            s = (s & 0xFFFF) + (s >> 16)
        out[Q:Q + 2] = struct.pack("!H", ~s & 0xFFFF)
    return bytes(out), cls


def stamp_buffer(data, offsets, first=0, n=None, t0_ns=0, step_ps=0, first_index=0, offset=0, tail=False, csum=True):
    """pbgpu_stamp over a packed buffer: `data` (bytes-like, the whole capacity if wanted), `offsets`
    (n_frames + 1 entries).  -> (the new bytes, {'stamped': .., 'short': .., 'other': ..})."""
    out = bytearray(bytes(data))
    if n is None:
        n = len(offsets) - 1 - first
    counts = {"stamped": 0, "short": 0, "other": 0}
    for j in range(n):
        o0, o1 = int(offsets[first + j]), int(offsets[first + j + 1])
        idx = first_index + j
        f, cls = stamp(bytes(out[o0:o1]), idx, stamp_time(idx, t0_ns, step_ps), offset, tail, csum)
        out[o0:o1] = f
        counts[cls] += 1
    return bytes(out), counts
