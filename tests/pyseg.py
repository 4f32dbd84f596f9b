"""L4 segmentation as include/pbgpu.h defines it (pbgpu_segment), in `struct` and Python integers.

The first half writes the segments of a frame from the definition; the second half checks any
output from scratch: every segment's lengths and checksums, and that the segments' payloads
concatenate to the source's.  The checksum routine is this file's own; nothing here is shared with
the library or with the other py*.py references."""
import struct

NO_L4_CSUM = 1
FIXED_ID = 2


def ones_sum(data: bytes) -> int:
    """The RFC 1071 sum of big-endian 16-bit words (an odd last byte padded with 0), folded until no
    carry is left."""
    if len(data) & 1:
        data = data + b"\x00"
    s = 0
    for (w,) in struct.iter_unpack("!H", data):
        s += w
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def csum(data: bytes) -> int:
    return ~ones_sum(data) & 0xFFFF


def l4_header_len(f: bytes):
    """H of an eligible frame (8: UDP, 20..60: TCP), None where the frame is not eligible."""
    L = len(f)
    if L < 34 or f[12:14] != b"\x08\x00" or f[14] != 0x45:
        return None
    if struct.unpack("!H", f[20:22])[0] & 0x3FFF:
        return None
    if f[23] == 17 and L >= 42:
        return 8
    if f[23] == 6 and L >= 54:
        h = 4 * (f[46] >> 4)
        if 20 <= h and 34 + h <= L:
            return h
    return None


def classify(f: bytes, mss: int) -> str:
    """"tcp" / "udp": split; "other": not eligible with L - 42 > mss; "fit": copied and not counted."""
    h = l4_header_len(f)
    if h is None:
        return "other" if len(f) - 42 > mss else "fit"
    if len(f) - 34 - h <= mss:
        return "fit"
    return "udp" if h == 8 else "tcp"


def pseudo(f: bytes, proto: int, l4len: int) -> bytes:
    return bytes(f[26:34]) + struct.pack("!BBH", 0, proto, l4len)


def segment(f: bytes, mss: int, flags: int = 0) -> list:
    """The output frames of source frame f."""
    if not 8 <= mss <= 65535 or flags & ~3:
        raise ValueError("mss or flags")
    f = bytes(f)
    if classify(f, mss) in ("fit", "other"):
        return [f]
    h = l4_header_len(f)
    tcp = h != 8
    pay = f[34 + h:]
    k = -(-len(pay) // mss)
    ident = struct.unpack("!H", f[18:20])[0]
    seq = struct.unpack("!I", f[38:42])[0]
    out = []
    for i in range(k):
        part = pay[i * mss:(i + 1) * mss]
        ip = bytearray(f[14:34])
        ip[2:4] = struct.pack("!H", 20 + h + len(part))
        if not flags & FIXED_ID:
            ip[4:6] = struct.pack("!H", (ident + i) & 0xFFFF)
        ip[10:12] = b"\x00\x00"
        ip[10:12] = struct.pack("!H", csum(bytes(ip)))
        l4 = bytearray(f[34:34 + h])
        if tcp:
            l4[4:8] = struct.pack("!I", (seq + i * mss) & 0xFFFFFFFF)
            if i != k - 1:
                l4[13] &= ~0x09 & 0xFF
            if i != 0:
                l4[13] &= ~0x80 & 0xFF
            at = 16
        else:
            l4[4:6] = struct.pack("!H", 8 + len(part))
            at = 6
        if not flags & NO_L4_CSUM:
            l4[at:at + 2] = b"\x00\x00"
            c = csum(pseudo(f, 6 if tcp else 17, h + len(part)) + bytes(l4) + part)
            if not tcp and c == 0:
                c = 0xFFFF
            l4[at:at + 2] = struct.pack("!H", c)
        out.append(f[0:14] + bytes(ip) + bytes(l4) + part)
    return out


def segment_all(frames, mss: int, flags: int = 0):
    """(output frames, the pbgpu_seg_result fields but device_ms) of a range of frames."""
    out = []
    cnt = dict(n_in=len(frames), n_out=0, n_split_tcp=0, n_split_udp=0, n_other=0, out_bytes=0, out_min_len=0,
               out_max_len=0)
    for f in frames:
        c = classify(f, mss)
        if c == "tcp":
            cnt["n_split_tcp"] += 1
        elif c == "udp":
            cnt["n_split_udp"] += 1
        elif c == "other":
            cnt["n_other"] += 1
        out += segment(f, mss, flags)
    cnt["n_out"] = len(out)
    cnt["out_bytes"] = sum(len(x) for x in out)
    if out:
        cnt["out_min_len"] = min(len(x) for x in out)
        cnt["out_max_len"] = max(len(x) for x in out)
    return out, cnt


# ---------------------------------------------------------------- checking an output from scratch
def l4_ok(x: bytes) -> bool:
    """The L4 checksum of a whole (unfragmented) TCP or UDP frame holds; a UDP 00 00 is "none"."""
    h = l4_header_len(x)
    if h is None:
        return False
    if h == 8 and x[40:42] == b"\x00\x00":
        return True
    return ones_sum(pseudo(x, 17 if h == 8 else 6, len(x) - 34) + x[34:]) == 0xFFFF


def check_segments(src: bytes, segs, mss: int, flags: int = 0):
    """Raises AssertionError unless segs is a right segmentation of the eligible frame src: lengths,
    IDs, sequence numbers, flags, stored lengths, both checksums, and the payloads' concatenation."""
    h = l4_header_len(src)
    assert h is not None
    pay = src[34 + h:]
    k = -(-len(pay) // mss)
    assert len(segs) == k and k >= 2
    assert b"".join(x[34 + h:] for x in segs) == pay
    ident = struct.unpack("!H", src[18:20])[0]
    seq = struct.unpack("!I", src[38:42])[0]
    for i, x in enumerate(segs):
        pi = len(x) - 34 - h
        assert pi == (mss if i < k - 1 else len(pay) - (k - 1) * mss) and pi >= 1
        assert x[0:14] == src[0:14]
        assert struct.unpack("!H", x[16:18])[0] == len(x) - 14
        assert struct.unpack("!H", x[18:20])[0] == (ident if flags & FIXED_ID else (ident + i) & 0xFFFF)
        assert ones_sum(x[14:34]) == 0xFFFF
        assert x[14:16] == src[14:16] and x[20:24] == src[20:24] and x[26:34] == src[26:34]
        if h == 8:
            assert x[34:38] == src[34:38] and struct.unpack("!H", x[38:40])[0] == 8 + pi
            at = 40
        else:
            assert x[34:38] == src[34:38] and x[42:47] == src[42:47] and x[48:50] == src[48:50]
            assert x[52:34 + h] == src[52:34 + h]
            assert struct.unpack("!I", x[38:42])[0] == (seq + i * mss) & 0xFFFFFFFF
            want = src[47] & ~((0x09 if i != k - 1 else 0) | (0x80 if i else 0))
            assert x[47] == want
            at = 50
        if flags & NO_L4_CSUM:
            assert x[at:at + 2] == src[at:at + 2]
        else:
            assert l4_ok(x) and not (h == 8 and x[40:42] == b"\x00\x00")


def check_all(src_frames, out_frames, mss: int, flags: int = 0):
    """Walks an output against its source frames: copied frames equal, split ones by check_segments."""
    at = 0
    for f in src_frames:
        if classify(f, mss) in ("tcp", "udp"):
            h = l4_header_len(f)
            k = -(-(len(f) - 34 - h) // mss)
            check_segments(f, out_frames[at:at + k], mss, flags)
            at += k
        else:
            assert out_frames[at] == f
            at += 1
    assert at == len(out_frames)
