"""Independent IPv4 fragmentation reference (pure Python, RFC 791/1071), written from the definition
of pbgpu_fragment in include/pbgpu.h.  Shares no code with the library."""
import struct


def _csum(hdr: bytes) -> int:
    s = sum(struct.unpack("!10H", hdr))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def _header(eth: bytes, ip: bytes, tot_len: int, frag: int) -> bytes:
    h = bytearray(ip)
    h[2:4] = struct.pack("!H", tot_len)
    h[6:8] = struct.pack("!H", frag)
    h[10:12] = b"\0\0"
    h[10:12] = struct.pack("!H", _csum(bytes(h)))
    return eth + bytes(h)


def classify(frame: bytes, mtu: int, ignore_df: bool = False) -> str:
    """'fit' (copied whole, no count), 'other', 'df' (copied whole, counted) or 'split'."""
    L = len(frame)
    if L - 14 <= mtu:
        return "fit"
    if L < 34 or frame[12:14] != b"\x08\x00" or frame[14] != 0x45:
        return "other"
    fo = struct.unpack("!H", frame[20:22])[0]
    if fo & 0x4000 and not ignore_df:
        return "df"
    return "split"


def fragment(frame: bytes, mtu: int, ignore_df: bool = False) -> list:
    assert 68 <= mtu <= 65535
    if classify(frame, mtu, ignore_df) != "split":
        return [bytes(frame)]
    fo = struct.unpack("!H", frame[20:22])[0]
    C = (mtu - 20) & ~7
    D = len(frame) - 34
    K = (D + C - 1) // C
    out = []
    for i in range(K):
        data = frame[34 + i * C:34 + min(D, (i + 1) * C)]
        mf = 0x2000 if i < K - 1 else fo & 0x2000
        frag = (fo & 0xC000) | mf | (((fo & 0x1FFF) + i * C // 8) & 0x1FFF)
        out.append(_header(frame[0:14], frame[14:34], 20 + len(data), frag) + data)
    return out


def reassemble(frames: list) -> bytes:
    """The unfragmented frame the fragments came from: sorted by offset, contiguous, MF on all but
    the last, tot_len, the fragment field (DF and the reserved bit kept) and the checksum restored."""
    if len(frames) == 1:
        return bytes(frames[0])
    parts = []
    for f in frames:
        assert len(f) >= 34 and f[12:14] == b"\x08\x00" and f[14] == 0x45
        assert f[0:14] == frames[0][0:14] and f[14:16] == frames[0][14:16] and f[18:20] == frames[0][18:20]
        assert f[22:24] == frames[0][22:24] and f[26:34] == frames[0][26:34]
        tot, _, frag = struct.unpack("!HHH", f[16:22])
        assert tot == len(f) - 14 and _csum(f[14:24] + b"\0\0" + f[26:34]) == struct.unpack("!H", f[24:26])[0]
        parts.append(((frag & 0x1FFF) * 8, frag, f[34:]))
    parts.sort(key=lambda p: p[0])
    assert parts[0][0] == 0
    data = b""
    for k, (off, frag, d) in enumerate(parts):
        assert off == len(data), "fragments not contiguous"
        assert bool(frag & 0x2000) == (k < len(parts) - 1), "MF"
        assert k == len(parts) - 1 or len(d) % 8 == 0
        data += d
    flags = parts[0][1] & 0xC000
    assert all(p[1] & 0xC000 == flags for p in parts)
    first = min(frames, key=lambda f: struct.unpack("!H", f[20:22])[0] & 0x1FFF)
    return _header(first[0:14], first[14:34], 20 + len(data), flags) + data


def fragment_all(frames: list, mtu: int, ignore_df: bool = False):
    """(output frames, counts) of a whole range, as pbgpu_frag_result counts them."""
    out, cnt = [], dict(n_in=len(frames), n_split=0, n_df=0, n_other=0)
    for f in frames:
        c = classify(f, mtu, ignore_df)
        cnt["n_split"] += c == "split"
        cnt["n_df"] += c == "df"
        cnt["n_other"] += c == "other"
        out += fragment(f, mtu, ignore_df)
    cnt["n_out"] = len(out)
    cnt["out_bytes"] = sum(len(f) for f in out)
    cnt["out_min_len"] = min((len(f) for f in out), default=0)
    cnt["out_max_len"] = max((len(f) for f in out), default=0)
    return out, cnt
