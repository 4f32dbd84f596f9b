"""Clean frames by class for the pbgpu_verify_wire tests: every frame with correct checksums and
lengths, composed here header by header (struct and integers; the checksums are summed by this
file's own csum(), not by the checker under test)."""
import struct

import numpy as np

VXLAN_PORT = 4789
PAYLOADS = (0, 1, 2, 15, 16, 17, 33)
TAGS = ("none", "q", "adq")            # no tag, one 8100, 88A8 + 8100
L3S = ("v4", "v4o6", "v4o15", "v6")    # IPv4 with IHL 5, 6, 15; IPv6
L4S = ("udp", "udp0", "tcp", "icmp", "gre", "frag_first", "frag_later", "ext44")
WRAPS = ("alone", "vx4_zero", "vx4_csum", "vx6")


def csum(b: bytes) -> int:
    if len(b) & 1:
        b += b"\x00"
    s = sum(struct.unpack(">%dH" % (len(b) // 2), b))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def _rb(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def eth(rng, tags: str, ethertype: int) -> bytes:
    t = {"none": b"", "q": struct.pack(">HH", 0x8100, 0x2064),
         "adq": struct.pack(">HHHH", 0x88A8, 0x0123, 0x8100, 0x0064)}[tags]
    return _rb(rng, 12) + t + struct.pack(">H", ethertype)


def l4_segment(rng, l4: str, six: bool, src: bytes, dst: bytes, payload: bytes, dport: int = None):
    """(protocol / next header, the L4 segment with its checksum) for an unfragmented packet."""
    def pseudo(proto, n):
        return src + dst + (struct.pack(">IBBBB", n, 0, 0, 0, proto) if six else struct.pack(">BBH", 0, proto, n))

    if l4 in ("udp", "udp0"):
        n = 8 + len(payload)
        seg = struct.pack(">HHHH", int(rng.integers(1024, 4000)), dport or int(rng.integers(5000, 60000)), n, 0) + payload
        if l4 == "udp0":
            return 17, seg
        c = csum(pseudo(17, n) + seg) or 0xFFFF
        return 17, seg[:6] + struct.pack(">H", c) + seg[8:]
    if l4 == "tcp":
        seg = _rb(rng, 12) + b"\x50\x18" + _rb(rng, 2) + b"\x00\x00" + _rb(rng, 2) + payload
        return 6, seg[:16] + struct.pack(">H", csum(pseudo(6, len(seg)) + seg)) + seg[18:]
    if l4 == "icmp":
        seg = bytes([128 if six else 8, 0, 0, 0]) + _rb(rng, 4) + payload
        c = csum((pseudo(58, len(seg)) if six else b"") + seg)
        return (58 if six else 1), seg[:2] + struct.pack(">H", c) + seg[4:]
    if l4 == "gre":
        return 47, b"\x00\x00\x08\x00" + payload
    if l4 == "ext44":
        return 44, bytes([17, 0, 0, 1]) + _rb(rng, 4) + payload
    raise ValueError(l4)


def packet(rng, l3: str, l4: str, payload: bytes, dport: int = None) -> bytes:
    """The L3 packet.  'icmp' is ICMPv6 under IPv6; the fragment classes and a UDP checksum of 00 00
    exist for IPv4 and ext44 for IPv6 only (None otherwise)."""
    six = l3 == "v6"
    if (l4.startswith("frag") and six) or (l4 == "ext44" and not six) or (l4 == "udp0" and six):
        return None
    src, dst = _rb(rng, 16 if six else 4), _rb(rng, 16 if six else 4)
    if l4.startswith("frag"):
        proto, seg = 17, _rb(rng, 8) + payload  # the bytes of a fragment are not an L4 header
        fo = 0x2000 if l4 == "frag_first" else 0x00B9
    else:
        proto, seg = l4_segment(rng, l4, six, src, dst, payload, dport)
        fo = 0x4000 if rng.integers(0, 2) else 0
    if six:
        return struct.pack(">IHBB", 0x60000000 | int(rng.integers(0, 1 << 28)), len(seg), proto,
                           int(rng.integers(1, 256))) + src + dst + seg
    ihl = {"v4": 5, "v4o6": 6, "v4o15": 15}[l3]
    opts = (b"\x94\x04\x00\x00" + b"\x01" * (4 * ihl - 24)) if ihl > 5 else b""
    h = struct.pack(">BBHHHBBH", 0x40 | ihl, int(rng.integers(0, 256)), 4 * ihl + len(seg), int(rng.integers(0, 65536)),
                    fo, int(rng.integers(1, 256)), proto, 0) + src + dst + opts
    return h[:10] + struct.pack(">H", csum(h)) + h[12:] + seg


def frame(rng, tags="none", l3="v4", l4="udp", plen=16, wrap="alone", outer_tags="none") -> bytes:
    """One clean frame of the class, or None where the class does not exist."""
    p = packet(rng, l3, l4, _rb(rng, plen))
    if p is None:
        return None
    f = eth(rng, tags, 0x86DD if l3 == "v6" else 0x0800) + p
    if wrap == "alone":
        return f
    vx = b"\x08\x00\x00\x00" + _rb(rng, 3) + b"\x00" + f
    ol3 = "v6" if wrap == "vx6" else "v4"
    ol4 = "udp0" if wrap == "vx4_zero" else "udp"
    return eth(rng, outer_tags, 0x86DD if ol3 == "v6" else 0x0800) + packet(rng, ol3, ol4, vx, dport=VXLAN_PORT)


def long_frame(kind: str, L: int, seed: int = 7, fill: int = None) -> bytes:
    """A clean frame of exactly L bytes: 'vx4' an IPv4 UDP frame inside VXLAN over IPv4 with a computed
    outer UDP checksum (both of its ranges are summed), 'vx4_zero' the same with an outer 00 00,
    'tcp6' an IPv6 TCP frame.  fill: every payload byte."""
    rng = np.random.default_rng([seed, L])
    if kind == "tcp6":
        pl = L - 74
        payload = _rb(rng, pl) if fill is None else bytes([fill]) * pl
        src, dst = (_rb(rng, 16), _rb(rng, 16)) if fill is None else (bytes([fill]) * 16,) * 2
        _, seg = l4_segment(rng, "tcp", True, src, dst, payload)
        f = eth(rng, "none", 0x86DD) + struct.pack(">IHBB", 0x60000000, len(seg), 6, 64) + src + dst + seg
    else:
        pl = L - 92
        inner = eth(rng, "none", 0x0800) + packet(rng, "v4", "udp", _rb(rng, pl) if fill is None else bytes([fill]) * pl)
        vx = b"\x08\x00\x00\x00" + _rb(rng, 3) + b"\x00" + inner
        f = eth(rng, "none", 0x0800) + packet(rng, "v4", "udp0" if kind == "vx4_zero" else "udp", vx, dport=VXLAN_PORT)
    assert len(f) == L
    return f


def zoo(seed: int = 1, payloads=PAYLOADS):
    """[(label, frame)]: every L3 x L4 class at every payload length untagged and alone, and at 17
    bytes of payload under every tagging and wrapping (tags on the inner and, for the wrappings, once
    on the outer frame)."""
    rng = np.random.default_rng(seed)
    out = []
    for l3 in L3S:
        for l4 in L4S:
            for pl in payloads:
                f = frame(rng, "none", l3, l4, pl)
                if f is not None:
                    out.append((f"{l3}-{l4}-{pl}", f))
            for tags in TAGS:
                for wrap in WRAPS:
                    if tags == "none" and wrap == "alone":
                        continue
                    f = frame(rng, tags, l3, l4, 17, wrap)
                    if f is not None:
                        out.append((f"{tags}-{l3}-{l4}-17-{wrap}", f))
            f = frame(rng, "none", l3, l4, 1, "vx4_csum", outer_tags="adq")
            if f is not None:
                out.append((f"{l3}-{l4}-1-vx4_csum-outer-adq", f))
    return out


def expected_info(label: str) -> int:
    """The info bits (NOL4 32, INNER 64) a zoo frame's class implies under port VXLAN_PORT."""
    label = "-" + label
    wrapped = "-vx" in label
    inner_eval = any(f"-{k}-" in label for k in ("udp", "tcp", "icmp"))
    outer_eval = "vx4_csum" in label or "vx6" in label
    code = 64 if wrapped else 0
    if not (inner_eval or (wrapped and outer_eval)):
        code |= 32
    return code


def pack(frames):
    """(bytes as np.uint8, offsets as np.uint64) of frames packed back to back."""
    off = np.zeros(len(frames) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(f) for f in frames])
    return np.frombuffer(b"".join(frames), dtype=np.uint8).copy(), off


def mutants(f: bytes):
    """One copy per byte position with that byte changed (one bit, by position)."""
    out = []
    for i in range(len(f)):
        m = bytearray(f)
        m[i] ^= 1 << (i % 8)
        out.append(bytes(m))
    return out
