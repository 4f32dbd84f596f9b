"""IPv4-to-IPv6 translated frames from their definition (include/pbgpu.h), with struct
and Python integers only: the reference the translation tests compare against.

Two halves that share no arithmetic.  xlat46() follows the definition, incremental checksum
updates included.  check6() knows nothing of IPv4 or of increments: it takes an IPv6 frame, builds
the pseudo header of RFC 8200 section 8.1 and sums the whole segment."""
import socket
import struct

OTHER = "other"


def prefix96(text: str) -> bytes:
    """'64:ff9b::' or '64:ff9b::/96' as the 12 prefix bytes."""
    addr, _, plen = text.partition("/")
    if plen not in ("", "96"):
        raise ValueError("only /96")
    b = socket.inet_pton(socket.AF_INET6, addr)
    if b[12:] != bytes(4):
        raise ValueError("address bits beyond the /96")
    return b[:12]


def classify(F: bytes) -> str:
    """'udp', 'tcp', 'icmp' or OTHER."""
    L = len(F)
    if L < 34 or F[12:14] != b"\x08\x00" or F[14] != 0x45:
        return OTHER
    if struct.unpack(">H", F[20:22])[0] & 0x3FFF:
        return OTHER
    if F[23] == 17 and L >= 42:
        return "udp"
    if F[23] == 6 and L >= 54:
        return "tcp"
    if F[23] == 1 and L >= 42 and F[34] in (8, 0):
        return "icmp"
    return OTHER


def fold(s: int) -> int:
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def words(b: bytes) -> int:
    return sum(struct.unpack(">%dH" % (len(b) // 2), b))


def flow_hash(F: bytes) -> int:
    """pbgpu_encap's hash of source bytes 26..37 up to x ^= x >> 15 (w2 = 0 for ICMP), 20 bits of it."""
    w0, w1, w2 = struct.unpack("<III", F[26:38])
    if F[23] == 1:
        w2 = 0
    x = w0 ^ w1 ^ w2
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    return x & 0xFFFFF


def xlat46(F: bytes, src_prefix: bytes, dst_prefix: bytes = None, flow_label: int = 0, hash_flow: bool = False):
    """The translated frame, or None for a frame that is `other`."""
    if dst_prefix is None:
        dst_prefix = src_prefix
    kind = classify(F)
    if kind == OTHER:
        return None
    L = len(F)
    tc = F[15]
    fl = flow_hash(F) if hash_flow else flow_label
    nh = {"udp": 17, "tcp": 6, "icmp": 58}[kind]
    src6 = bytes(src_prefix) + F[26:30]
    dst6 = bytes(dst_prefix) + F[30:34]
    hdr = F[0:12] + b"\x86\xdd" + bytes([0x60 | tc >> 4, (tc & 15) << 4 | fl >> 16]) + \
        struct.pack(">HHBB", fl & 0xFFFF, L - 34, nh, F[22]) + src6 + dst6
    l4 = bytearray(F[34:])
    K = words(bytes(src_prefix)) + words(bytes(dst_prefix))
    if kind == "udp":
        C = struct.unpack(">H", F[40:42])[0]
        r = ~fold((~C & 0xFFFF) + K) & 0xFFFF
        l4[6:8] = struct.pack(">H", r or 0xFFFF)
    elif kind == "tcp":
        C = struct.unpack(">H", F[50:52])[0]
        r = ~fold((~C & 0xFFFF) + K) & 0xFFFF
        l4[16:18] = struct.pack(">H", r)
    else:
        C = struct.unpack(">H", F[36:38])[0]
        w = struct.unpack(">H", F[34:36])[0]
        w2 = ((128 if F[34] == 8 else 129) << 8) | (w & 0xFF)
        PS = words(src6) + words(dst6) + (L - 34) + 58
        r = ~fold((~C & 0xFFFF) + (~w & 0xFFFF) + w2 + PS) & 0xFFFF
        l4[0] = w2 >> 8
        l4[2:4] = struct.pack(">H", r)
    return hdr + bytes(l4)


def xlat_all(frames, *a, **kw):
    return [xlat46(f, *a, **kw) for f in frames]


# ---------------------------------------------------------------- the from-scratch checker
def segment_sum(G: bytes) -> int:
    """An Ethernet + IPv6 frame's upper-layer checksum sum, folded: RFC 8200 8.1's pseudo header
    (source address, destination address, upper-layer length as 32 bits, 3 zero bytes, next header)
    and the whole segment, an odd last byte padded with a zero byte.  0xFFFF means good."""
    seg = G[54:]
    nh = G[20]
    pseudo = G[22:38] + G[38:54] + struct.pack(">I", len(seg)) + b"\x00\x00\x00" + bytes([nh])
    if len(seg) & 1:
        seg = seg + b"\x00"
    s = 0
    for i in range(0, len(pseudo), 2):
        s += (pseudo[i] << 8) | pseudo[i + 1]
    for i in range(0, len(seg), 2):
        s += (seg[i] << 8) | seg[i + 1]
    while s > 0xFFFF:
        s = (s >> 16) + (s & 0xFFFF)
    return s


def check6(G: bytes) -> bool:
    """Good: ethertype 86 DD, version 6, payload length = the frame's, next header UDP / TCP /
    ICMPv6, and the checksum over pseudo header and segment folds to 0xFFFF; a UDP checksum field
    of 0 is never good (RFC 8200 8.1)."""
    if len(G) < 54 or G[12:14] != b"\x86\xdd" or G[14] >> 4 != 6:
        return False
    if (G[18] << 8 | G[19]) != len(G) - 54 or G[20] not in (17, 6, 58):
        return False
    if G[20] == 17 and G[60:62] == b"\x00\x00":
        return False
    return segment_sum(G) == 0xFFFF


def set_csum6(G: bytes) -> bytes:
    """G with its upper-layer checksum field computed from scratch (for known-answer frames)."""
    at = {17: 60, 6: 70, 58: 56}[G[20]]
    Z = G[:at] + b"\x00\x00" + G[at + 2:]
    c = ~segment_sum(Z) & 0xFFFF
    if G[20] == 17 and c == 0:
        c = 0xFFFF
    return Z[:at] + struct.pack(">H", c) + Z[at + 2:]


# ---------------------------------------------------------------- IPv4 test frames
def frame4(kind: str, L: int, rng, tos: int = None, icmp_type: int = 8, l4_csum: int = None) -> bytes:
    """An Ethernet + IPv4 + UDP / TCP / ICMP frame of L bytes with random addresses, ports and
    payload and good checksums (summed from scratch here); l4_csum forces the stored L4 checksum."""
    proto = {"udp": 17, "tcp": 6, "icmp": 1}[kind]
    rb = lambda n: rng.integers(0, 256, n, dtype="uint8").tobytes()
    tos = int(rng.integers(0, 256)) if tos is None else tos
    ip = struct.pack(">BBHHHBBH", 0x45, tos, L - 14, int(rng.integers(0, 65536)), 0x4000 if rng.integers(0, 2) else 0,
                     int(rng.integers(1, 256)), proto, 0) + rb(8)
    ip = ip[:10] + struct.pack(">H", ~fold(words(ip)) & 0xFFFF) + ip[12:]
    body = L - 34
    if kind == "udp":
        l4, at = rb(4) + struct.pack(">HH", body, 0) + rb(body - 8), 6
    elif kind == "tcp":
        l4, at = rb(12) + b"\x50\x02" + rb(2) + b"\x00\x00" + rb(2) + rb(body - 20), 16
    else:
        l4, at = bytes([icmp_type, 0, 0, 0]) + rb(body - 4), 2
    if l4_csum is None:
        pseudo = b"" if kind == "icmp" else ip[12:20] + struct.pack(">HH", proto, body)
        l4_csum = ~fold(words(pseudo + l4 + (b"\x00" if body & 1 else b""))) & 0xFFFF
    l4 = l4[:at] + struct.pack(">H", l4_csum) + l4[at + 2:]
    return rb(12) + b"\x08\x00" + ip + l4
