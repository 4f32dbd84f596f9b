"""pbgpu_verify_wire's definition (include/pbgpu.h) restated: struct and Python
integers, big-endian sums.  Shares no code with pyverify, pyxlat, pyencap or the library; every
rule is read off RFC 791, 768, 793, 792, 8200, 4443, 7348 and IEEE 802.1Q / 802.1ad."""
import struct

L3_CSUM, L3_LEN, L4_CSUM, UDP_LEN = 1, 2, 4, 8
ALL = 15
MALFORMED, NOL4, INNER, OTHER = 16, 32, 64, 128
BAD = 31  # the bits that make a frame bad


def be16(F: bytes, o: int) -> int:
    return struct.unpack_from(">H", F, o)[0]


def sum16(b: bytes) -> int:
    """Big-endian 16-bit words added, an odd last byte padded as the high byte; folded."""
    if len(b) & 1:
        b = b + b"\x00"
    s = sum(struct.unpack(">%dH" % (len(b) // 2), b))
    while s > 0xFFFF:
        s = (s & 0xFFFF) + (s >> 16)
    return s


class _Walk:
    def __init__(self, port):
        self.port = port
        self.evaluated = False
        self.malformed = False
        self.l3 = 0  # 4 / 6: the outermost ethertype


def _level(F: bytes, b: int, e: int, depth: int, w: _Walk) -> int:
    """The bits of F[b:e), every failure bit as if enabled."""
    def malformed():
        w.malformed = True
        return MALFORMED

    # 1. Ethernet
    if e - b < 14:
        return malformed()
    o, tags = b + 12, 0
    while tags < 2 and o + 2 <= e and be16(F, o) in (0x8100, 0x88A8):
        o += 4
        tags += 1
    if o + 2 > e:
        return malformed()
    et, l3 = be16(F, o), o + 2
    bits = 0
    # 2. not IP
    if et not in (0x0800, 0x86DD):
        return OTHER if depth == 0 else 0
    if depth == 0:
        w.l3 = 4 if et == 0x0800 else 6
    if et == 0x0800:
        # 3. IPv4
        if l3 + 20 > e or F[l3] >> 4 != 4:
            return malformed()
        ihl = 4 * (F[l3] & 15)
        if ihl < 20 or l3 + ihl > e:
            return malformed()
        if sum16(F[l3:l3 + ihl]) != 0xFFFF:
            bits |= L3_CSUM
        if be16(F, l3 + 2) != e - l3:
            bits |= L3_LEN
        l4, S = l3 + ihl, e - l3 - ihl
        if be16(F, l3 + 6) & 0x3FFF:
            return bits  # a fragment
        proto = F[l3 + 9]
        pseudo = F[l3 + 12:l3 + 20] + struct.pack(">BBH", 0, proto, S)
        six = False
    else:
        # 4. IPv6
        if l3 + 40 > e or F[l3] >> 4 != 6:
            return malformed()
        if be16(F, l3 + 4) != e - l3 - 40:
            bits |= L3_LEN
        l4, S = l3 + 40, e - l3 - 40
        proto = F[l3 + 6]
        pseudo = F[l3 + 8:l3 + 40] + struct.pack(">IBBBB", S, 0, 0, 0, proto)
        six = True
    seg = F[l4:e]
    if proto == 17:
        if S < 8:
            return malformed()
        if be16(F, l4 + 4) != S:
            bits |= UDP_LEN
        if seg[6:8] == b"\x00\x00":
            if six:
                bits |= L4_CSUM
                w.evaluated = True
        else:
            w.evaluated = True
            if sum16(pseudo + seg) != 0xFFFF:
                bits |= L4_CSUM
        # 5. VXLAN
        if depth == 0 and w.port and be16(F, l4 + 2) == w.port and S >= 16 and F[l4 + 8] & 0x08:
            bits |= INNER
            bits |= _level(F, l4 + 16, e, 1, w)
    elif proto == 6:
        if S < 20:
            return malformed()
        w.evaluated = True
        if sum16(pseudo + seg) != 0xFFFF:
            bits |= L4_CSUM
    elif proto == 1 and not six:
        if S < 8:
            return malformed()
        w.evaluated = True
        if sum16(seg) != 0xFFFF:
            bits |= L4_CSUM
    elif proto == 58 and six:
        if S < 4:
            return malformed()
        w.evaluated = True
        if sum16(pseudo + seg) != 0xFFFF:
            bits |= L4_CSUM
    return bits


def walk(F: bytes, checks: int = ALL, vxlan_port: int = 0):
    """(code, 4 / 6 / 0 by the outermost ethertype)."""
    F = bytes(F)
    w = _Walk(vxlan_port)
    bits = _level(F, 0, len(F), 0, w)
    code = bits & (checks & ALL) | bits & (MALFORMED | INNER | OTHER)
    if not (bits & OTHER) and not w.malformed and not w.evaluated:
        code |= NOL4
    return code, w.l3


def code(F: bytes, checks: int = ALL, vxlan_port: int = 0) -> int:
    return walk(F, checks, vxlan_port)[0]


FIELDS = ("n_checked", "n_bad", "bad_malformed", "bad_l3_csum", "bad_l3_len", "bad_l4_csum", "bad_udp_len",
          "first_bad", "n_ipv4", "n_ipv6", "n_inner", "n_nol4", "n_other")


def result(frames, checks: int = ALL, vxlan_port: int = 0, first: int = 0):
    """(codes, the result's fields but device_ms) of a range of frames whose first has index `first`."""
    r = dict.fromkeys(FIELDS, 0)
    r["first_bad"] = 2 ** 64 - 1
    codes = []
    for j, F in enumerate(frames):
        c, l3 = walk(F, checks, vxlan_port)
        codes.append(c)
        r["n_checked"] += 1
        if c & BAD:
            r["n_bad"] += 1
            r["first_bad"] = min(r["first_bad"], first + j)
        for bit, name in ((MALFORMED, "bad_malformed"), (L3_CSUM, "bad_l3_csum"), (L3_LEN, "bad_l3_len"),
                          (L4_CSUM, "bad_l4_csum"), (UDP_LEN, "bad_udp_len"), (INNER, "n_inner"), (NOL4, "n_nol4"),
                          (OTHER, "n_other")):
            r[name] += bool(c & bit)
        r["n_ipv4"] += l3 == 4
        r["n_ipv6"] += l3 == 6
    return codes, r
