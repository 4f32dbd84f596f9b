"""Encapsulated frames from their definition (include/pbgpu.h), with struct and
Python integers only: the reference the encapsulation tests compare against."""
import struct


def vlan(frame: bytes, tci: int, tpid: int = 0x8100) -> bytes:
    """An 802.1Q tag after the MAC addresses."""
    return frame[:12] + struct.pack(">HH", tpid or 0x8100, tci) + frame[12:]


def sport(frame: bytes) -> int:
    """The hashed outer source port: frame bytes 26..37, a missing byte counting as 0."""
    w0, w1, w2 = struct.unpack("<III", (frame[26:38] + bytes(12))[:12])
    x = w0 ^ w1 ^ w2
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    return 49152 + (x & 0x3FFF)


def csum1071(b: bytes) -> int:
    s = sum(struct.unpack(">%dH" % (len(b) // 2), b))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def vxlan(frame: bytes, dst_mac: bytes, src_mac: bytes, src_ip: bytes, dst_ip: bytes, vni: int, src_port: int = 0,
          dst_port: int = 0, ttl: int = 0, tos: int = 0) -> bytes:
    """RFC 7348: outer Ethernet, IPv4 (DF, id 0), UDP (checksum 0) and VXLAN headers, then the frame."""
    L = len(frame)
    eth = bytes(dst_mac) + bytes(src_mac) + b"\x08\x00"
    ip = struct.pack(">BBHHHBBH", 0x45, tos, L + 36, 0, 0x4000, ttl or 64, 17, 0) + bytes(src_ip) + bytes(dst_ip)
    ip = ip[:10] + struct.pack(">H", csum1071(ip)) + ip[12:]
    udp = struct.pack(">HHHH", src_port or sport(frame), dst_port or 4789, L + 16, 0)
    vx = b"\x08\x00\x00\x00" + vni.to_bytes(3, "big") + b"\x00"
    return eth + ip + udp + vx + frame
