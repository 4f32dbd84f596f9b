"""Frames for the segmentation tests (test_seg_cpu.py, test_gpu_seg.py): TCP and UDP frames with
every stored length and checksum right, and one frame of each class pbgpu_segment copies."""
import struct

import numpy as np

import pyverify

ETH = bytes.fromhex("0a0b0c0d0e0f" "1a1b1c1d1e1f" "0800")
ADDR = bytes([10, 20, 0, 1, 10, 60, 0, 195])


def payload(P: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, P, dtype=np.uint8).tobytes()


def finish(f: bytearray) -> bytes:
    """tot_len, the IPv4 checksum and the L4 checksum of a TCP / UDP frame set from its bytes."""
    f[16:18] = struct.pack("!H", len(f) - 14)
    f[24:26] = b"\x00\x00"
    f[24:26] = struct.pack("!H", pyverify.ip_csum_value(bytes(f)))
    at = 40 if f[23] == 17 else 50
    c = pyverify.l4_csum_value(bytes(f))
    f[at:at + 2] = struct.pack("!H", 0xFFFF if (c == 0 and f[23] == 17) else c)
    return bytes(f)


def udp(P: int, seed: int = 0, ident: int = 0x1234, pay: bytes = None, fo: int = 0x4000) -> bytes:
    pay = payload(P, seed) if pay is None else pay
    ip = struct.pack("!BBHHHBBH", 0x45, seed & 0xFF, 0, ident & 0xFFFF, fo, 64, 17, 0) + ADDR
    l4 = struct.pack("!HHHH", 0x1234, 0x6987, 8 + len(pay), 0)
    return finish(bytearray(ETH + ip + l4 + pay))


def tcp(P: int, seed: int = 0, ident: int = 0x1234, seq: int = 0x01020304, flags: int = 0x18, H: int = 20,
        pay: bytes = None, fo: int = 0x4000) -> bytes:
    pay = payload(P, seed) if pay is None else pay
    ip = struct.pack("!BBHHHBBH", 0x45, seed & 0xFF, 0, ident & 0xFFFF, fo, 64, 6, 0) + ADDR
    opts = bytes((0x11 * (i + 1) + seed) & 0xFF for i in range(H - 20))
    l4 = struct.pack("!HHIIBBHHH", 0x1234, 0x01BB, seq & 0xFFFFFFFF, 0x0A0B0C0D, (H // 4) << 4, flags, 0x0200, 0, 0)
    return finish(bytearray(ETH + ip + l4 + opts + pay))


def udp_zero_first(mss: int, seed: int = 0) -> bytes:
    """A UDP frame of 2 mss + 3 payload bytes whose first segment at `mss` (even) has a computed
    checksum of 0x0000: the slice's last word is set to what the rest of the sum leaves open."""
    pay = bytearray(payload(2 * mss + 3, seed))
    pay[mss - 2:mss] = b"\x00\x00"
    f = udp(len(pay), seed, pay=bytes(pay))
    rest = pyverify.ones_sum(f[26:34] + struct.pack("!HH", 17, 8 + mss) + f[34:38] + struct.pack("!HH", 8 + mss, 0) +
                             bytes(pay[:mss]))
    pay[mss - 2:mss] = struct.pack("!H", (0xFFFF - rest) % 0xFFFF)
    return udp(len(pay), seed, pay=bytes(pay))


def ineligible(L: int, seed: int = 0) -> dict:
    """One frame of L >= 60 bytes of each class that is copied unchanged, by name."""
    out = {}
    f = bytearray(udp(L - 42, seed))
    f[23] = 1  # ICMP
    out["icmp"] = bytes(f)
    out["first_fragment"] = udp(L - 42, seed, fo=0x2000)
    out["later_fragment"] = udp(L - 42, seed, fo=0x0010)
    f = bytearray(udp(L - 42, seed))
    f[14] = 0x46
    out["ihl6"] = bytes(f)
    f = bytearray(udp(L - 42, seed))
    f[12:14] = b"\x86\xdd"
    out["not_ipv4"] = bytes(f)
    f = bytearray(tcp(L - 54, seed))
    f[46] = 0x40
    out["tcp_doff4"] = bytes(f)
    f = bytearray(tcp(L - 54, seed))
    f[23] = 47  # GRE: neither TCP nor UDP
    out["other_proto"] = bytes(f)
    return out
