"""What the stamp tests share: a maker of UDP / TCP / ICMP frames whose checksums sit where the
protocols put them, the validity check (tests/pyverify.py's sums), and the packing helper."""
import struct

import numpy as np

import pystamp
import pyverify


def _l4_sum(frame):
    proto, l4 = frame[23], bytes(frame[34:])
    if proto in (6, 17):
        l4 = bytes(frame[26:34]) + struct.pack("!BBH", 0, proto, len(l4)) + l4
    return pyverify.ones_sum(l4)


def l4_ok(frame):
    """The L4 segment (with the pseudo header for TCP and UDP) folds to 0xFFFF, as pbgpu_verify asks."""
    return _l4_sum(bytes(frame)) == 0xFFFF


def frame_ok(frame):
    frame = bytes(frame)
    return pyverify.ip_csum_ok(frame) and struct.unpack("!H", frame[16:18])[0] == len(frame) - 14 and l4_ok(frame)


def l4_frame(proto, L, seed, doff=5, fo=0, ethertype=b"\x08\x00", vihl=0x45, csum=True):
    """L seeded random bytes made into an Ethernet + IPv4 frame of protocol `proto` (from 34 B on):
    tot_len and the IPv4 checksum hold, a TCP frame carries `doff`, and with csum the L4 checksum is
    written at its own place (UDP 40, TCP 50, ICMP 36) where the frame has room for it."""
    f = bytearray(np.random.default_rng([int(seed), int(L), int(proto)]).integers(0, 256, L, dtype=np.uint8).tobytes())
    if L < 34:
        return bytes(f)
    f[12:14] = ethertype
    f[14:24] = struct.pack("!BBHHHBB", vihl, seed & 0xFF, L - 14, seed & 0xFFFF, fo, 64, proto)
    f[24:26] = b"\0\0"
    f[24:26] = struct.pack("!H", pyverify.inet_csum(bytes(f[14:34])))
    if proto == 17 and L >= 40:
        f[38:40] = struct.pack("!H", L - 34)
    if proto == 6 and L >= 47:
        f[46] = (doff << 4) | (f[46] & 0x0F)
    Q = pystamp.CSUM_AT.get(proto)
    if csum and Q is not None and L >= Q + 2:
        f[Q:Q + 2] = b"\0\0"
        f[Q:Q + 2] = struct.pack("!H", 0xFFFF - _l4_sum(f))
    return bytes(f)


def pack(frames):
    """(data, offsets) of frames back to back."""
    off = np.concatenate([[0], np.cumsum([len(f) for f in frames], dtype=np.uint64)]).astype(np.uint64)
    return np.frombuffer(b"".join(bytes(f) for f in frames), dtype=np.uint8), off
