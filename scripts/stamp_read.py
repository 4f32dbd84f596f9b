#!/usr/bin/env python3
"""Reads the stamps of a capture back: stamp_read.py FILE head|tail[:OFF]

FILE is a pcap file (microsecond or nanosecond magic, little-endian) whose frames went through
pbgpu_stamp (pcktbatch-gpu --stamp) with the same position.  A frame carries a stamp where
pbgpu_stamp's eligibility rule (include/pbgpu.h) says so: Ethernet + IPv4 without options, not a
fragment, ICMP / TCP / UDP, and room for 16 bytes at the position.  The stamp is BE64(index),
BE64(T ns).

Prints one JSON line:
  frames, stamped      records in the file, records that carry a stamp
  min_index, max_index lowest and highest index seen (null without stamps)
  missing              indices in [min_index, max_index] that never arrived
  duplicates           arrivals of an index that had arrived before
  out_of_order         arrivals whose index is below the highest index seen before them
  delta_ns_min / _median / _max
                       record timestamp - T, in ns; in a microsecond file both sides are cut to
                       whole microseconds first, and the record's seconds are taken modulo 2^32 as
                       the file stores them
numpy only."""
import json
import sys

import numpy as np

MAGIC_US, MAGIC_NS = 0xA1B2C3D4, 0xA1B23C4D
CSUM_PROTOS = (1, 6, 17)


def parse_spec(spec):
    """'head', 'tail', 'head:OFF', 'tail:OFF' -> (tail, offset)."""
    where, _, off = spec.partition(":")
    if where not in ("head", "tail") or (_ and not off.isdigit()):
        raise ValueError("position is head[:OFF] or tail[:OFF], OFF in bytes: %r" % spec)
    offset = int(off) if off else 0
    if offset > 65535:
        raise ValueError("OFF is at most 65535: %r" % spec)
    return where == "tail", offset


def stamp_at(f, tail, offset):
    """Where frame f (a uint8 array) carries its stamp, or -1."""
    L = len(f)
    if L < 34 or f[12] != 0x08 or f[13] != 0x00 or f[14] != 0x45:
        return -1
    if ((int(f[20]) << 8) | int(f[21])) & 0x3FFF:
        return -1
    proto = int(f[23])
    if proto not in CSUM_PROTOS:
        return -1
    H = 8
    if proto == 6:
        if L < 47:
            return -1
        H = 4 * (int(f[46]) >> 4)
        if H < 20:
            return -1
    P0 = 34 + H
    S = L - 16 - offset if tail else P0 + offset
    return S if P0 <= S and S + 16 <= L else -1


def analyse(data, tail=False, offset=0):
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    if len(buf) < 24:
        raise ValueError("shorter than a pcap file header")
    magic = int(buf[:4].view("<u4")[0])
    if magic not in (MAGIC_US, MAGIC_NS):
        raise ValueError("not a little-endian pcap magic: %#x" % magic)
    nsec = magic == MAGIC_NS
    pos, frames = 24, 0
    idx, ts, rec = [], [], []
    while pos + 16 <= len(buf):
        sec, frac, caplen, _ = (int(v) for v in buf[pos:pos + 16].view("<u4"))
        pos += 16
        if pos + caplen > len(buf):
            raise ValueError("truncated record at %d" % (pos - 16))
        f = buf[pos:pos + caplen]
        pos += caplen
        frames += 1
        S = stamp_at(f, tail, offset)
        if S < 0:
            continue
        be = f[S:S + 16].view(">u8")
        idx.append(int(be[0]))
        ts.append(int(be[1]))
        rec.append((sec, frac))
    out = dict(frames=frames, stamped=len(idx), min_index=None, max_index=None, missing=0, duplicates=0,
               out_of_order=0, delta_ns_min=None, delta_ns_median=None, delta_ns_max=None)
    if not idx:
        return out
    a = np.array(idx, dtype=np.uint64)
    uniq = np.unique(a)
    lo, hi = int(uniq[0]), int(uniq[-1])
    out.update(min_index=lo, max_index=hi, missing=hi - lo + 1 - len(uniq), duplicates=len(a) - len(uniq))
    before = np.maximum.accumulate(a)
    out["out_of_order"] = int(np.count_nonzero(a[1:] < before[:-1]))
    deltas = []
    for (sec, frac), T in zip(rec, ts):
        t_sec, t_frac = (T // 10**9) % 2**32, T % 10**9
        if not nsec:
            t_frac, frac = t_frac // 1000 * 1000, frac * 1000
        deltas.append((sec - t_sec) * 10**9 + frac - t_frac)
    d = np.array(deltas, dtype=np.int64)
    out.update(delta_ns_min=int(d.min()), delta_ns_median=float(np.median(d)), delta_ns_max=int(d.max()))
    return out


def main(argv):
    if len(argv) != 3:
        sys.stderr.write(__doc__)
        return 2
    try:
        tail, offset = parse_spec(argv[2])
        with open(argv[1], "rb") as fh:
            res = analyse(fh.read(), tail, offset)
    except (OSError, ValueError) as e:
        sys.stderr.write("stamp_read: %s\n" % e)
        return 1
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
