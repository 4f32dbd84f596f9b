"""The pcap stream in plain Python, straight from the stream definition in include/pbgpu.h: the
reference the pcap tests compare against byte for byte.  `struct` and Python integers only."""
import struct

MAGIC_US = 0xA1B2C3D4
MAGIC_NS = 0xA1B23C4D
FILE_HEADER_LEN = 24
RECORD_HEADER_LEN = 16


def pcap_file_header(nsec=False):
    """magic, version 2.4 as one word, thiszone 0, sigfigs 0, snaplen 65535, linktype 1 (Ethernet)."""
    return struct.pack("<6I", MAGIC_NS if nsec else MAGIC_US, 0x00040002, 0, 0, 65535, 1)


def stamp(index, t0_ns, step_ps, nsec=False):
    """(ts_sec, ts_frac) of the frame with global index `index`."""
    t = t0_ns + (index * step_ps) // 1000
    frac = t % 10**9
    return (t // 10**9) % 2**32, frac if nsec else frac // 1000


def pcap_stream(frames, t0_ns=0, step_ps=0, first_index=0, file_header=True, nsec=False):
    """The stream of `frames` (an iterable of bytes-like): frame j is stamped as index
    first_index + j."""
    out = [pcap_file_header(nsec)] if file_header else []
    for j, f in enumerate(frames):
        f = bytes(f)
        sec, frac = stamp(first_index + j, t0_ns, step_ps, nsec)
        out.append(struct.pack("<4I", sec, frac, len(f), len(f)))
        out.append(f)
    return b"".join(out)


def read_pcap(data):
    """A capture's (nsec, [(ts_sec, ts_frac, frame bytes)]); both little-endian magics; caplen must
    equal len (nothing here truncates) and the records must end exactly at the end."""
    data = bytes(data)
    if len(data) < FILE_HEADER_LEN:
        raise ValueError("shorter than a pcap file header")
    magic, version, zone, sigfigs, snaplen, link = struct.unpack_from("<6I", data, 0)
    if magic not in (MAGIC_US, MAGIC_NS):
        raise ValueError("not a little-endian pcap magic: %#x" % magic)
    if (version, zone, sigfigs, snaplen, link) != (0x00040002, 0, 0, 65535, 1):
        raise ValueError("unexpected pcap file header")
    recs, pos = [], FILE_HEADER_LEN
    while pos < len(data):
        if pos + RECORD_HEADER_LEN > len(data):
            raise ValueError("truncated record header at %d" % pos)
        sec, frac, caplen, length = struct.unpack_from("<4I", data, pos)
        pos += RECORD_HEADER_LEN
        if caplen != length or pos + caplen > len(data):
            raise ValueError("bad record lengths at %d" % (pos - RECORD_HEADER_LEN))
        recs.append((sec, frac, data[pos:pos + caplen]))
        pos += caplen
    return magic == MAGIC_NS, recs
