"""L4 segmentation without a GPU: the reference (tests/pyseg.py) against the two answers worked out
from the definition, against its own properties and the two other checkers (tests/pyverify.py,
tests/pywire.py), the ABI, and what pcktbatch-gpu --segment and the host driver refuse."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import pb_configs as pc
import pbgpu
import pyseg
import pyverify
import pywire
import seg_frames as sf
from cmdline_binding import OurCmd
from pbgpu import Sequence, SequenceT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pb-af-xdp_amd")
LIBDIR = os.path.join(PKG, "lib")
BIN = os.path.join(PKG, "bin", "pcktbatch-gpu")
BUILD = os.path.join(ROOT, "tests", "_build")

ETH = "0a0b0c0d0e0f" "1a1b1c1d1e1f" "0800"
IPS = "0a140001" "0a3c00c3"


def clean(x: bytes) -> bool:
    """Clean under both other checkers: pyverify's IPv4 checksum, tot_len and L4 checksum (a UDP sum of 0
    stored as 0xFFFF), and no pywire bit but the information ones."""
    d = pyverify.parse(x)
    want = pyverify.l4_csum_value(x)
    if d["proto"] == 17 and want == 0:
        want = 0xFFFF
    return (pyverify.ip_csum_ok(x) and d["tot_len"] == len(x) - 14 and d["l4_csum"] == want
            and pywire.code(x) & (pywire.BAD | pywire.NOL4) == 0)


# ---- the two known answers, byte for byte
def test_udp_at_mss_8_byte_by_byte():
    pay = bytes(range(0x01, 0x12))
    src = bytes.fromhex(ETH + "4500" "002d" "ffff" "4000" "4011" "25ad" + IPS + "1234" "6987" "0019" "1da5") + pay
    assert len(src) == 59 and clean(src)
    want = [
        bytes.fromhex(ETH + "4500" "0024" "ffff" "4000" "4011" "25b6" + IPS + "1234" "6987" "0010" "5eeb") + pay[0:8],
        bytes.fromhex(ETH + "4500" "0024" "0000" "4000" "4011" "25b6" + IPS + "1234" "6987" "0010" "3ecb") + pay[8:16],
        bytes.fromhex(ETH + "4500" "001d" "0001" "4000" "4011" "25bc" + IPS + "1234" "6987" "0009" "5e0d") + pay[16:],
    ]
    assert pyseg.segment(src, 8) == want
    assert all(clean(x) for x in want)
    assert pyseg.segment(src, 17) == [src] and pyseg.segment(src, 16) != [src]
    pyseg.check_segments(src, want, 8)


def test_tcp_at_mss_9_byte_by_byte():
    pay = bytes(range(0xA0, 0xB3))
    src = bytes.fromhex(ETH + "4500" "003b" "0007" "4000" "4006" "25a3" + IPS + "1234" "01bb" "fffffffe" "00000000"
                        "5099" "0200" "e43f" "0000") + pay
    assert len(src) == 73 and clean(src)
    rows = [("0031", "0007", "25ad", "fffffffe", "90", "4db7", pay[0:9]),
            ("0031", "0008", "25ac", "00000007", "10", "210b", pay[9:18]),
            ("0029", "0009", "25b3", "00000010", "19", "d2b7", pay[18:])]
    want = [bytes.fromhex(ETH + "4500" + tot + ident + "4000" "4006" + ipc + IPS + "1234" "01bb" + seq + "00000000"
                          "50" + fl + "0200" + l4c + "0000") + p for tot, ident, ipc, seq, fl, l4c, p in rows]
    assert pyseg.segment(src, 9) == want
    assert all(clean(x) for x in want)
    pyseg.check_segments(src, want, 9)


# ---- properties
MSSES = (8, 9, 536, 1448, 1460, 1472, 8960)


def _payload_lengths(mss, H):
    return sorted({0, 1, mss - 1, mss, mss + 1, 2 * mss - 1, 2 * mss, 2 * mss + 1, 65493 + 8 - H})


@pytest.mark.parametrize("mss", MSSES)
@pytest.mark.parametrize("proto,H", [("udp", 8), ("tcp", 20)])
def test_properties(mss, proto, H):
    for P in _payload_lengths(mss, H):
        f = sf.udp(P, P, ident=0x4321) if proto == "udp" else sf.tcp(P, P, ident=0x4321, seq=0x1000, flags=0xDB)
        assert len(f) == 34 + H + P <= 65535 and clean(f)
        out = pyseg.segment(f, mss)
        k = max(1, -(-P // mss))
        assert len(out) == k, P
        if k == 1:
            assert out == [f]
            continue
        assert [len(x) for x in out] == [34 + H + mss] * (k - 1) + [34 + H + P - (k - 1) * mss], P
        assert sum(len(x) for x in out) == len(f) + (k - 1) * (34 + H)
        assert [struct.unpack("!H", x[18:20])[0] for x in out] == [(0x4321 + i) & 0xFFFF for i in range(k)]
        if proto == "tcp":
            assert [struct.unpack("!I", x[38:42])[0] for x in out] == [0x1000 + i * mss for i in range(k)]
            assert [x[47] for x in out] == [0xDB & ~0x09] + [0xDB & ~0x89] * (k - 2) + [0xDB & ~0x80]
        else:
            assert [struct.unpack("!H", x[38:40])[0] for x in out] == [len(x) - 34 for x in out]
        if k <= 64:  # every segment; of the 65,535-B frames' thousands the ends and a stride
            picks = range(k)
        else:
            picks = sorted(set(range(0, k, max(1, k // 50))) | {0, 1, k - 2, k - 1})
        assert all(clean(out[i]) for i in picks), P
        pyseg.check_segments(f, out, mss)
        assert pyseg.classify(f, mss) == proto


def test_id_and_sequence_number_wrap():
    f = sf.tcp(100, 1, ident=0xFFFE, seq=0xFFFFFF00, flags=0x18)
    out = pyseg.segment(f, 30)
    assert [struct.unpack("!H", x[18:20])[0] for x in out] == [0xFFFE, 0xFFFF, 0, 1]
    assert [struct.unpack("!I", x[38:42])[0] for x in out] == [0xFFFFFF00, 0xFFFFFF1E, 0xFFFFFF3C, 0xFFFFFF5A]
    g = sf.tcp(400, 2, ident=0xFFFE, seq=0xFFFFFF00)
    out = pyseg.segment(g, 100)
    assert [struct.unpack("!I", x[38:42])[0] for x in out] == [0xFFFFFF00, 0xFFFFFF64, 0xFFFFFFC8, 0x2C]
    assert all(clean(x) for x in out)
    u = sf.udp(30, 3, ident=0xFFFE)
    assert [struct.unpack("!H", x[18:20])[0] for x in pyseg.segment(u, 8)] == [0xFFFE, 0xFFFF, 0, 1]
    assert [struct.unpack("!H", x[18:20])[0] for x in pyseg.segment(u, 8, pyseg.FIXED_ID)] == [0xFFFE] * 4


@pytest.mark.parametrize("H", [24, 60])
def test_tcp_options_are_copied_into_every_segment(H):
    f = sf.tcp(3000, H, H=H, flags=0x99)
    assert clean(f) and pyseg.l4_header_len(f) == H
    out = pyseg.segment(f, 1460)
    assert [len(x) for x in out] == [34 + H + 1460, 34 + H + 1460, 34 + H + 80]
    assert all(x[54:34 + H] == f[54:34 + H] and x[46] == f[46] for x in out)
    assert all(clean(x) for x in out)
    pyseg.check_segments(f, out, 1460)


def test_udp_checksum_of_zero_is_stored_as_ffff():
    """A payload whose first segment's computed checksum is 0x0000.  The search is pyseg's alone and
    fixed by its seed: a random payload, its first slice's last word then set to what the rest of
    the sum (pyseg.ones_sum) leaves open; a try counts when the stored field reads FF FF."""
    rng = np.random.default_rng(768)
    for tries in range(1, 4001):
        pay = bytearray(rng.integers(0, 256, 40, dtype=np.uint8).tobytes())
        pay[14:16] = b"\x00\x00"
        f = sf.udp(40, 0, pay=bytes(pay))
        rest = pyseg.ones_sum(pyseg.pseudo(f, 17, 24) + f[34:38] + struct.pack("!HH", 24, 0) + bytes(pay[:16]))
        pay[14:16] = struct.pack("!H", (0xFFFF - rest) % 0xFFFF)
        f = sf.udp(40, 0, pay=bytes(pay))
        out = pyseg.segment(f, 16)
        if out[0][40:42] == b"\xff\xff":
            break
    else:
        raise AssertionError("no payload found")
    x = bytearray(out[0])
    x[40:42] = b"\x00\x00"
    assert pyseg.csum(pyseg.pseudo(f, 17, 24) + bytes(x[34:])) == 0  # computed 0, so 0xFFFF is what is stored
    assert clean(out[0]) and pyseg.l4_ok(out[0])
    pyseg.check_segments(f, out, 16)


# ---- what is copied unchanged
def test_every_ineligible_class_is_copied_unchanged():
    for name, f in sf.ineligible(1700, 5).items():
        assert pyseg.l4_header_len(f) is None, name
        assert pyseg.segment(f, 536) == [f] and pyseg.segment(f, 536, 3) == [f], name
        assert pyseg.classify(f, 536) == "other" and pyseg.classify(f, 1658) == "fit", name
    # shorter than the headers: nothing to cut at any mss
    for L in (14, 20, 33):
        assert pyseg.segment(bytes(L), 8) == [bytes(L)] and pyseg.classify(bytes(L), 8) == "fit"
    # a TCP header that claims more bytes than the frame has
    f = bytearray(sf.tcp(39, 9))
    f[46] = 0xF0
    assert len(f) == 93 and pyseg.l4_header_len(bytes(f)) is None
    assert pyseg.segment(bytes(f), 8) == [bytes(f)] and pyseg.classify(bytes(f), 8) == "other"
    f[46] = 0xE0  # 56 B of header, 3 of payload: eligible, too short to cut at mss 8
    assert pyseg.l4_header_len(bytes(f)) == 56 and pyseg.classify(bytes(f), 8) == "fit"
    # eligible, but no more payload than one segment takes
    g = sf.tcp(1460, 1)
    assert pyseg.segment(g, 1460) == [g] and pyseg.classify(g, 1460) == "fit"
    assert pyseg.classify(sf.udp(1472, 1), 1472) == "fit" and pyseg.classify(sf.udp(1473, 1), 1472) == "udp"


def test_both_flags():
    f = sf.tcp(100, 7, ident=77, flags=0x18)
    base = pyseg.segment(f, 40)
    nocs = pyseg.segment(f, 40, pyseg.NO_L4_CSUM)
    fid = pyseg.segment(f, 40, pyseg.FIXED_ID)
    assert all(x[50:52] == f[50:52] for x in nocs)
    assert [x[:50] + x[52:] for x in nocs] == [x[:50] + x[52:] for x in base]
    assert [struct.unpack("!H", x[18:20])[0] for x in fid] == [77, 77, 77] and all(clean(x) for x in fid)
    both = pyseg.segment(f, 40, 3)
    assert [x[18:20] for x in both] == [f[18:20]] * 3 and all(x[50:52] == f[50:52] for x in both)
    for fl in (0, 1, 2, 3):
        pyseg.check_segments(f, pyseg.segment(f, 40, fl), 40, fl)
    u = sf.udp(100, 8)
    assert all(x[40:42] == u[40:42] for x in pyseg.segment(u, 40, pyseg.NO_L4_CSUM))
    with pytest.raises(ValueError):
        pyseg.segment(f, 7)
    with pytest.raises(ValueError):
        pyseg.segment(f, 40, 4)


def test_segment_all_counts():
    frames = [sf.udp(18, 1), sf.udp(3000, 2), sf.tcp(3000, 3), sf.ineligible(1700, 4)["icmp"], sf.tcp(1460, 5),
              sf.payload(14, 6)]
    out, cnt = pyseg.segment_all(frames, 1460)
    assert cnt == dict(n_in=6, n_out=10, n_split_tcp=1, n_split_udp=1, n_other=1,
                       out_bytes=sum(map(len, frames)) + 2 * 42 + 2 * 54, out_min_len=14, out_max_len=1700)
    pyseg.check_all(frames, out, 1460)
    bad = list(out)
    bad[2] = bad[2][:100] + bytes([bad[2][100] ^ 1]) + bad[2][101:]
    with pytest.raises(AssertionError):
        pyseg.check_all(frames, bad, 1460)


# ---- the ABI
def test_struct_sizes():
    lib = pbgpu.load_library()
    assert lib.pbgpu_abi_size(18) == C.sizeof(pbgpu.SegOpts) == 16
    assert lib.pbgpu_abi_size(19) == C.sizeof(pbgpu.SegResult) == 64
    assert (pbgpu.SEG_NO_L4_CSUM, pbgpu.SEG_FIXED_ID) == (1, 2)


def test_symbols_reject_null():
    lib = pbgpu.load_library()
    frames, dst, opts, res = pbgpu.Frames(), pbgpu.Frames(), pbgpu.SegOpts(1460, 0, 0), pbgpu.SegResult()
    a, b = C.c_uint64(), C.c_uint64()
    for fn in (lib.pbgpu_segment_size, lib.pbgpu_segment_bound):
        assert fn(None, C.byref(frames), 0, 0, C.byref(opts), C.byref(a), C.byref(b)) == -22
        assert fn(None, None, 0, 0, None, None, None) == -22
    assert lib.pbgpu_segment(None, C.byref(frames), 0, 0, C.byref(opts), C.byref(dst), C.byref(res)) == -22
    assert lib.pbgpu_segment(None, None, 0, 0, None, None, None) == -22


# ---- pcktbatch-gpu --segment: malformed values are refused before any GPU is opened
BASE = ["-z", "--interface", "pbnodev0", "--dip", "10.0.0.2", "--smac", "02:00:00:00:00:01", "--dmac",
        "02:00:00:00:00:02", "--protocol", "udp", "--pmin", "22", "--pmax", "22", "--seed", "7", "--delay", "0",
        "--maxpckts", "10"]
BAD_SPECS = ["bogus", "", "7", "65536", "-1", "1460x", "1460:", "1460:fixed", "1460:fixedid:1", "1460:fixedidx",
             ":fixedid", "0x5b4", "99999999999999999999", " 1460"]


@pytest.mark.parametrize("spec", BAD_SPECS)
def test_cli_refuses_malformed_values(tmp_path, spec):
    out = tmp_path / "out.pcap"
    r = subprocess.run([BIN] + BASE + ["--segment", spec, "--pcapdump", str(out)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0
    assert "--segment" in r.stderr and spec in r.stderr
    assert "GPU" not in r.stderr and not out.exists()


def test_cli_allows_one_segment(tmp_path):
    out = tmp_path / "out.pcap"
    r = subprocess.run([BIN] + BASE + ["--segment", "1460", "--segment", "536", "--pcapdump", str(out)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--segment" in r.stderr and not out.exists()


def test_help_lists_segment():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--segment MSS[:fixedid]" in r.stdout


# ---- the host driver with a builder that cannot segment
def test_stub_builder_refuses_segment(capfd):
    """tests/host_stub.c's table ends before the segmentation members: they are NULL, and seq_send
    refuses the sequence before it takes a slot or starts a thread; without --segment it runs."""
    os.makedirs(BUILD, exist_ok=True)
    stub_path = os.path.join(BUILD, "libpbhost_stub_seg.so")
    tmp = f"{stub_path}.{os.getpid()}"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread", "-o", tmp,
                    os.path.join(ROOT, "tests", "host_stub.c"), "-L" + LIBDIR, "-lpbhost", "-Wl,-rpath," + LIBDIR],
                   check=True)
    os.replace(tmp, stub_path)
    host = C.CDLL(os.path.join(LIBDIR, "libpbhost.so"))
    stub = C.CDLL(stub_path)
    host.seq_send.argtypes = [C.c_char_p, SequenceT, C.c_uint16, OurCmd]
    host.seq_send.restype = None
    host.pb_shutdown_stats.argtypes = [C.c_void_p]
    host.pb_sequence_totals.argtypes = [C.c_uint16, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    host.pb_set_segment.argtypes = [C.POINTER(pbgpu.SegOpts)]
    host.pb_get_segment.restype = C.POINTER(pbgpu.SegOpts)
    host.cmd_line_af_xdp_defaults.argtypes = [C.POINTER(OurCmd)]
    cfg = pc.c2_udp_64()
    cfg.update(maxpckts=64, delay=0)
    seq = Sequence.from_config(cfg)
    cmd = OurCmd()
    host.cmd_line_af_xdp_defaults(C.byref(cmd))

    def run():
        host.pb_reset()
        stub.stub_install()
        host.seq_send(b"lo", seq.c, 1, cmd)
        err = host.pb_shutdown_stats(None)
        p, b = C.c_uint64(), C.c_uint64()
        host.pb_sequence_totals(0, C.byref(p), C.byref(b))
        return err, p.value

    try:
        assert not host.pb_get_segment()
        opts = pbgpu.SegOpts(536, pbgpu.SEG_FIXED_ID, 0)
        host.pb_set_segment(C.byref(opts))
        got = host.pb_get_segment().contents
        assert (got.mss, got.flags) == (536, 2)
        err, pckts = run()
        assert (err, pckts) == (-95, 0)
        assert "--segment" in capfd.readouterr().err
        host.pb_set_segment(None)
        assert not host.pb_get_segment()
        assert run() == (0, 64)
    finally:
        host.pb_set_segment(None)
        host.pb_reset()
        stub.stub_uninstall()
