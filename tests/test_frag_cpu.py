"""IPv4 fragmentation without a GPU: the reference (tests/pyfrag.py) against answers worked out by
hand and against its own properties, the ABI, and what pcktbatch-gpu --fragment and the host driver
refuse."""
import ctypes as C
import hashlib
import os
import struct
import subprocess

import pytest

import pb_configs as pc
import pbgpu
import pyfrag
import pyverify
from cmdline_binding import OurCmd
from pbgpu import Sequence, SequenceT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pb-af-xdp_amd")
LIBDIR = os.path.join(PKG, "lib")
BIN = os.path.join(PKG, "bin", "pcktbatch-gpu")
BUILD = os.path.join(ROOT, "tests", "_build")

ETH = "020000000002" "020000000001" "0800"


def mk_frame(L: int, fo: int = 0, ethertype: bytes = b"\x08\x00", vihl: int = 0x45) -> bytes:
    """An L-byte frame with a consistent IPv4 header (tot_len, checksum) and patterned data."""
    f = bytearray((i * 7 + L) & 0xFF for i in range(L))
    f[0:12] = bytes.fromhex(ETH[:24])
    if L >= 14:
        f[12:14] = ethertype
    if L >= 34:
        f[14:34] = struct.pack("!BBHHHBBH", vihl, 0, L - 14, 0x1234, fo, 64, 17, 0) + bytes([192, 0, 2, 1, 198, 51, 100, 2])
        f[24:26] = struct.pack("!H", pyverify.ip_csum_value(bytes(f)))
    return bytes(f)


# ---- hand-worked answers
def test_short_frame_at_mtu_68_byte_by_byte():
    """84 B: 50 data bytes behind the headers, tot_len 70 > 68.  C = 48: fragments of 48 and 2 data bytes,
    tot_len 68 and 22, fragment fields 0x2000 (MF, offset 0) and 0x0006 (offset 48 / 8)."""
    data = bytes(range(100, 150))
    src = bytes.fromhex(ETH + "4500" "0046" "1234" "0000" "4011" "7c3c" "c0000201" "c6336402") + data
    assert pyverify.ip_csum_ok(src) and len(src) == 84
    f0 = bytes.fromhex(ETH + "4500" "0044" "1234" "2000" "4011" "5c3e" "c0000201" "c6336402") + data[:48]
    f1 = bytes.fromhex(ETH + "4500" "0016" "1234" "0006" "4011" "7c66" "c0000201" "c6336402") + data[48:]
    assert pyfrag.fragment(src, 68) == [f0, f1]
    assert pyfrag.fragment(src, 69) == [f0, f1]  # C stays 48
    assert pyfrag.fragment(src, 70) == [src] and pyfrag.fragment(src, 75) == [src]
    assert pyfrag.reassemble([f1, f0]) == src


def test_9043_byte_example():
    f = bytearray((i * 7 + 3) & 0xFF for i in range(9043))
    f[12:14], f[14], f[20:22] = b"\x08\x00", 0x45, b"\x00\x00"
    out = pyfrag.fragment(bytes(f), 1500)
    assert [len(x) for x in out] == [1514] * 6 + [163] and sum(len(x) for x in out) == 9247
    assert hashlib.sha256(b"".join(out)).hexdigest() == "c949ae62aefc61c22d413ecfd02209d736e0561ae73552c869aa9a8e12a65685"
    assert b"".join(x[34:] for x in out) == bytes(f[34:])
    assert [struct.unpack("!H", x[20:22])[0] for x in out] == [0x2000 + 185 * i for i in range(6)] + [185 * 6]
    assert len(pyfrag.fragment(mk_frame(65535), 68)) == 1365


# ---- properties
MTUS = (68, 69, 75, 76, 576, 1500, 9000)


def _lengths(mtu):
    c = (mtu - 20) & ~7
    return sorted({34, 35, mtu + 13, mtu + 14, mtu + 15, mtu + 22, 34 + 3 * c, 34 + 3 * c + 1, 65535})


@pytest.mark.parametrize("mtu", MTUS)
def test_properties(mtu):
    c = (mtu - 20) & ~7
    for L in _lengths(mtu):
        f = mk_frame(L)
        out = pyfrag.fragment(f, mtu)
        k = 1 if L - 14 <= mtu else -(-(L - 34) // c)
        assert len(out) == k, L
        assert all(len(x) - 14 <= mtu for x in out), L
        assert all(pyverify.ip_csum_ok(x) and struct.unpack("!H", x[16:18])[0] == len(x) - 14 for x in out), L
        assert pyfrag.reassemble(out) == f, L
        assert sum(len(x) for x in out) == L + 34 * (k - 1), L
        assert all((len(x) - 34) % 8 == 0 for x in out[:-1]), L


# ---- pass-through and fragments of fragments
def test_df_and_ignore_df():
    f = mk_frame(1600, fo=0x4000)
    assert pyfrag.fragment(f, 1500) == [f] and pyfrag.classify(f, 1500) == "df"
    out = pyfrag.fragment(f, 1500, ignore_df=True)
    assert [len(x) for x in out] == [1514, 120]
    assert [struct.unpack("!H", x[20:22])[0] for x in out] == [0x6000, 0x4000 + 185]
    assert pyfrag.reassemble(out) == f
    assert pyfrag.fragment(mk_frame(1514, fo=0x4000), 1500) == [mk_frame(1514, fo=0x4000)]
    assert pyfrag.classify(mk_frame(1514, fo=0x4000), 1500) == "fit"


def test_not_ipv4_without_options_is_copied():
    for f in (mk_frame(1600, ethertype=b"\x86\xdd"), mk_frame(1600, vihl=0x46), mk_frame(1600, vihl=0x65)):
        assert pyfrag.fragment(f, 576) == [f] and pyfrag.fragment(f, 576, True) == [f]
        assert pyfrag.classify(f, 576) == "other"
    assert pyfrag.fragment(bytes(20), 68) == [bytes(20)] and pyfrag.classify(bytes(20), 68) == "fit"


def test_source_that_is_a_middle_fragment():
    """MF set, offset 100 (800 B): every piece keeps MF, the offsets go on from 100."""
    f = mk_frame(34 + 1000, fo=0x2000 | 100)
    out = pyfrag.fragment(f, 576)
    assert [len(x) - 34 for x in out] == [552, 448]
    assert [struct.unpack("!H", x[20:22])[0] for x in out] == [0x2000 | 100, 0x2000 | (100 + 69)]
    assert b"".join(x[34:] for x in out) == f[34:] and all(pyverify.ip_csum_ok(x) for x in out)
    last = pyfrag.fragment(mk_frame(34 + 1000, fo=8150), 576)  # a last fragment: the offset wraps mod 2^13
    assert [struct.unpack("!H", x[20:22])[0] for x in last] == [0x2000 | 8150, 27]


def test_fragment_all_counts():
    frames = [mk_frame(60), mk_frame(1600), mk_frame(1600, fo=0x4000), mk_frame(1600, vihl=0x46), mk_frame(3000)]
    out, cnt = pyfrag.fragment_all(frames, 1500)
    assert cnt == dict(n_in=5, n_out=8, n_split=2, n_df=1, n_other=1, out_bytes=sum(map(len, frames)) + 34 * 3,
                       out_min_len=40, out_max_len=1600)  # 3000 B: 1514 + 1514 + 40
    assert len(out) == 8


# ---- the ABI
def test_struct_sizes():
    lib = pbgpu.load_library()
    assert lib.pbgpu_abi_size(10) == C.sizeof(pbgpu.FragOpts) == 16
    assert lib.pbgpu_abi_size(11) == C.sizeof(pbgpu.FragResult) == 64
    assert pbgpu.FRAG_IGNORE_DF == 1


def test_symbols_reject_null():
    lib = pbgpu.load_library()
    frames, dst, opts, res = pbgpu.Frames(), pbgpu.Frames(), pbgpu.FragOpts(1500, 0, 0), pbgpu.FragResult()
    a, b = C.c_uint64(), C.c_uint64()
    for fn in (lib.pbgpu_fragment_size, lib.pbgpu_fragment_bound):
        assert fn(None, C.byref(frames), 0, 0, C.byref(opts), C.byref(a), C.byref(b)) == -22
        assert fn(None, None, 0, 0, None, None, None) == -22
    assert lib.pbgpu_fragment(None, C.byref(frames), 0, 0, C.byref(opts), C.byref(dst), C.byref(res)) == -22
    assert lib.pbgpu_fragment(None, None, 0, 0, None, None, None) == -22


# ---- pcktbatch-gpu --fragment: malformed values are refused before any GPU is opened
BASE = ["-z", "--interface", "pbnodev0", "--dip", "10.0.0.2", "--smac", "02:00:00:00:00:01", "--dmac",
        "02:00:00:00:00:02", "--protocol", "udp", "--pmin", "22", "--pmax", "22", "--seed", "7", "--delay", "0",
        "--maxpckts", "10"]
BAD_SPECS = ["bogus", "", "67", "65536", "-1", "1500x", "1500:", "1500:df", "1500:ignoredf:1", "1500:ignoredfx",
             ":ignoredf", "0x5dc", "99999999999999999999", " 1500"]


@pytest.mark.parametrize("spec", BAD_SPECS)
def test_cli_refuses_malformed_values(tmp_path, spec):
    out = tmp_path / "out.pcap"
    r = subprocess.run([BIN] + BASE + ["--fragment", spec, "--pcapdump", str(out)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0
    assert "--fragment" in r.stderr and spec in r.stderr
    assert "GPU" not in r.stderr and not out.exists()


def test_cli_allows_one_fragment(tmp_path):
    out = tmp_path / "out.pcap"
    r = subprocess.run([BIN] + BASE + ["--fragment", "1500", "--fragment", "576", "--pcapdump", str(out)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--fragment" in r.stderr and not out.exists()


def test_help_lists_fragment():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--fragment MTU[:ignoredf]" in r.stdout


# ---- the host driver with a builder that cannot fragment
def test_stub_builder_refuses_fragment(capfd):
    """tests/host_stub.c's table ends before the fragmentation members: they are NULL, and seq_send
    refuses the sequence before it takes a slot or starts a thread; without --fragment it runs."""
    os.makedirs(BUILD, exist_ok=True)
    stub_path = os.path.join(BUILD, "libpbhost_stub_frag.so")
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
    host.pb_set_fragment.argtypes = [C.POINTER(pbgpu.FragOpts)]
    host.pb_get_fragment.restype = C.POINTER(pbgpu.FragOpts)
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
        assert not host.pb_get_fragment()
        opts = pbgpu.FragOpts(576, pbgpu.FRAG_IGNORE_DF, 0)
        host.pb_set_fragment(C.byref(opts))
        got = host.pb_get_fragment().contents
        assert (got.mtu, got.flags) == (576, 1)
        err, pckts = run()
        assert (err, pckts) == (-95, 0)
        assert "--fragment" in capfd.readouterr().err
        host.pb_set_fragment(None)
        assert not host.pb_get_fragment()
        assert run() == (0, 64)
    finally:
        host.pb_set_fragment(None)
        host.pb_reset()
        stub.stub_uninstall()
