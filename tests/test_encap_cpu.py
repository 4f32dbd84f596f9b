"""Encapsulation without a GPU: the reference (tests/pyencap.py) against answers worked out by
hand, the ABI, and what pcktbatch-gpu --encap and the host driver refuse."""
import ctypes as C
import hashlib
import os
import subprocess

import pytest

import pb_configs as pc
import pbgpu
import pyencap
import pyverify
from cmdline_binding import OurCmd
from pbgpu import Sequence, SequenceT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pb-af-xdp_amd")
LIBDIR = os.path.join(PKG, "lib")
BIN = os.path.join(PKG, "bin", "pcktbatch-gpu")
BUILD = os.path.join(ROOT, "tests", "_build")

SRC60 = bytes(range(60))
KAT = dict(dst_mac=bytes.fromhex("020000000002"), src_mac=bytes.fromhex("020000000001"), src_ip=bytes([192, 0, 2, 1]),
           dst_ip=bytes([198, 51, 100, 2]), vni=0x123456)


def test_vxlan_known_answer():
    out = pyencap.vxlan(SRC60, **KAT)
    assert len(out) == 110
    assert out[:50].hex() == ("020000000002" "020000000001" "0800" "4500" "0060" "0000" "4000" "4011" "4e56" "c0000201"
                              "c6336402" "e0f9" "12b5" "004c" "0000" "08000000" "12345600")
    assert out[50:] == SRC60
    assert hashlib.sha256(out).hexdigest() == "92d465012369696a3f3146365a81f9cd2ea457c3b81c994924a105ab21acf3bb"


def test_hashed_source_port_known_answers():
    assert pyencap.sport(SRC60) == 0xE0F9
    assert pyencap.sport(bytes(range(30))) == 54354  # bytes 30..37 missing: they count as 0
    assert pyencap.sport(bytes(14)) == 49152
    assert all(49152 <= pyencap.sport(bytes([i]) * n) <= 65535 for i in (1, 77, 255) for n in (14, 27, 38, 64))


def test_vlan_known_answer():
    out = pyencap.vlan(SRC60, 0xA064)
    assert len(out) == 64 and out[:20].hex() == "000102030405060708090a0b" "8100a064" "0c0d0e0f"
    assert out[16:] == SRC60[12:]
    assert pyencap.vlan(SRC60, 5, 0x88A8)[12:16].hex() == "88a80005"
    assert pyencap.vlan(SRC60, 5, 0) == pyencap.vlan(SRC60, 5)


def test_fixed_fields_and_defaults():
    out = pyencap.vxlan(SRC60, **dict(KAT, src_port=4242, dst_port=8472, ttl=9, tos=0xB8))
    assert out[15] == 0xB8 and out[22] == 9 and out[34:38].hex() == "1092" "2118"
    assert pyencap.vxlan(SRC60, **KAT)[22] == 64


def test_vxlan_outer_header_verifies_for_every_length():
    """The outer IPv4 header's checksum and tot_len as the CPU checker reads them, 14..1500 B."""
    for L in range(14, 1501):
        out = pyencap.vxlan(bytes((i * 7 + L) & 0xFF for i in range(L)), **KAT)
        assert len(out) == L + 50
        assert pyverify.ip_csum_ok(out), L
        assert pyverify.parse(out)["tot_len"] == len(out) - 14, L
        assert out[38:40] == (L + 16).to_bytes(2, "big") and out[40:42] == b"\x00\x00"


# ---- the ABI
def test_opts_struct_size():
    lib = pbgpu.load_library()
    assert lib.pbgpu_abi_size(9) == C.sizeof(pbgpu.EncapOpts) == 44
    assert (pbgpu.ENCAP_VLAN, pbgpu.ENCAP_VXLAN) == (1, 2)
    o = pbgpu.EncapOpts.make(pbgpu.ENCAP_VXLAN, **KAT)
    assert (o.mode, o.vni, bytes(o.dst_mac), bytes(o.src_ip)) == (2, 0x123456, KAT["dst_mac"], KAT["src_ip"])
    with pytest.raises(TypeError):
        pbgpu.EncapOpts.make(pbgpu.ENCAP_VLAN, vid=5)


def test_symbols_reject_null():
    lib = pbgpu.load_library()
    frames, dst, opts = pbgpu.Frames(), pbgpu.Frames(), pbgpu.EncapOpts.make(pbgpu.ENCAP_VLAN, tci=1)
    a, b, ms = C.c_uint64(), C.c_uint64(), C.c_double()
    assert lib.pbgpu_encap_size(None, C.byref(frames), 0, 0, C.byref(opts), C.byref(a), C.byref(b)) == -22
    assert lib.pbgpu_encap(None, C.byref(frames), 0, 0, C.byref(opts), C.byref(dst), C.byref(ms)) == -22
    assert lib.pbgpu_encap(None, None, 0, 0, None, None, None) == -22
    assert lib.pbgpu_encap_size(None, None, 0, 0, None, None, None) == -22


# ---- pcktbatch-gpu --encap: malformed specs are refused before any GPU is opened
BASE = ["-z", "--interface", "pbnodev0", "--dip", "10.0.0.2", "--smac", "02:00:00:00:00:01", "--dmac",
        "02:00:00:00:00:02", "--protocol", "udp", "--pmin", "22", "--pmax", "22", "--seed", "7", "--delay", "0",
        "--maxpckts", "10"]
BAD_SPECS = ["bogus", "vlan", "vlan:", "vlan:4096", "vlan:-1", "vlan:1x", "vlan:100:8", "vlan:100:5:1",
             "vxlan:16777216:192.0.2.1:198.51.100.2", "vxlan:5000", "vxlan:5000:192.0.2.1", "vxlan:5000:192.0.2:198.51.100.2",
             "vxlan:5000:192.0.2.1:nowhere", "vxlan:5000::198.51.100.2", "vxlan:5000:192.0.2.1:198.51.100.2:0",
             "vxlan:5000:192.0.2.1:198.51.100.2:65536", "vxlan:x:192.0.2.1:198.51.100.2"]


@pytest.mark.parametrize("spec", BAD_SPECS)
def test_cli_refuses_malformed_specs(tmp_path, spec):
    out = tmp_path / "out.pcap"
    r = subprocess.run([BIN] + BASE + ["--encap", spec, "--pcapdump", str(out)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0
    assert "--encap" in r.stderr and spec in r.stderr
    assert "GPU" not in r.stderr and not out.exists()


def test_cli_allows_one_encap(tmp_path):
    out = tmp_path / "out.pcap"
    r = subprocess.run([BIN] + BASE + ["--encap", "vlan:1", "--encap", "vlan:2", "--pcapdump", str(out)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--encap" in r.stderr and not out.exists()


def test_help_lists_encap():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--encap vlan:VID[:PCP]" in r.stdout and "vxlan:VNI:SRCIP:DSTIP[:DPORT]" in r.stdout


# ---- the host driver with a builder that cannot encapsulate
def test_stub_builder_refuses_encap(capfd):
    """tests/host_stub.c's table ends before the encapsulation members: they are NULL, and seq_send
    refuses the sequence before it takes a slot or starts a thread; without --encap it runs."""
    os.makedirs(BUILD, exist_ok=True)
    stub_path = os.path.join(BUILD, "libpbhost_stub_encap.so")
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
    host.pb_set_encap.argtypes = [C.POINTER(pbgpu.EncapOpts)]
    host.pb_get_encap.restype = C.POINTER(pbgpu.EncapOpts)
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
        assert not host.pb_get_encap()
        opts = pbgpu.EncapOpts.make(pbgpu.ENCAP_VLAN, tci=100)
        host.pb_set_encap(C.byref(opts))
        assert host.pb_get_encap().contents.tci == 100
        err, pckts = run()
        assert (err, pckts) == (-95, 0)
        assert "--encap" in capfd.readouterr().err
        host.pb_set_encap(None)
        assert not host.pb_get_encap()
        assert run() == (0, 64)
    finally:
        host.pb_set_encap(None)
        host.pb_reset()
        stub.stub_uninstall()
