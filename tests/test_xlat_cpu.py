"""IPv4-to-IPv6 translation without a GPU: the reference (tests/pyxlat.py) on the oracle's frames
through its own from-scratch checker, answers written out in hex, the checksum corners, the ABI,
and what pcktbatch-gpu --xlat6 and the host driver parse and refuse."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import pb_configs as pc
import pbgpu
import pyxlat
from cmdline_binding import OurCmd
from pbgpu import Sequence, SequenceT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pb-af-xdp_amd")
LIBDIR = os.path.join(PKG, "lib")
BIN = os.path.join(PKG, "bin", "pcktbatch-gpu")
BUILD = os.path.join(ROOT, "tests", "_build")

CARRY, ZERO, NEUTRAL = "2001:db8:ffff:ffff:ffff:ffff::/96", "::/96", "64:ff9b::/96"


# ---- the reference against the from-scratch checker, on the oracle's frames
@pytest.fixture(scope="module")
def built():
    """A few hundred iterations of the four configurations, built once."""
    return {name: ob.frames(Sequence.from_config(pc.get(name)), 0, 100, 300, pc.SEED_BASE)
            for name in ("c2_udp_64", "c3_udp_var", "c4_tcp_syn", "c5_icmp_echo")}


@pytest.mark.parametrize("prefix", [CARRY, ZERO, NEUTRAL])
@pytest.mark.parametrize("cfg", ["c2_udp_64", "c3_udp_var", "c4_tcp_syn", "c5_icmp_echo"])
def test_translated_oracle_frames_check_good_from_scratch(built, cfg, prefix):
    p = pyxlat.prefix96(prefix)
    frames = built[cfg]
    assert len(frames) == 300
    for hash_flow in (False, True):
        out = pyxlat.xlat_all(frames, p, flow_label=0x54321, hash_flow=hash_flow)
        for f, g in zip(frames, out):
            assert len(g) == len(f) + 20 and pyxlat.check6(g)
            assert g[:12] == f[:12] and g[21] == f[22] and g[34:38] == f[26:30] and g[50:54] == f[30:34]
            fl = (g[15] & 15) << 16 | g[16] << 8 | g[17]
            assert fl == (pyxlat.flow_hash(f) if hash_flow else 0x54321)
    if cfg == "c3_udp_var":
        assert len({len(f) for f in frames}) > 100


@pytest.mark.parametrize("cfg,at", [("c2_udp_64", 40), ("c3_udp_var", 40), ("c4_tcp_syn", 50)])
def test_neutral_prefix_leaves_the_checksum(built, cfg, at):
    """64:ff9b::/96 sums to 0xFFFF, the ones' complement zero: the stored checksum stays, but for
    0xFFFF itself, which comes out in its other spelling."""
    p = pyxlat.prefix96(NEUTRAL)
    assert pyxlat.fold(pyxlat.words(p)) == 0xFFFF
    seen = 0
    for f in built[cfg]:
        g = pyxlat.xlat46(f, p)
        if f[at:at + 2] != b"\xff\xff":
            assert g[at + 20:at + 22] == f[at:at + 2]
            seen += 1
    assert seen > 290


# ---- answers written out; their checksums come from the from-scratch half
P_SRC, P_DST = pyxlat.prefix96(CARRY), pyxlat.prefix96(NEUTRAL)
KAT = {
    "udp": ("020000000002020000000001080045b80027123440003f113c7ec0000221c63364071234003500135ba34142434445464748494a4b",
            "02000000000202000000000186dd6b8123450013113f20010db8ffffffffffffffffc00002210064ff9b0000000000000000c6336407"
            "1234003500132dea4142434445464748494a4b"),
    "tcp": ("020000000002020000000001080045b8002e123440003f063c82c0000221c63364079c4001bb010203040000000050022000bd8b0000"
            "68656c6c6f21",
            "02000000000202000000000186dd6b812345001a063f20010db8ffffffffffffffffc00002210064ff9b0000000000000000c6336407"
            "9c4001bb0102030400000000500220008fd2000068656c6c6f21"),
    "icmp": ("020000000002020000000001080045b8002d123440003f013c88c0000221c633640708006c18beef000770696e672d7061796c6f6164"
             "2d30313233",
             "02000000000202000000000186dd6b81234500193a3f20010db8ffffffffffffffffc00002210064ff9b0000000000000000c6336407"
             "8000d9aebeef000770696e672d7061796c6f61642d30313233"),
}


@pytest.mark.parametrize("kind", list(KAT))
def test_known_answer(kind):
    f, g = (bytes.fromhex(h) for h in KAT[kind])
    assert pyxlat.classify(f) == kind
    assert pyxlat.set_csum6(g) == g and pyxlat.check6(g)  # the written answer's checksum is the from-scratch one
    assert pyxlat.xlat46(f, P_SRC, P_DST, flow_label=0x12345) == g
    # traffic class 0xB8 and the label share bytes 14..17; the hop limit is the TTL
    assert g[14:18].hex() == "6b812345" and g[21] == 63
    if kind == "icmp":
        reply = bytearray(f)
        reply[34] = 0
        reply[36:38] = ((int.from_bytes(f[36:38], "big") + 0x0800) % 0xFFFF).to_bytes(2, "big")  # type 8 -> 0
        r6 = pyxlat.xlat46(bytes(reply), P_SRC, P_DST)
        assert r6[54] == 129 and pyxlat.check6(r6)


def test_classes():
    f = bytes.fromhex(KAT["udp"][0])

    def mut(at, val, base=f):
        b = bytearray(base)
        b[at:at + len(val)] = val
        return bytes(b)

    assert pyxlat.classify(f[:42]) == "udp" and pyxlat.classify(f[:41]) == pyxlat.OTHER
    for bad in (f[:33], mut(12, b"\x08\x06"), mut(14, b"\x46"), mut(20, b"\x20\x00"), mut(20, b"\x00\x01"),
                mut(23, b"\x2f"), mut(23, b"\x06")):
        assert pyxlat.classify(bad) == pyxlat.OTHER and pyxlat.xlat46(bad, P_SRC) is None
    assert pyxlat.classify(mut(20, b"\xc0\x00")) == "udp"  # DF and the reserved bit are no fragment
    t = bytes.fromhex(KAT["tcp"][0])
    assert pyxlat.classify(t[:54]) == "tcp" and pyxlat.classify(t[:53]) == pyxlat.OTHER
    i = bytes.fromhex(KAT["icmp"][0])
    assert pyxlat.classify(mut(34, b"\x03", i)) == pyxlat.OTHER and pyxlat.classify(mut(34, b"\x00", i)) == "icmp"
    assert pyxlat.classify(i[:42]) == "icmp" and pyxlat.classify(i[:41]) == pyxlat.OTHER


def test_udp_zero_becomes_ffff_and_tcp_keeps_zero():
    """A frame whose stored checksum makes the translated one 0x0000: UDP leaves with 0xFFFF (RFC 8200
    8.1) and still checks good from scratch; TCP with the same arithmetic keeps 0x0000 and checks good."""
    p = pyxlat.prefix96(CARRY)
    K = pyxlat.fold(2 * pyxlat.words(p))
    rng = np.random.default_rng(3)
    for kind, L, at, pay in (("udp", 64, 40, 62), ("tcp", 60, 50, 58)):
        f = bytearray(pyxlat.frame4(kind, L, rng))
        c = int.from_bytes(f[at:at + 2], "big")
        w = int.from_bytes(f[pay:pay + 2], "big")
        # the stored checksum becomes K, a payload word moves with it: the segment still sums to 0xFFFF
        f[at:at + 2] = K.to_bytes(2, "big")
        f[pay:pay + 2] = ((w + c - K) % 0xFFFF).to_bytes(2, "big")
        g = pyxlat.xlat46(bytes(f), p)
        assert g[at + 20:at + 22] == (b"\xff\xff" if kind == "udp" else b"\x00\x00")
        assert pyxlat.segment_sum(g) == 0xFFFF
        assert pyxlat.check6(g)
    # a stored 0 gets no special case: a UDP frame built without a checksum leaves with a wrong one
    f = pyxlat.frame4("udp", 64, rng, l4_csum=0)
    g = pyxlat.xlat46(f, p)
    assert g[60:62] == (~K & 0xFFFF or 0xFFFF).to_bytes(2, "big") and not pyxlat.check6(g)


# ---- the ABI
def test_struct_sizes():
    lib = pbgpu.load_library()
    assert lib.pbgpu_abi_size(14) == C.sizeof(pbgpu.XlatOpts) == 40
    assert lib.pbgpu_abi_size(15) == C.sizeof(pbgpu.XlatResult) == 56
    assert pbgpu.XLAT_HASH_FLOW == 1
    o = pbgpu.XlatOpts.make(P_SRC, flow_label=7, hash_flow=True)
    assert (bytes(o.src_prefix), bytes(o.dst_prefix), o.flow_label, o.flags, o.reserved) == (P_SRC, P_SRC, 7, 1, 0)
    assert bytes(pbgpu.XlatOpts.make(P_SRC, P_DST).dst_prefix) == P_DST
    with pytest.raises(ValueError):
        pbgpu.XlatOpts.make(bytes(16))


def test_symbols_reject_null():
    lib = pbgpu.load_library()
    frames, dst, opts = pbgpu.Frames(), pbgpu.Frames(), pbgpu.XlatOpts.make(P_SRC)
    a, b, res = C.c_uint64(), C.c_uint64(), pbgpu.XlatResult()
    assert lib.pbgpu_xlat46_size(None, C.byref(frames), 0, 0, C.byref(opts), C.byref(a), C.byref(b)) == -22
    assert lib.pbgpu_xlat46(None, C.byref(frames), 0, 0, C.byref(opts), C.byref(dst), C.byref(res)) == -22
    assert lib.pbgpu_xlat46(None, None, 0, 0, None, None, None) == -22
    assert lib.pbgpu_xlat46_size(None, None, 0, 0, None, None, None) == -22


# ---- pcktbatch-gpu --xlat6: parsed and refused before any GPU is opened
BASE = ["-z", "--interface", "pbnodev0", "--dip", "10.0.0.2", "--smac", "02:00:00:00:00:01", "--dmac",
        "02:00:00:00:00:02", "--protocol", "udp", "--pmin", "22", "--pmax", "22", "--seed", "7", "--delay", "0",
        "--maxpckts", "10"]
BAD_SPECS = ["bogus", "64:ff9b::", "64:ff9b::/64", "64:ff9b::/128", "64:ff9b::/96x", "64:ff9b::1:0/96",
             "64:ff9b::0.0.0.1/96", "10.0.0.0/96", "64:ff9b::/96,", "64:ff9b::/96,2001:db8::/64", "64:ff9b::/96,nowhere/96",
             "64:ff9b::/96:", "64:ff9b::/96:hash", "64:ff9b::/96:hashflow:x", "64:ff9b::/96:hashflow,2001:db8::/96",
             "64:ff9b::/96,2001:db8::/96,::/96", ":hashflow", "/96"]


@pytest.mark.parametrize("spec", BAD_SPECS)
def test_cli_refuses_malformed_specs(tmp_path, spec):
    out = tmp_path / "out.pcap"
    r = subprocess.run([BIN] + BASE + ["--xlat6", spec, "--pcapdump", str(out)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0
    assert "--xlat6" in r.stderr and spec in r.stderr
    assert "GPU" not in r.stderr and not out.exists()


@pytest.mark.parametrize("spec,line", [
    ("64:ff9b::/96", "XLAT6: src=64:ff9b::/96 dst=64:ff9b::/96 hashflow=0"),
    ("2001:db8:ffff:ffff:ffff:ffff::/96,64:ff9b::/96",
     "XLAT6: src=2001:db8:ffff:ffff:ffff:ffff::/96 dst=64:ff9b::/96 hashflow=0"),
    ("::/96:hashflow", "XLAT6: src=::/96 dst=::/96 hashflow=1"),
    ("2001:DB8:0:0:1::/96,::/96:hashflow", "XLAT6: src=2001:db8:0:0:1::/96 dst=::/96 hashflow=1"),
])
def test_cli_parses_prefixes(spec, line):
    r = subprocess.run([BIN] + BASE + ["--xlat6", spec, "-l"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert line in r.stdout.splitlines()
    plain = subprocess.run([BIN] + BASE + ["-l"], capture_output=True, text=True, timeout=60)
    assert "XLAT6" not in plain.stdout
    assert [x for x in r.stdout.splitlines() if not x.startswith("XLAT6")] == plain.stdout.splitlines()


def _refused(tmp_path, extra, dumping=True):
    out = tmp_path / "out.pcap"
    r = subprocess.run([BIN] + BASE + ["--xlat6", "64:ff9b::/96"] + extra + (["--pcapdump", str(out)] if dumping else []),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--xlat6" in r.stderr and "GPU" not in r.stderr and not out.exists()
    return r.stderr


def test_cli_allows_one_xlat6(tmp_path):
    assert "more than once" in _refused(tmp_path, ["--xlat6", "::/96"])


@pytest.mark.parametrize("dumping", [True, False])
def test_cli_refuses_fragment_beside_xlat6(tmp_path, dumping):
    assert "--fragment" in _refused(tmp_path, ["--fragment", "576"], dumping)


@pytest.mark.parametrize("dumping", [True, False])
def test_cli_refuses_udp_without_l4_checksum(tmp_path, dumping):
    assert "l4csum" in _refused(tmp_path, ["--l4csum", "0"], dumping)


def test_help_lists_xlat6():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--xlat6 SRC6/96[,DST6/96][:hashflow]" in r.stdout


# ---- the host driver with a builder that cannot translate
def test_stub_builder_refuses_xlat6(capfd):
    """tests/host_stub.c's table ends before the translation members: they are NULL, and seq_send
    refuses the sequence before it takes a slot or starts a thread; without --xlat6 it runs."""
    os.makedirs(BUILD, exist_ok=True)
    stub_path = os.path.join(BUILD, "libpbhost_stub_xlat.so")
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
    host.pb_set_xlat.argtypes = [C.POINTER(pbgpu.XlatOpts)]
    host.pb_get_xlat.restype = C.POINTER(pbgpu.XlatOpts)
    host.cmd_line_af_xdp_defaults.argtypes = [C.POINTER(OurCmd)]
    cfg = pc.c2_udp_64()
    cfg.update(maxpckts=64, delay=0)
    seq = Sequence.from_config(cfg)
    nocsum = dict(cfg, l4csum=0)
    seq0 = Sequence.from_config(nocsum)
    cmd = OurCmd()
    host.cmd_line_af_xdp_defaults(C.byref(cmd))

    def run(s=seq):
        host.pb_reset()
        stub.stub_install()
        host.seq_send(b"lo", s.c, 1, cmd)
        err = host.pb_shutdown_stats(None)
        p, b = C.c_uint64(), C.c_uint64()
        host.pb_sequence_totals(0, C.byref(p), C.byref(b))
        return err, p.value

    try:
        assert not host.pb_get_xlat()
        opts = pbgpu.XlatOpts.make(P_SRC, P_DST, hash_flow=True)
        host.pb_set_xlat(C.byref(opts))
        got = host.pb_get_xlat().contents
        assert (bytes(got.src_prefix), bytes(got.dst_prefix), got.flags) == (P_SRC, P_DST, 1)
        err, pckts = run()
        assert (err, pckts) == (-95, 0)
        assert "--xlat6" in capfd.readouterr().err
        # a UDP sequence without its L4 checksum is refused whatever the builder can do
        err, pckts = run(seq0)
        assert (err, pckts) == (-22, 0)
        assert "l4csum" in capfd.readouterr().err
        host.pb_set_xlat(None)
        assert not host.pb_get_xlat()
        assert run() == (0, 64)
        assert run(seq0) == (0, 64)
    finally:
        host.pb_set_xlat(None)
        host.pb_reset()
        stub.stub_uninstall()
