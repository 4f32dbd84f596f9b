"""pbgpu_verify_wire without a GPU: the definition's restatement (tests/pywire.py) against the other
pure-Python references on the oracle's frames - pyverify on plain frames and their byte mutants,
pyencap, pyxlat's from-scratch checker, pyfrag - answers written out in hex, every MALFORMED rule at
its boundary, the ABI, and what pcktbatch-gpu --verifywire and the host driver parse and refuse."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import pb_configs as pc
import pbgpu
import pyencap
import pyfrag
import pyverify
import pywire as pw
import pyxlat
import wire_frames as wf
from cmdline_binding import OurCmd
from pbgpu import Sequence, SequenceT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pb-af-xdp_amd")
LIBDIR = os.path.join(PKG, "lib")
BIN = os.path.join(PKG, "bin", "pcktbatch-gpu")
BUILD = os.path.join(ROOT, "tests", "_build")
CONFIGS = ("c2_udp_64", "c3_udp_var", "c4_tcp_syn", "c5_icmp_echo")
PORT = 4789
VX = dict(dst_mac=bytes.fromhex("0200000000a2"), src_mac=bytes.fromhex("0200000000a1"), src_ip=bytes([192, 0, 2, 1]),
          dst_ip=bytes([198, 51, 100, 2]), vni=0x123456)


@pytest.fixture(scope="module")
def built():
    """300 iterations of the four configurations from the oracle, built once."""
    return {name: ob.frames(Sequence.from_config(pc.get(name)), 0, 100, 300, pc.SEED_BASE) for name in CONFIGS}


def mutants(frames, step=7):
    """One single-byte mutant per frame, the position moving through the frame with the frame's index."""
    out = []
    for k, f in enumerate(frames):
        m = bytearray(f)
        p = (k * step) % len(f)
        m[p] ^= 1 << (k % 8)
        out.append((p, bytes(m)))
    return out


# ---- the oracle's frames
@pytest.mark.parametrize("cfg", CONFIGS)
def test_oracle_frames_are_clean(built, cfg):
    frames = built[cfg]
    assert len(frames) == 300
    codes, r = pw.result(frames)
    assert set(codes) <= {0, pw.NOL4} and r["n_bad"] == 0 and r["n_ipv4"] == 300 and r["first_bad"] == 2**64 - 1
    assert r["n_nol4"] == sum(f[23] == 17 and f[40:42] == b"\0\0" for f in frames) < 3


def _pyverify_code(f):
    """pyverify's verdict in pbgpu_verify's bits: IPv4 checksum 1, tot_len 2, L4 sum 4."""
    d = pyverify.parse(f)
    code = 0 if pyverify.ip_csum_ok(f) else 1
    if d["tot_len"] != len(f) - 14:
        code |= 2
    l4 = d["l4"]
    pseudo = d["saddr"] + d["daddr"] + struct.pack("!BBH", 0, d["proto"], len(l4)) if d["proto"] in (6, 17) else b""
    if pyverify.ones_sum(pseudo + l4) != 0xFFFF:
        code |= 4
    return code


STRUCTURE = {12, 13, 14, 20, 21, 23}  # ethertype, version / IHL, the fragment field, the protocol: what decides the walk


@pytest.mark.parametrize("cfg", CONFIGS)
def test_equal_to_pyverify_on_plain_frames_and_mutants(built, cfg):
    """IP_CSUM -> L3_CSUM, TOT_LEN -> L3_LEN, L4 -> L4, bit for bit; only frames whose stored UDP checksum
    is 00 00 are left out (there it means "none"), and the mutants of the bytes that decide which headers
    are walked, which pyverify takes for granted."""
    frames = built[cfg]
    cases = [(None, f) for f in frames] + mutants(frames) + mutants(frames, 13)
    seen = left_out = 0
    for p, f in cases:
        if p in STRUCTURE:
            continue
        if f[23] == 17 and f[40:42] == b"\0\0":
            left_out += 1
            continue
        assert pw.code(f) & 7 == _pyverify_code(f), (p, f.hex())
        seen += 1
    assert left_out < len(cases) // 100 and seen > 800


@pytest.mark.parametrize("cfg", CONFIGS)
def test_through_the_repacks(built, cfg):
    frames = built[cfg]
    plain, _ = pw.result(frames)
    # VLAN, one tag and two
    for tagged in ([pyencap.vlan(f, 0x2064) for f in frames],
                   [pyencap.vlan(pyencap.vlan(f, 100), 0x0123, 0x88A8) for f in frames]):
        codes, r = pw.result(tagged)
        assert codes == plain and r["n_bad"] == 0
    # VXLAN: the inner frame is found behind the port only
    vx = [pyencap.vxlan(f, **VX) for f in frames]
    codes, r = pw.result(vx, vxlan_port=PORT)
    assert codes == [c | pw.INNER for c in plain] and r["n_inner"] == 300 and r["n_bad"] == 0
    codes, r = pw.result(vx)
    assert set(codes) == {pw.NOL4} and r["n_inner"] == 0  # the outer UDP checksum is 00 00
    for k, (p, m) in enumerate(mutants(vx, 11)):
        inner = pw.code(m[50:])
        want_bad = (p >= 50 and inner & pw.BAD) or 14 <= p < 34 or p in (38, 39)
        if p not in (12, 13, 36, 37, 40, 41, 42):  # the outer ethertype, port, checksum and the VXLAN flags decide the walk
            assert bool(pw.code(m, vxlan_port=PORT) & pw.BAD) == bool(want_bad), (k, p)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_translated_frames_and_pyxlat_checker(built, cfg):
    """Translated frames are clean, and on every mutant this checker and pyxlat's from-scratch one agree
    on whether the L4 side of the frame is good."""
    prefix = pyxlat.prefix96("2001:db8:ffff:ffff:ffff:ffff::/96")
    six = pyxlat.xlat_all(built[cfg], prefix, flow_label=0x54321)
    codes, r = pw.result(six)
    assert set(codes) == {0} and r["n_ipv6"] == 300
    l4_side = pw.L4_CSUM | pw.L3_LEN | pw.MALFORMED | pw.NOL4 | pw.OTHER
    n_bad = 0
    for step in (7, 13, 29):
        for p, m in mutants(six, step):
            good = not pw.code(m) & l4_side
            assert good == pyxlat.check6(m), (p, m.hex())
            n_bad += not good
    assert n_bad > 300


def test_fragments_have_no_l4_to_check(built):
    frames = built["c3_udp_var"]
    out = [g for f in frames for g in pyfrag.fragment(f, 576, ignore_df=True)]
    assert len(out) > 500
    codes, r = pw.result(out)
    assert r["n_bad"] == 0
    for g, c in zip(out, codes):
        is_fragment = bool(struct.unpack(">H", g[20:22])[0] & 0x3FFF)
        assert c == (pw.NOL4 if is_fragment else 0)
    assert 0 < r["n_nol4"] < len(out)


# ---- one known answer per class: (frame, code under WIRE_ALL with port 4789, outermost L3)
KAT = {
    "v4_udp": ("e7e2ecfe08ec1a14e34d6924080045e80020cca90000ea112c5e564803add9d0a317067d57c6000c0dade8cad43d", (0, 4)),
    "v4_udp_nocsum": ("35eeb8961c91d9cce318e79d0800454300202b6c00007511e656485b2714462e7e2a061ad7db000c000067a630de", (32, 4)),
    "v4_tcp": ("9361f883c259c9985b4b5d58080045f9002ba43b0000cc0634d84f8efa1af49ad67c0ac0d390600804b086682f01501844384e99460d5f"
               "b76a", (0, 4)),
    "v4_icmp": ("26d35dd4d47a913622da285e080045470021b88e4000e00172495ff4d234f1cf4bc4080005a777765671701d4a536a", (0, 4)),
    "v4_ihl6_udp": ("0d1565c82fff9a77e00038f80800464400242691000013118b5b757fbdcc897aa3ce9404000009264d30000c67b9aceb3446",
                    (0, 4)),
    "v6_udp": ("013af2e57d011832cf973b1486dd6f705aa8000c113e0960856295b491e375d2ce9d2c284c494c9a195ff29615c6abd8165d4714bc7c"
               "09af7815000c787dbbf7a243", (0, 6)),
    "v6_tcp": ("d52e753a0ee1e7158d7e1c0686dd6ae80e140015062003b5c53e2a51b6a3bb344e2f88375e340c34cde7fcbd02d0ccefc78dcd5724ea"
               "ff0a255f2d8844129c467ad5501877e1577fe22857", (0, 6)),
    "v6_icmpv6": ("ee9977559fce8b1b16faf36c86dd691f26f9000c3aea8cda34b20c88b58a9cfb3b56384cc7afaed38c57587992fdd2819d468d90d"
                  "bad800066d626105840bbcd832e", (0, 6)),
    "v4_gre": ("95ca986befbb578d374b48670800457e001c95db40008f2f3b4cf8abb1335d2f12ff000008006d43829b", (32, 4)),
    "v4_first_fragment": ("ad4a3499de99470322dad30a080045aa002484d820002111a0308fd9ef8b7da5570c4153be576a9279536aa768fe863c"
                          "a6f1", (32, 4)),
    "v4_later_fragment": ("47113168d6c05a0db3d9f2db0800450c0024527500b92a1156682f6c6fef64bee30dd690019a9ea4fa012e64f3035801"
                          "c33d", (32, 4)),
    "v6_fragment_header": ("dafe19612c21bf4a29aee96886dd6cd4d2f6000c2c8e6031730318d0250074375bb735e6e05c96e7fa74786056adba9e"
                           "cd966ac9c8ad11000001ca1a7a252a6ad673", (32, 6)),
    "vlan_v4_udp": ("c9acf0b3136b2d56235ebe19810020640800454a002022830000a511caedfda6d990d2aa7e3007073c8c000cc4227b4654c7",
                    (0, 4)),
    "qinq_v6_tcp": ("273aab900ee86dfe8099851688a801238100006486dd6f7cf60e001606e4a5798e474c9094617ff7f037bee759089548b2212a"
                    "a230d9ae3c918c58a5a18ac1c86b32e602bbaeeaa54cc05018a6a0deebe9bcc0bd", (0, 6)),
    "vxlan4_zero_v4_udp": ("ba246681c843a34365c005050800457100527c5c00006c11ec5283d58bab2610afea0b0412b5003e000008000000455"
                           "58c001170bc48f2130a883fedfd9c080045840020352100007011c2bd767fc79e14160037066e87aa000cee10dcb2548f",
                           (64, 4)),
    "vxlan4_csum_v4_tcp": ("2a667a82a5bb4a3879858523080045d3005cccd140005a11bfbd7bbcca5e5670f6a3062c12b5004833b808000000cad"
                           "65d0006a53da21fe8bce0b0f7b2e7080045b5002a9d3440007806c7d03514edd94bc42e62a68884021da946c89fab22"
                           "045018dccb15e00fbfbf9f", (64, 4)),
    "vxlan6_vlan_v4_icmp": ("680a33643ca3ac2379e65d2186dd612293980040119050209a60e9879d975376a55ca3854b0d296bf34f6c364d0f8c"
                            "5cef15629842420acb12b50040e71f0800000024f6a60061733634c233d9bf7c177f6c81002064080045f1001e9014"
                            "40006701652ae03b25e44758d0370800ff10a1351ca73b12", (64, 6)),
    "vxlan4_zero_v4_gre": ("8a7bab27e52226ed1ad05938080045f7004c240d4000a81154c4ec4e0377ae20baf20a2112b50038000008000000"
                           "95de710076a45522a0647fca574bcd12080045d4001a26370000502f9c0ee4e811e8f4e7bbe3000008000dff", (96, 4)),
    "arp": ("ffffffffffff020000000001080600010800060400010200000000010a0000010000000000000a000002", (128, 0)),
}


@pytest.mark.parametrize("name", list(KAT))
def test_known_answer(name):
    h, want = KAT[name]
    f = bytes.fromhex(h)
    assert pw.walk(f, pw.ALL, PORT) == want
    if want[0] & pw.INNER:  # without the port the outer verdict alone
        assert pw.code(f) == (0 if "csum" in name or "vxlan6" in name else pw.NOL4)
    if want[0] == 0:  # the last byte belongs to a summed segment
        assert pw.code(f[:-1] + bytes([f[-1] ^ 1]), pw.ALL, PORT) & pw.L4_CSUM
        assert pw.code(f[:-1] + bytes([f[-1] ^ 1]), pw.ALL & ~pw.L4_CSUM, PORT) & pw.L4_CSUM == 0


# ---- every MALFORMED rule at its boundary length and one byte beyond it
def test_malformed_boundaries():
    k = {n: bytes.fromhex(h) for n, (h, _) in KAT.items()}
    M = pw.MALFORMED

    def c(f):
        return pw.code(f, pw.ALL, PORT)

    # rule 1: 14 bytes of Ethernet; a tag needs its ethertype to fit
    assert c(k["arp"][:13]) == M and c(k["arp"][:14]) == pw.OTHER and c(b"") == M
    assert c(k["vlan_v4_udp"][:17]) == M and c(k["vlan_v4_udp"][:16]) == M and c(k["qinq_v6_tcp"][:21]) == M
    three = k["vlan_v4_udp"][:12] + b"\x81\x00\x00\x01" * 3 + k["vlan_v4_udp"][16:]
    assert c(three) == pw.OTHER  # the third tag is an ethertype like any other: only two are skipped
    # rule 3: 20 bytes of IPv4, the version, IHL >= 5, the options fit
    u, g = k["v4_udp"], k["v4_gre"]  # protocol 47 asks nothing of the bytes behind the header
    assert c(g[:33]) == M and c(g[:34]) == pw.L3_LEN | pw.NOL4
    assert c(u[:14] + b"\x55" + u[15:]) == M and c(u[:14] + b"\x44" + u[15:]) == M
    o = k["v4_ihl6_udp"]
    o = o[:23] + b"\x2f" + o[24:]
    assert c(o[:37]) == M and not c(o[:38]) & M
    # UDP 8, TCP 20, ICMP 8 bytes
    assert c(u[:41]) == M and not c(u[:42]) & M
    t = k["v4_tcp"]
    assert c(t[:53]) == M and not c(t[:54]) & M
    i = k["v4_icmp"]
    assert c(i[:41]) == M and not c(i[:42]) & M
    # rule 4: 40 bytes of IPv6, the version; UDP 8, TCP 20, ICMPv6 4
    s = k["v6_udp"]
    x = k["v6_fragment_header"]  # next header 44 asks nothing of the bytes behind the header
    assert c(x[:53]) == M and c(x[:54]) == pw.L3_LEN | pw.NOL4 and c(s[:14] + b"\x4f" + s[15:]) == M
    assert c(s[:61]) == M and not c(s[:62]) & M
    s = k["v6_tcp"]
    assert c(s[:73]) == M and not c(s[:74]) & M
    s = k["v6_icmpv6"]
    assert c(s[:57]) == M and not c(s[:58]) & M
    # rule 5: a VXLAN header needs 16 bytes of UDP segment; the inner frame 14
    v = k["vxlan4_zero_v4_udp"]
    assert not c(v[:49]) & (M | pw.INNER) and c(v[:50]) & (M | pw.INNER) == M | pw.INNER
    assert c(v[:63]) & M and not c(v[:62] + b"\x08\x06") & M  # 14 bytes of a non-IP inner frame are enough
    vg = k["vxlan4_zero_v4_gre"]
    assert c(vg[:83]) & M and not c(vg[:84]) & M  # the inner IPv4 header, protocol 47 behind it
    assert c(v[:91]) & M and not c(v[:92]) & M  # the inner UDP header


def test_ipv6_udp_zero_checksum_is_a_failure():
    f = bytearray(bytes.fromhex(KAT["v6_udp"][0]))
    f[60:62] = b"\0\0"
    assert pw.code(bytes(f)) == pw.L4_CSUM  # evaluated (no NOL4), and failed
    assert pw.code(bytes(f), pw.ALL & ~pw.L4_CSUM) == 0
    g = bytearray(bytes.fromhex(KAT["v4_udp"][0]))
    g[40:42] = b"\0\0"
    assert pw.code(bytes(g)) == pw.NOL4  # over IPv4 it means "none"
    t = bytearray(bytes.fromhex(KAT["v4_tcp"][0]))
    t[50:52] = b"\0\0"
    assert pw.code(bytes(t)) == pw.L4_CSUM  # TCP has no "none"


def test_rule_6_malformed_level_keeps_the_outer_bits():
    v = bytearray(bytes.fromhex(KAT["vxlan4_zero_v4_udp"][0]))
    v[24] ^= 0xFF  # the outer IPv4 checksum
    cut = bytes(v[:len(v) - 13])  # the inner UDP header no longer fits; the outer lengths are now wrong too
    got = pw.code(cut, pw.ALL, PORT)
    assert got == pw.L3_CSUM | pw.L3_LEN | pw.UDP_LEN | pw.INNER | pw.MALFORMED
    # a malformed outer level gives MALFORMED alone, whatever else was wrong with it
    u = bytearray(bytes.fromhex(KAT["v4_udp"][0]))
    u[24] ^= 0xFF
    assert pw.code(bytes(u)) == pw.L3_CSUM and pw.code(bytes(u[:41])) == pw.MALFORMED


def test_zoo_classes():
    z = wf.zoo()
    assert len(z) > 400
    for label, f in z:
        assert pw.code(f, pw.ALL, PORT) == wf.expected_info(label), label


# ---- the ABI
def test_struct_sizes():
    lib = pbgpu.load_library()
    assert lib.pbgpu_abi_size(16) == C.sizeof(pbgpu.WireOpts) == 16
    assert lib.pbgpu_abi_size(17) == C.sizeof(pbgpu.WireResult) == 112
    assert (pbgpu.WIRE_L3_CSUM, pbgpu.WIRE_L3_LEN, pbgpu.WIRE_L4_CSUM, pbgpu.WIRE_UDP_LEN, pbgpu.WIRE_ALL) == (1, 2, 4, 8, 15)
    assert (pbgpu.WIRE_MALFORMED, pbgpu.WIRE_NOL4, pbgpu.WIRE_INNER, pbgpu.WIRE_OTHER) == (16, 32, 64, 128)
    assert (pw.L3_CSUM, pw.L3_LEN, pw.L4_CSUM, pw.UDP_LEN, pw.MALFORMED, pw.NOL4, pw.INNER, pw.OTHER) == (1, 2, 4, 8, 16, 32, 64, 128)
    assert lib.pbgpu_verify_wire(None, None, 0, 0, None, None, None) == -22


# ---- pcktbatch-gpu --verifywire
BASE = ["-z", "--interface", "pbnodev0", "--dip", "10.0.0.2", "--smac", "02:00:00:00:00:01", "--dmac",
        "02:00:00:00:00:02", "--protocol", "udp", "--pmin", "22", "--pmax", "22", "--seed", "7", "--delay", "0",
        "--maxpckts", "10"]


def test_cli_parses_and_lists_verifywire():
    r = subprocess.run([BIN] + BASE + ["--verifywire", "-l"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "VERIFYWIRE: on" in r.stdout.splitlines()
    both = subprocess.run([BIN] + BASE + ["--verify", "--verifywire", "-l"], capture_output=True, text=True, timeout=60)
    assert both.returncode == 0 and both.stdout == r.stdout
    plain = subprocess.run([BIN] + BASE + ["--verify", "-l"], capture_output=True, text=True, timeout=60)
    assert plain.returncode == 0 and "VERIFYWIRE" not in plain.stdout
    assert plain.stdout.splitlines() == [x for x in r.stdout.splitlines() if x != "VERIFYWIRE: on"]
    h = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0 and "--verifywire =>" in h.stdout


def test_stub_builder_refuses_verifywire(capfd):
    """tests/host_stub.c's table ends before verify_wire: it is NULL, and seq_send refuses the sequence
    before it takes a slot or starts a thread; without the option it runs."""
    os.makedirs(BUILD, exist_ok=True)
    stub_path = os.path.join(BUILD, "libpbhost_stub_wire.so")
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
        assert host.pb_get_verify_wire() == 0
        host.pb_set_verify_wire(1)
        assert host.pb_get_verify_wire() == 1
        assert run() == (-95, 0)
        cap = capfd.readouterr()
        assert "--verifywire" in cap.err and "as sent" not in cap.out
        host.pb_set_verify_wire(0)
        assert run() == (0, 64)
        assert "as sent" not in capfd.readouterr().out
    finally:
        host.pb_set_verify_wire(0)
        host.pb_reset()
        stub.stub_uninstall()
