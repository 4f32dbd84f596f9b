"""Stamping without a GPU: the reference (tests/pystamp.py) against answers worked out by hand and
against the verifier's sums, the ABI, scripts/stamp_read.py on captures with known faults, and what
pcktbatch-gpu --stamp and the host driver refuse."""
import ctypes as C
import json
import os
import struct
import subprocess
import sys

import pytest

import pb_configs as pc
import pbgpu
import pypcap
import pystamp
import pyverify
from cmdline_binding import OurCmd
from pbgpu import Sequence, SequenceT
from stamp_frames import frame_ok, l4_frame, l4_ok

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pb-af-xdp_amd")
LIBDIR = os.path.join(PKG, "lib")
BIN = os.path.join(PKG, "bin", "pcktbatch-gpu")
BUILD = os.path.join(ROOT, "tests", "_build")
READER = os.path.join(ROOT, "scripts", "stamp_read.py")

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import stamp_read  # noqa: E402


# ---- the ABI
def test_struct_sizes():
    lib = pbgpu.load_library()
    assert lib.pbgpu_abi_size(12) == C.sizeof(pbgpu.StampOpts) == 32
    assert lib.pbgpu_abi_size(13) == C.sizeof(pbgpu.StampResult) == 40
    assert (pbgpu.STAMP_TAIL, pbgpu.STAMP_NO_CSUM) == (1, 2)


def test_symbol_rejects_null():
    lib = pbgpu.load_library()
    frames, opts, res = pbgpu.Frames(), pbgpu.StampOpts(), pbgpu.StampResult()
    assert lib.pbgpu_stamp(None, C.byref(frames), 0, 0, C.byref(opts), C.byref(res)) == -22
    assert lib.pbgpu_stamp(None, None, 0, 0, None, None) == -22


# ---- a hand-worked answer
def test_udp_58_byte_by_byte():
    """58 B of UDP: 16 payload bytes, all replaced.  Old payload 00 01 .. 0f, index 1, T 2: the sum of
    the old words is 0x0001 + 0x0203 + .. + 0x0e0f = 0x3840, of the new ones 1 + 2 = 3."""
    f = bytearray(58)
    f[12:14], f[14], f[23] = b"\x08\x00", 0x45, 17
    f[42:58] = bytes(range(16))
    f[40:42] = b"\x12\x34"
    out, cls = pystamp.stamp(bytes(f), 1, 2)
    assert cls == "stamped" and out[42:58] == struct.pack("!QQ", 1, 2)
    s = (~0x1234 & 0xFFFF) + 8 * 0xFFFF - 0x3840 + 3
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    assert out[40:42] == struct.pack("!H", ~s & 0xFFFF)
    assert out[:40] == bytes(f[:40])
    # the same through RFC 1071 from scratch: the sum moved by new - old
    assert (pyverify.ones_sum(bytes(f[34:])) - pyverify.ones_sum(out[34:])) % 0xFFFF == 0


# ---- eligibility, and validity after the stamp
CASES = [(17, L, 5) for L in (58, 59, 60, 64, 65, 98, 199)] + [(1, L, 5) for L in (58, 59, 98, 101)] + \
        [(6, L, 5) for L in (70, 71, 90)] + [(6, L, 8) for L in (82, 83, 120)]


@pytest.mark.parametrize("proto,L,doff", CASES)
def test_valid_frames_stay_valid(proto, L, doff):
    f = l4_frame(proto, L, 3, doff)
    assert frame_ok(f)
    H = 8 if proto != 6 else 4 * doff
    room = L - 34 - H - 16
    for tail in (False, True):
        for offset in range(0, room + 2):
            out, cls = pystamp.stamp(f, 0xDEADBEEF00 + offset, 1_700_000_000_123_456_789, offset, tail)
            if offset > room:
                assert cls == "short" and out == f
                continue
            assert cls == "stamped" and out != f
            _, S, Q = pystamp.position(f, offset, tail)
            assert S == (L - 16 - offset if tail else 34 + H + offset)
            assert out[S:S + 16] == struct.pack("!QQ", 0xDEADBEEF00 + offset, 1_700_000_000_123_456_789)
            assert [i for i in range(L) if out[i] != f[i] and not (S <= i < S + 16 or Q <= i < Q + 2)] == []
            assert frame_ok(out), (tail, offset)


@pytest.mark.parametrize("L,offset,tail,a,words", [(64, 0, False, 8, 8), (64, 1, False, 9, 9), (65, 0, True, 15, 9),
                                                   (59, 0, True, 9, 9), (59, 1, True, 8, 8)])
def test_even_and_odd_a_and_the_missing_byte(L, offset, tail, a, words):
    """Even a: 8 words.  Odd a: 9, and where the stamp ends a frame of odd L4 length the 9th word's
    second byte lies past the frame and counts as 0."""
    f = l4_frame(17, L, 11)
    cls, S, _ = pystamp.position(f, offset, tail)
    assert cls == "stamped" and S - 34 == a
    assert len(pystamp._words(f, a)) == words
    if a & 1 and S + 16 == L:
        assert pystamp._words(f, a)[-1] == f[L - 1] << 8
    out, _ = pystamp.stamp(f, 2**64 - 1, 2**63 + 5, offset, tail)
    assert frame_ok(out)


def test_no_csum_leaves_the_field():
    f = l4_frame(17, 98, 9)
    out, cls = pystamp.stamp(f, 7, 8, 3, False, csum=False)
    assert cls == "stamped" and out[40:42] == f[40:42] and out[45:61] == struct.pack("!QQ", 7, 8)
    assert out[:45] == f[:45] and out[61:] == f[61:] and not l4_ok(out)


def test_classes():
    udp = l4_frame(17, 98, 1)
    assert pystamp.stamp(l4_frame(17, 57, 1), 0, 0)[1] == "short"
    assert pystamp.stamp(l4_frame(6, 46, 1), 0, 0)[1] == "short"
    assert pystamp.stamp(l4_frame(6, 69, 1), 0, 0)[1] == "short"
    assert pystamp.stamp(l4_frame(6, 81, 1, doff=8), 0, 0)[1] == "short"
    assert pystamp.stamp(l4_frame(6, 82, 1, doff=8), 0, 0)[1] == "stamped"
    others = [l4_frame(17, 98, 1, ethertype=b"\x86\xdd"), l4_frame(17, 98, 1, vihl=0x46), l4_frame(17, 98, 1, fo=0x2000),
              l4_frame(17, 98, 1, fo=0x0001), l4_frame(47, 98, 1), l4_frame(6, 98, 1, doff=4), udp[:33], udp[:13], b""]
    for f in others:
        assert pystamp.stamp(f, 0, 0) == (f, "other")
    assert pystamp.stamp(l4_frame(17, 98, 1, fo=0x4000), 0, 0)[1] == "stamped"  # DF is no fragment
    assert pystamp.stamp(l4_frame(17, 98, 1, fo=0x8000), 0, 0)[1] == "stamped"


def test_stamp_buffer_counts_and_time():
    frames = [l4_frame(17, 64, 1), l4_frame(17, 50, 2), l4_frame(47, 64, 3), l4_frame(1, 98, 4)]
    data = b"".join(frames)
    off = [0, 64, 114, 178, 276]
    out, cnt = pystamp.stamp_buffer(data, off, first=1, n=3, t0_ns=10**18, step_ps=672_000, first_index=5)
    assert cnt == dict(stamped=1, short=1, other=1)
    assert out[:178] == data[:178]
    assert out[178 + 42:178 + 58] == struct.pack("!QQ", 7, 10**18 + 7 * 672_000 // 1000)
    assert pystamp.stamp_time(7, 10**18, 672_000) == sum(pypcap.stamp(7, 10**18, 672_000, nsec=True)[i] * m
                                                       for i, m in ((0, 10**9), (1, 1)))


# ---- scripts/stamp_read.py
def _capture(indices, t0_ns, step_ps, nsec, late_ns=0, tail=False, offset=0, extra=()):
    """A capture of 98-B UDP frames stamped with `indices` in that order, record j written at the
    scheduled time of its own stamp plus late_ns; `extra` frames (unstamped) are appended."""
    out = [pypcap.pcap_file_header(nsec)]
    for idx in indices:
        T = pystamp.stamp_time(idx, t0_ns, step_ps)
        f, cls = pystamp.stamp(l4_frame(17, 98, idx), idx, T, offset, tail)
        assert cls == "stamped"
        t = T + late_ns
        frac = t % 10**9 if nsec else t % 10**9 // 1000
        out.append(struct.pack("<4I", t // 10**9 % 2**32, frac, len(f), len(f)) + f)
    for f in extra:
        out.append(struct.pack("<4I", 0, 0, len(f), len(f)) + f)
    return b"".join(out)


@pytest.mark.parametrize("nsec", [False, True])
@pytest.mark.parametrize("tail,offset", [(False, 0), (True, 0), (False, 5), (True, 7)])
def test_reader_clean_capture(nsec, tail, offset):
    cap = _capture(range(100, 164), 1_700_000_000_000_000_000, 672_000, nsec, tail=tail, offset=offset)
    got = stamp_read.analyse(cap, tail, offset)
    assert got == dict(frames=64, stamped=64, min_index=100, max_index=163, missing=0, duplicates=0, out_of_order=0,
                       delta_ns_min=0, delta_ns_median=0.0, delta_ns_max=0)


def test_reader_drops_duplicates_and_swaps(tmp_path):
    idx = list(range(40))
    for d in (7, 8, 30):       # three drops
        idx.remove(d)
    idx.insert(10, 3)          # 3 arrives again (a duplicate, and below the highest seen: out of order)
    a, b = idx.index(20), idx.index(21)
    idx[a], idx[b] = idx[b], idx[a]  # one swap: 20 arrives after 21
    others = [l4_frame(47, 98, 1), l4_frame(17, 50, 2)]
    cap = _capture(idx, 5 * 10**9, 10**9, True, late_ns=1500, extra=others)
    path = tmp_path / "faults.pcap"
    path.write_bytes(cap)
    r = subprocess.run([sys.executable, READER, str(path), "head"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    assert json.loads(lines[0]) == dict(frames=40, stamped=38, min_index=0, max_index=39, missing=3, duplicates=1,
                                        out_of_order=2, delta_ns_min=1500, delta_ns_median=1500.0, delta_ns_max=1500)


def test_reader_microsecond_file_cuts_both_sides():
    cap = _capture(range(8), 1_700_000_000_000_000_999, 1_234_567, False)
    got = stamp_read.analyse(cap)
    assert (got["delta_ns_min"], got["delta_ns_max"], got["stamped"]) == (0, 0, 8)


@pytest.mark.parametrize("spec", ["", "mid", "head:", "head:x", "tail:-1", "head:65536", "head:1:2"])
def test_reader_refuses_bad_position(tmp_path, spec):
    path = tmp_path / "c.pcap"
    path.write_bytes(pypcap.pcap_file_header())
    r = subprocess.run([sys.executable, READER, str(path), spec], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == ""


# ---- scripts/stamp_host.c: the benchmark's host method computes the same bytes
@pytest.mark.parametrize("tail,offset,csum", [(False, 0, True), (True, 0, True), (False, 3, True), (True, 5, False)])
def test_bench_host_method_equals_reference(tail, offset, csum):
    import numpy as np
    from stamp_frames import pack

    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libstamp_host.so")
    tmp = f"{so}.{os.getpid()}"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread", "-o", tmp,
                    os.path.join(ROOT, "scripts", "stamp_host.c")], check=True)
    os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.stamp_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                               C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)]
    frames = [l4_frame((17, 6, 1, 47)[j % 4], 30 + (j * 13) % 120, j, doff=(5, 8, 4)[j % 3]) for j in range(500)]
    data, off = pack(frames)
    want, cnt = pystamp.stamp_buffer(data.tobytes(), off, 0, None, 10**18, 672_000, 2**40, offset, tail, csum)
    buf, counts = data.copy(), (C.c_uint64 * 3)()
    flags = (1 if tail else 0) | (0 if csum else 2)
    assert lib.stamp_host(buf.ctypes.data, off.ctypes.data, 0, 500, 10**18, 672_000, 2**40, offset, flags, 16, counts) == 0
    assert buf.tobytes() == want and list(counts) == [cnt["stamped"], cnt["short"], cnt["other"]]
    fixed = [l4_frame(17, 65, j) for j in range(300)]
    data, off = pack(fixed)
    want, _ = pystamp.stamp_buffer(data.tobytes(), off, 0, None, 5, 1000, 7, offset, tail, csum)
    buf = data.copy()
    assert lib.stamp_host(buf.ctypes.data, None, 65, 300, 5, 1000, 7, offset, flags, 3, counts) == 0
    assert buf.tobytes() == want


# ---- pcktbatch-gpu --stamp: malformed values are refused before any GPU is opened
BASE = ["-z", "--interface", "pbnodev0", "--dip", "10.0.0.2", "--smac", "02:00:00:00:00:01", "--dmac",
        "02:00:00:00:00:02", "--protocol", "udp", "--pmin", "22", "--pmax", "22", "--seed", "7", "--delay", "0",
        "--maxpckts", "10"]
BAD_SPECS = ["bogus", "", "mid:3", "head:", "head:x", "head:65536", "tail:-1", "head:1:2", "Head", "tail:0x10",
             "head:99999999999999999999", " head"]


@pytest.mark.parametrize("spec", BAD_SPECS)
def test_cli_refuses_malformed_values(tmp_path, spec):
    out = tmp_path / "out.pcap"
    r = subprocess.run([BIN] + BASE + ["--stamp", spec, "--pcapdump", str(out)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0
    assert "--stamp" in r.stderr and spec in r.stderr
    assert "GPU" not in r.stderr and not out.exists()


def test_cli_allows_one_stamp(tmp_path):
    out = tmp_path / "out.pcap"
    r = subprocess.run([BIN] + BASE + ["--stamp", "head", "--stamp", "tail:4", "--pcapdump", str(out)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--stamp given more than once" in r.stderr and not out.exists()


def test_help_lists_stamp():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--stamp head[:OFF] | tail[:OFF]" in r.stdout and "scheduled" in r.stdout


# ---- the host driver with a builder that cannot stamp
def test_stub_builder_refuses_stamp(capfd):
    """tests/host_stub.c's table ends before the stamp member: it is NULL, and seq_send refuses the
    sequence before it takes a slot or starts a thread; without --stamp it runs."""
    os.makedirs(BUILD, exist_ok=True)
    stub_path = os.path.join(BUILD, "libpbhost_stub_stamp.so")
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
    host.pb_set_stamp.argtypes = [C.POINTER(pbgpu.StampOpts), C.c_int]
    host.pb_get_stamp.restype = C.POINTER(pbgpu.StampOpts)
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
        assert not host.pb_get_stamp()
        opts = pbgpu.StampOpts(0, 0, 0, 4, pbgpu.STAMP_TAIL)
        host.pb_set_stamp(C.byref(opts), 0)
        got = host.pb_get_stamp().contents
        assert (got.offset, got.flags) == (4, 1)
        err, pckts = run()
        assert (err, pckts) == (-95, 0)
        assert "--stamp" in capfd.readouterr().err
        host.pb_set_stamp(None, 0)
        assert not host.pb_get_stamp()
        assert run() == (0, 64)
    finally:
        host.pb_set_stamp(None, 0)
        host.pb_reset()
        stub.stub_uninstall()
