"""The pcap surface without a GPU: the Python reference stream (tests/pypcap.py) against a
hand-written known answer, the file the existing --pcap hook writes, the option struct's size, and
pcktbatch-gpu --pcapdump's refusals and help text."""
import ctypes as C
import os
import subprocess

import pytest

import pbgpu
import pypcap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pb-af-xdp_amd")
BIN = os.path.join(PKG, "bin", "pcktbatch-gpu")

# ---- the known answer: frames of 0, 1 and 60 bytes, t0 = 1699999999.999998500 s, 1000 ns apart:
# the three stamps are ...99.999998500, ...99.999999500 and 1700000000.000000500, so the second
# rolls over inside the stream.  Written out by hand, little-endian.
KAT_FRAMES = [b"", b"\xab", bytes(range(60))]
KAT_T0 = 1_699_999_999_999_998_500
KAT_STEP = 1_000_000
KAT_US = (
    b"\xd4\xc3\xb2\xa1\x02\x00\x04\x00\x00\x00\x00\x00\x00\x00\x00\x00\xff\xff\x00\x00\x01\x00\x00\x00"
    # record 0: 1699999999 = 0x6553f0ff s, 999998 = 0xf423e us, length 0
    b"\xff\xf0\x53\x65\x3e\x42\x0f\x00\x00\x00\x00\x00\x00\x00\x00\x00"
    # record 1: same second, 999999 = 0xf423f us, length 1
    b"\xff\xf0\x53\x65\x3f\x42\x0f\x00\x01\x00\x00\x00\x01\x00\x00\x00\xab"
    # record 2: 1700000000 = 0x6553f100 s, 0 us, length 60
    b"\x00\xf1\x53\x65\x00\x00\x00\x00\x3c\x00\x00\x00\x3c\x00\x00\x00"
    b"\x00\x01\x02\x03\x04\x05\x06\x07\x08\x09\x0a\x0b\x0c\x0d\x0e\x0f"
    b"\x10\x11\x12\x13\x14\x15\x16\x17\x18\x19\x1a\x1b\x1c\x1d\x1e\x1f"
    b"\x20\x21\x22\x23\x24\x25\x26\x27\x28\x29\x2a\x2b\x2c\x2d\x2e\x2f"
    b"\x30\x31\x32\x33\x34\x35\x36\x37\x38\x39\x3a\x3b"
)
KAT_NS = (
    b"\x4d\x3c\xb2\xa1\x02\x00\x04\x00\x00\x00\x00\x00\x00\x00\x00\x00\xff\xff\x00\x00\x01\x00\x00\x00"
    # 999998500 = 0x3b9ac424 ns, 999999500 = 0x3b9ac80c ns, 500 = 0x1f4 ns
    b"\xff\xf0\x53\x65\x24\xc4\x9a\x3b\x00\x00\x00\x00\x00\x00\x00\x00"
    b"\xff\xf0\x53\x65\x0c\xc8\x9a\x3b\x01\x00\x00\x00\x01\x00\x00\x00\xab"
    b"\x00\xf1\x53\x65\xf4\x01\x00\x00\x3c\x00\x00\x00\x3c\x00\x00\x00"
    b"\x00\x01\x02\x03\x04\x05\x06\x07\x08\x09\x0a\x0b\x0c\x0d\x0e\x0f"
    b"\x10\x11\x12\x13\x14\x15\x16\x17\x18\x19\x1a\x1b\x1c\x1d\x1e\x1f"
    b"\x20\x21\x22\x23\x24\x25\x26\x27\x28\x29\x2a\x2b\x2c\x2d\x2e\x2f"
    b"\x30\x31\x32\x33\x34\x35\x36\x37\x38\x39\x3a\x3b"
)


@pytest.mark.parametrize("nsec,want", [(False, KAT_US), (True, KAT_NS)])
def test_pypcap_known_answer(nsec, want):
    got = pypcap.pcap_stream(KAT_FRAMES, KAT_T0, KAT_STEP, 0, True, nsec)
    assert got == want
    assert len(got) == 24 + 16 * 3 + 61
    # without the file header: the same bytes from 24 on; a later first_index continues the clock
    assert pypcap.pcap_stream(KAT_FRAMES, KAT_T0, KAT_STEP, 0, False, nsec) == want[24:]
    assert pypcap.pcap_stream(KAT_FRAMES[1:], KAT_T0, KAT_STEP, 1, False, nsec) == want[24 + 16:]
    is_ns, recs = pypcap.read_pcap(want)
    assert is_ns == nsec and [r[2] for r in recs] == KAT_FRAMES
    assert [r[0] for r in recs] == [1699999999, 1699999999, 1700000000]
    assert [r[1] for r in recs] == ([999998500, 999999500, 500] if nsec else [999998, 999999, 0])


def test_pypcap_seconds_wrap_and_bad_input():
    assert pypcap.stamp(0, (2**32 + 5) * 10**9 + 7, 0, True) == (5, 7)
    assert pypcap.stamp(3, 0, 333_333, True) == (0, 999)  # floor(999999 / 1000), not 3 * floor(333.333)
    with pytest.raises(ValueError):
        pypcap.read_pcap(b"\x00" * 24)
    with pytest.raises(ValueError):
        pypcap.read_pcap(KAT_US[:-1])


@pytest.mark.parametrize("mod", ["dpkt", "scapy"])
def test_known_answer_parses_with_a_third_party_reader(mod, tmp_path):
    m = pytest.importorskip(mod)
    if mod == "dpkt":
        import io

        got = [bytes(buf) for _, buf in m.pcap.Reader(io.BytesIO(KAT_US))]
    else:
        from scapy.utils import RawPcapReader

        path = tmp_path / "kat.pcap"
        path.write_bytes(KAT_US)
        got = [bytes(pkt) for pkt, _ in RawPcapReader(str(path))]
    assert got == KAT_FRAMES


def test_read_pcap_reads_the_tx_hooks_file(tmp_path):
    """pb_pcap_open / pb_pcap_tx (the --pcap path) write the file header the stream definition
    names; read_pcap takes the file apart."""
    lib = C.CDLL(os.path.join(PKG, "lib", "libpbhost.so"))
    lib.pb_pcap_open.restype = C.c_void_p
    lib.pb_pcap_open.argtypes = [C.c_char_p]
    lib.pb_pcap_tx.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_uint16]
    lib.pb_pcap_close.argtypes = [C.c_void_p]
    path = tmp_path / "hook.pcap"
    h = lib.pb_pcap_open(str(path).encode())
    assert h
    frames = [bytes(range(60)), b"\x01\x02\x03", bytes(200)]
    for f in frames:
        assert lib.pb_pcap_tx(h, 0, f, len(f)) == 0
    lib.pb_pcap_close(h)
    data = path.read_bytes()
    assert data[:24] == pypcap.pcap_file_header(False) == KAT_US[:24]
    is_ns, recs = pypcap.read_pcap(data)
    assert not is_ns and [r[2] for r in recs] == frames
    assert all(r[1] < 10**6 for r in recs)


def test_opts_struct_size():
    lib = pbgpu.load_library()
    assert lib.pbgpu_abi_size(8) == C.sizeof(pbgpu.PcapOpts) == 32
    assert pbgpu.PcapOpts.flags.offset == 24 and pbgpu.PcapOpts.reserved.offset == 28
    assert lib.pbgpu_abi_size(99) == 0
    assert (pbgpu.PCAP_FILE_HEADER, pbgpu.PCAP_NSEC) == (1, 2)


def test_null_arguments_are_refused():
    lib = pbgpu.load_library()
    frames, dst, opts = pbgpu.Frames(), pbgpu.Frames(), pbgpu.PcapOpts()
    n, ms = C.c_uint64(), C.c_double()
    assert lib.pbgpu_pcap_size(None, C.byref(frames), 0, 0, 1, C.byref(n)) == -22
    assert lib.pbgpu_pcap_pack(None, C.byref(frames), 0, 0, C.byref(opts), C.byref(dst), C.byref(n), C.byref(ms)) == -22


# ---- pcktbatch-gpu --pcapdump: what it refuses, before any GPU is opened
BASE = ["-z", "--interface", "pbnodev0", "--dip", "10.0.0.2", "--smac", "02:00:00:00:00:01", "--dmac",
        "02:00:00:00:00:02", "--protocol", "udp", "--pmin", "22", "--pmax", "22", "--seed", "7", "--delay", "0"]
REFUSALS = {
    "no_maxpckts": [],
    "maxbytes": ["--maxpckts", "100", "--maxbytes", "6400"],
    "time": ["--maxpckts", "100", "--time", "1"],
    "pcap": ["--maxpckts", "100", "--pcap", "{other}"],
    "tx_xsk": ["--maxpckts", "100", "--tx", "xsk"],
    "gpus_2": ["--maxpckts", "100", "--gpus", "2"],
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_pcapdump_refusals(tmp_path, case):
    out, other = tmp_path / "out.pcap", tmp_path / "other.pcap"
    args = [a.format(other=other) for a in REFUSALS[case]]
    r = subprocess.run([BIN] + BASE + args + ["--pcapdump", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--pcapdump" in r.stderr
    assert not out.exists() and not other.exists()


def test_help_lists_pcapdump():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--pcapdump" in r.stdout and "--pcapt0" in r.stdout
