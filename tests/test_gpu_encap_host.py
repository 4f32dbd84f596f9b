"""pcktbatch-gpu --encap on the GPU: what --pcapdump writes and what the loopback TX path sends are
tests/pyencap.py applied to the frames of the same run without --encap (same arguments, seed, MACs
and --pcapt0); the end-of-run totals count the encapsulated bytes; --verify and -v."""
import os
import re
import subprocess

import pytest

import pb_configs as pc
import pyencap
import pypcap
from pbgpu import parse_mac

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pb-af-xdp_amd", "bin", "pcktbatch-gpu")
T0 = 1_700_000_000_000_000_000
COMMON = ["-z", "--interface", "pbnodev0", "--smac", pc.SMAC, "--dmac", pc.DMAC, "--dip", pc.DIP, "--sip",
          "10.20.0.0/16", "--protocol", "udp", "--udport", "27015"]
TOTAL = re.compile(r"^\[(\d+)\] Completed sequence with a total of (\d+) packets and (\d+) bytes\.", re.M)
SENT = re.compile(r"^\[1\]\[1\] Sent (\d+) bytes of data from (\S+) to (\S+)\.$", re.M)

SPECS = {
    "vxlan": "vxlan:5000:192.0.2.1:198.51.100.2",
    "vxlan_dport": "vxlan:16777215:10.1.2.3:10.4.5.6:8472",
    "vlan": "vlan:100:5",
}


def encap(spec, frame):
    f = spec.split(":")
    if f[0] == "vlan":
        return pyencap.vlan(frame, (int(f[2]) << 13 if len(f) > 2 else 0) | int(f[1]))
    return pyencap.vxlan(frame, dst_mac=parse_mac(pc.DMAC), src_mac=parse_mac(pc.SMAC),
                         src_ip=bytes(int(x) for x in f[2].split(".")), dst_ip=bytes(int(x) for x in f[3].split(".")),
                         vni=int(f[1]), dst_port=int(f[4]) if len(f) > 4 else 0)


def run(args):
    r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def dump(tmp_path, args, name):
    out = tmp_path / name
    r = run(args + ["--pcapdump", str(out), "--pcapt0", str(T0)])
    return r, out.read_bytes()


@pytest.mark.parametrize("spec", list(SPECS))
@pytest.mark.parametrize("pmin,pmax", [(22, 22), (0, 900)])
def test_pcapdump_with_encap(tmp_path, pmin, pmax, spec):
    """1000 frames in batches of 256 (four, the last partial) at 1 Mpps."""
    args = COMMON + ["--pmin", str(pmin), "--pmax", str(pmax), "--pps", "1000000", "--maxpckts", "1000", "--gpubatch",
                     "256", "--seed", "7"]
    _, plain = dump(tmp_path, args, "plain.pcap")
    frames = [f for _, _, f in pypcap.read_pcap(plain)[1]]
    assert len(frames) == 1000
    r, got = dump(tmp_path, args + ["--encap", SPECS[spec]], "encap.pcap")
    want = [encap(SPECS[spec], f) for f in frames]
    assert got == pypcap.pcap_stream(want, T0, 10**6, 0, True, False)
    assert TOTAL.findall(r.stdout) == [("1", "1000", str(sum(len(f) for f in want)))]


@pytest.mark.parametrize("spec", ["vxlan", "vlan"])
def test_loopback_tx_path_and_totals(tmp_path, spec):
    """One TX thread through the loopback ring into --pcap: the frames sent, in order, are the
    encapsulated ones, and the totals line counts their bytes."""
    args = COMMON + ["--pmin", "0", "--pmax", "300", "--maxpckts", "3000", "--delay", "0", "--gpubatch", "1000",
                     "--seed", "4242", "--threads", "1", "--track", "1"]
    plain, enc = tmp_path / "plain.pcap", tmp_path / "enc.pcap"
    r0 = run(args + ["--pcap", str(plain)])
    r1 = run(args + ["--pcap", str(enc), "--encap", SPECS[spec]])
    a = [f for _, _, f in pypcap.read_pcap(plain.read_bytes())[1]]
    b = [f for _, _, f in pypcap.read_pcap(enc.read_bytes())[1]]
    want = [encap(SPECS[spec], f) for f in a]
    assert len(a) == 3000 and b == want
    P = 4 if spec == "vlan" else 50
    assert TOTAL.findall(r0.stdout) == [("1", "3000", str(sum(len(f) for f in a)))]
    assert TOTAL.findall(r1.stdout) == [("1", "3000", str(sum(len(f) for f in a) + 3000 * P))]


def test_maxbytes_counts_encapsulated_bytes(tmp_path):
    """64-B frames under VXLAN are 114 B on the ring: --maxbytes 11400 is 100 frames, not 179."""
    args = COMMON + ["--pmin", "22", "--pmax", "22", "--maxbytes", "11400", "--delay", "0", "--seed", "3", "--threads", "1",
                     "--gpubatch", "1000", "--track", "1", "--encap", SPECS["vxlan"]]
    r = run(args)
    assert TOTAL.findall(r.stdout) == [("1", "100", "11400")]


@pytest.mark.parametrize("spec", ["vxlan", "vlan"])
def test_verify_with_encap(tmp_path, spec):
    args = COMMON + ["--pmin", "0", "--pmax", "500", "--maxpckts", "2000", "--delay", "0", "--gpubatch", "512",
                     "--seed", "11", "--verify", "--encap", SPECS[spec]]
    r = run(args + ["--threads", "1"])
    assert r.stdout.splitlines()[-1] == "Verified 2000 frames on the GPU: 0 bad."
    r, got = dump(tmp_path, args, "v.pcap")
    assert r.stdout.splitlines()[-1] == "Verified 2000 frames on the GPU: 0 bad."
    assert len(pypcap.read_pcap(got)[1]) == 2000


def test_frames_that_outgrow_the_umem_slot_are_refused(tmp_path):
    """64-B frames fit 64-B slots; with the 50-B outer header they do not: refused with a message
    before anything is sent, and 128-B slots take them."""
    args = COMMON + ["--pmin", "22", "--pmax", "22", "--maxpckts", "100", "--delay", "0", "--seed", "3", "--threads", "1",
                     "--track", "1", "--encap", SPECS["vxlan"]]
    out = tmp_path / "none.pcap"
    r = subprocess.run([BIN] + args + ["--umemslot", "64", "--pcap", str(out)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "--encap" in r.stderr and "64-B UMEM slot" in r.stderr
    assert pypcap.read_pcap(out.read_bytes())[1] == []
    r = run(args + ["--umemslot", "128"])
    assert TOTAL.findall(r.stdout) == [("1", "100", "11400")]


def test_verbose_line_reads_past_the_vlan_tag():
    """-v under vlan: the inner addresses and ports, and the length as sent; under vxlan the outer ones."""
    args = COMMON + ["--pmin", "22", "--pmax", "22", "--maxpckts", "50", "--delay", "0", "--seed", "5", "--threads", "1",
                     "-v"]
    plain = SENT.findall(run(args).stdout)
    assert len(plain) == 50 and all(n == "64" and dst == pc.DIP + ":27015" for n, _, dst in plain)
    tagged = SENT.findall(run(args + ["--encap", SPECS["vlan"]]).stdout)
    assert tagged == [("68", src, dst) for _, src, dst in plain]
    outer = SENT.findall(run(args + ["--encap", SPECS["vxlan"]]).stdout)
    assert len(outer) == 50
    for n, src, dst in outer:
        ip, port = src.split(":")
        assert n == "114" and ip == "192.0.2.1" and 49152 <= int(port) <= 65535 and dst == "198.51.100.2:4789"
