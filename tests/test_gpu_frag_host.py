"""pcktbatch-gpu --fragment on the GPU: what --pcapdump writes and what the loopback TX path sends are
tests/pyfrag.py applied to the frames of the same run without --fragment (same arguments, seed, MACs
and --pcapt0); quotas, totals, --encap, --verify and -v."""
import os
import re
import subprocess

import pytest

import pb_configs as pc
import pyencap
import pyfrag
import pypcap
from pbgpu import parse_mac

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pb-af-xdp_amd", "bin", "pcktbatch-gpu")
T0 = 1_700_000_000_000_000_000
COMMON = ["-z", "--interface", "pbnodev0", "--smac", pc.SMAC, "--dmac", pc.DMAC, "--dip", pc.DIP, "--sip",
          "10.20.0.0/16", "--protocol", "udp", "--udport", "27015"]
JUMBO = COMMON + ["--pmin", "9001", "--pmax", "9001"]  # udp_jumbo_fixed_odd: 9043-B frames
TOTAL = re.compile(r"^\[(\d+)\] Completed sequence with a total of (\d+) packets and (\d+) bytes\.", re.M)
FRAGS = re.compile(r"^\[(\d+)\] Fragmented into (\d+) frames\.$", re.M)
SENT = re.compile(r"^\[1\]\[\d+\] Sent (\d+) bytes of data from (\S+):(\d+) to (\S+):(\d+)\.$", re.M)


def run(args):
    r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def dump(tmp_path, args, name):
    out = tmp_path / name
    r = run(args + ["--pcapdump", str(out), "--pcapt0", str(T0)])
    return r, out.read_bytes()


def frames_of(pcap_bytes):
    return [f for _, _, f in pypcap.read_pcap(pcap_bytes)[1]]


def frag_all(frames, mtu, ignore_df=False):
    return [x for f in frames for x in pyfrag.fragment(f, mtu, ignore_df)]


def regroup(frags, mtu_frames):
    """The fragments back in groups, one per source frame, by the count pyfrag gave for each."""
    out, i = [], 0
    for k in mtu_frames:
        out.append(frags[i:i + k])
        i += k
    assert i == len(frags)
    return out


@pytest.mark.parametrize("pmin,pmax,mtu", [(9001, 9001, "1500"), (0, 3000, "576"), (22, 22, "1500:ignoredf")])
def test_pcapdump_with_fragment(tmp_path, pmin, pmax, mtu):
    """300 packets in batches of 64 (five, the last partial) at 1 Mpps: the capture holds pyfrag's
    fragments, stamped by their own index, and reassembles to the run without --fragment."""
    args = COMMON + ["--pmin", str(pmin), "--pmax", str(pmax), "--pps", "1000000", "--maxpckts", "300", "--gpubatch",
                     "64", "--seed", "7"]
    _, plain = dump(tmp_path, args, "plain.pcap")
    frames = frames_of(plain)
    assert len(frames) == 300
    r, got = dump(tmp_path, args + ["--fragment", mtu], "frag.pcap")
    m = int(mtu.split(":")[0])
    want = frag_all(frames, m)
    assert got == pypcap.pcap_stream(want, T0, 10**6, 0, True, False)
    groups = regroup(frames_of(got), [len(pyfrag.fragment(f, m)) for f in frames])
    assert [pyfrag.reassemble(g) for g in groups] == frames
    assert TOTAL.findall(r.stdout) == [("1", "300", str(sum(len(f) for f in want)))]
    assert FRAGS.findall(r.stdout) == [("1", str(len(want)))]
    if pmin == 9001:
        assert len(want) == 2100


def test_jumbo_frames_send_only_with_fragment(tmp_path):
    """9043-B frames do not fit 4-KiB UMEM slots: refused without --fragment; with --fragment 1500 the
    loopback TX path sends pyfrag's fragments of them, in order, and the totals count what was sent."""
    args = JUMBO + ["--maxpckts", "200", "--delay", "0", "--gpubatch", "64", "--seed", "4242", "--threads", "1",
                    "--track", "1"]
    none = tmp_path / "none.pcap"
    r = subprocess.run([BIN] + args + ["--pcap", str(none)], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "Error landing frames" in r.stderr
    assert pypcap.read_pcap(none.read_bytes())[1] == []
    _, plain = dump(tmp_path, args, "plain.pcap")
    frames = frames_of(plain)
    assert len(frames) == 200 and all(len(f) == 9043 for f in frames)
    sent = tmp_path / "sent.pcap"
    r = run(args + ["--fragment", "1500", "--pcap", str(sent)])
    want = frag_all(frames, 1500)
    assert frames_of(sent.read_bytes()) == want
    assert TOTAL.findall(r.stdout) == [("1", "1400", str(9247 * 200))]


def test_loopback_tx_path_variable_lengths(tmp_path):
    args = COMMON + ["--pmin", "0", "--pmax", "4000", "--maxpckts", "1500", "--delay", "0", "--gpubatch", "500",
                     "--seed", "99", "--threads", "1", "--track", "1"]
    plain, sent = tmp_path / "plain.pcap", tmp_path / "sent.pcap"
    run(args + ["--pcap", str(plain)])
    r = run(args + ["--pcap", str(sent), "--fragment", "576"])
    a = frames_of(plain.read_bytes())
    want = frag_all(a, 576)
    assert len(a) == 1500 and frames_of(sent.read_bytes()) == want
    assert TOTAL.findall(r.stdout) == [("1", str(len(want)), str(sum(len(f) for f in want)))]


def test_fragment_then_encap(tmp_path):
    """--encap takes the fragments: the MTU is the inner packet's."""
    spec = "vxlan:5000:192.0.2.1:198.51.100.2"
    args = JUMBO + ["--pps", "1000000", "--maxpckts", "100", "--gpubatch", "32", "--seed", "7"]
    _, plain = dump(tmp_path, args, "plain.pcap")
    frags = frag_all(frames_of(plain), 1500)
    want = [pyencap.vxlan(f, dst_mac=parse_mac(pc.DMAC), src_mac=parse_mac(pc.SMAC), src_ip=bytes([192, 0, 2, 1]),
                          dst_ip=bytes([198, 51, 100, 2]), vni=5000) for f in frags]
    r, got = dump(tmp_path, args + ["--fragment", "1500", "--encap", spec], "fe.pcap")
    assert got == pypcap.pcap_stream(want, T0, 10**6, 0, True, False)
    assert TOTAL.findall(r.stdout) == [("1", "100", str(sum(len(f) for f in want)))]
    sent = tmp_path / "sent.pcap"
    r = run(args + ["--fragment", "1500", "--encap", spec, "--pcap", str(sent), "--delay", "0", "--threads", "1",
                    "--track", "1"])
    assert frames_of(sent.read_bytes()) == want
    assert TOTAL.findall(r.stdout) == [("1", "700", str(sum(len(f) for f in want)))]


def test_verify_with_fragment(tmp_path):
    args = COMMON + ["--pmin", "0", "--pmax", "5000", "--maxpckts", "1000", "--delay", "0", "--gpubatch", "256",
                     "--seed", "11", "--verify", "--fragment", "1500"]
    r = run(args + ["--threads", "1"])
    assert r.stdout.splitlines()[-1] == "Verified 1000 frames on the GPU: 0 bad."
    r, got = dump(tmp_path, args, "v.pcap")
    assert r.stdout.splitlines()[-1] == "Verified 1000 frames on the GPU: 0 bad."
    assert len(frames_of(got)) > 1000


def test_maxpckts_counts_packets_and_maxbytes_counts_sent_bytes(tmp_path):
    """--maxpckts 10 builds 10 packets (70 frames on the ring); --maxbytes 92470 is 10 packets' fragments."""
    base = JUMBO + ["--delay", "0", "--seed", "3", "--threads", "1", "--gpubatch", "8", "--track", "1", "--fragment", "1500"]
    r = run(base + ["--maxpckts", "10"])
    assert TOTAL.findall(r.stdout) == [("1", "70", "92470")]
    r = run(base + ["--maxbytes", "92470"])
    assert TOTAL.findall(r.stdout) == [("1", "70", "92470")]
    r = run(base + ["--maxbytes", "3000"])  # ends inside the first packet: two fragments
    assert TOTAL.findall(r.stdout) == [("1", "2", "3028")]


def test_verbose_line_prints_ports_0_for_later_fragments():
    args = JUMBO + ["--maxpckts", "5", "--delay", "0", "--seed", "5", "--threads", "1", "--fragment", "1500", "-v"]
    lines = SENT.findall(run(args).stdout)
    assert len(lines) == 35
    for i, (n, _, sport, dst, dport) in enumerate(lines):
        first = i % 7 == 0
        assert n == ("163" if i % 7 == 6 else "1514") and dst == pc.DIP
        assert dport == "27015" if first else (sport, dport) == ("0", "0")
