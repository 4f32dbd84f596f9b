"""pcktbatch-gpu --segment on the GPU: what --pcapdump writes and what the loopback TX path sends are
tests/pyseg.py applied to the frames of the same run without --segment (same arguments, seed, MACs
and --pcapt0); the options beside it, quotas and totals."""
import os
import re
import subprocess

import pytest

import pb_configs as pc
import pyencap
import pyfrag
import pypcap
import pyseg
import pyxlat
from pbgpu import parse_mac

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pb-af-xdp_amd", "bin", "pcktbatch-gpu")
T0 = 1_700_000_000_000_000_000
COMMON = ["-z", "--interface", "pbnodev0", "--smac", pc.SMAC, "--dmac", pc.DMAC, "--dip", pc.DIP, "--sip",
          "10.20.0.0/16"]
UDP = COMMON + ["--protocol", "udp", "--udport", "27015", "--pmin", "9001", "--pmax", "9001"]  # 9043-B frames
TCP = COMMON + ["--protocol", "tcp", "--tdport", "80", "--ack", "1", "--psh", "1", "--fin", "1", "--cwr", "1", "--pmin",
                "9001", "--pmax", "9001"]  # 9055-B frames
PROTO = {"udp": UDP, "tcp": TCP}
TOTAL = re.compile(r"^\[(\d+)\] Completed sequence with a total of (\d+) packets and (\d+) bytes\.", re.M)
SEGS = re.compile(r"^\[(\d+)\] Segmented into (\d+) frames\.$", re.M)
SRC6 = "64:ff9b::/96"
VXSPEC = "vxlan:5000:192.0.2.1:198.51.100.2"


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


def seg_all(frames, mss, flags=0):
    return [x for f in frames for x in pyseg.segment(f, mss, flags)]


@pytest.mark.parametrize("proto", ["udp", "tcp"])
def test_pcapdump_with_segment(tmp_path, proto):
    """300 packets in batches of 64 (five, the last partial) at 1 Mpps: the capture holds pyseg's
    segments of the run without --segment, stamped by their own index."""
    args = PROTO[proto] + ["--pps", "1000000", "--maxpckts", "300", "--gpubatch", "64", "--seed", "7"]
    _, plain = dump(tmp_path, args, "plain.pcap")
    frames = frames_of(plain)
    assert len(frames) == 300 and all(len(f) == (9043 if proto == "udp" else 9055) for f in frames)
    r, got = dump(tmp_path, args + ["--segment", "1460"], "seg.pcap")
    want = seg_all(frames, 1460)
    assert len(want) == 2100
    assert got == pypcap.pcap_stream(want, T0, 10**6, 0, True, False)
    pyseg.check_all(frames, frames_of(got), 1460)
    assert TOTAL.findall(r.stdout) == [("1", "300", str(sum(len(f) for f in want)))]
    assert SEGS.findall(r.stdout) == [("1", "2100")]
    # :fixedid keeps the packet's ID in every segment
    _, got = dump(tmp_path, args + ["--segment", "1460:fixedid"], "fid.pcap")
    assert frames_of(got) == seg_all(frames, 1460, pyseg.FIXED_ID)


@pytest.mark.parametrize("proto", ["udp", "tcp"])
def test_jumbo_frames_send_in_2k_slots_only_with_segment(tmp_path, proto):
    """9-KB frames do not fit 2-KiB UMEM slots: refused without --segment; with --segment 1460 the
    loopback TX path sends pyseg's segments of them, in order, and the totals count what was sent."""
    args = PROTO[proto] + ["--maxpckts", "200", "--delay", "0", "--gpubatch", "64", "--seed", "4242", "--threads", "1",
                           "--track", "1", "--umemslot", "2048"]
    none = tmp_path / "none.pcap"
    r = subprocess.run([BIN] + args + ["--pcap", str(none)], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "Error landing frames" in r.stderr
    assert pypcap.read_pcap(none.read_bytes())[1] == []
    _, plain = dump(tmp_path, args, "plain.pcap")
    frames = frames_of(plain)
    assert len(frames) == 200
    sent = tmp_path / "sent.pcap"
    r = run(args + ["--segment", "1460", "--pcap", str(sent)])
    want = seg_all(frames, 1460)
    assert frames_of(sent.read_bytes()) == want
    assert TOTAL.findall(r.stdout) == [("1", "1400", str(sum(len(f) for f in want)))]


@pytest.mark.parametrize("proto", ["udp", "tcp"])
def test_verify_and_verifywire_beside_segment(tmp_path, proto):
    args = PROTO[proto] + ["--maxpckts", "500", "--delay", "0", "--gpubatch", "128", "--seed", "11", "--verify",
                           "--verifywire", "--segment", "1460"]
    for r in (run(args + ["--threads", "1", "--umemslot", "2048"]), dump(tmp_path, args, "v.pcap")[0]):
        assert "Verified 500 frames on the GPU: 0 bad." in r.stdout
        assert r.stdout.splitlines()[-1].startswith(
            "Verified 3500 frames as sent on the GPU: 0 bad (3500 IPv4, 0 IPv6, 0 with an inner frame, 0 without"), r.stdout


@pytest.mark.parametrize("proto", ["udp", "tcp"])
def test_stamp_head_lands_in_segment_0_only(tmp_path, proto):
    """One batch, so that both runs stamp packet j with index j (a later batch's first index is the
    frames packed before it, segments here as fragments under --fragment)."""
    args = PROTO[proto] + ["--pps", "1000000", "--maxpckts", "100", "--gpubatch", "128", "--seed", "5", "--stamp", "head"]
    _, stamped = dump(tmp_path, args, "stamped.pcap")
    frames = frames_of(stamped)
    _, plain = dump(tmp_path, [a for a in args if a not in ("--stamp", "head")], "plain.pcap")
    assert frames != frames_of(plain)
    _, got = dump(tmp_path, args + ["--segment", "1460"], "ss.pcap")
    out = frames_of(got)
    assert out == seg_all(frames, 1460)
    pyseg.check_all(frames, out, 1460)
    unstamped = seg_all(frames_of(plain), 1460)
    hl = 42 if proto == "udp" else 54
    for i, (a, b) in enumerate(zip(out, unstamped)):
        assert (a[hl:] != b[hl:]) == (i % 7 == 0)  # the payload differs in each packet's first segment alone


def test_fragment_xlat6_and_encap_take_the_segments(tmp_path):
    args = TCP + ["--pps", "1000000", "--maxpckts", "100", "--gpubatch", "32", "--seed", "7"]
    _, plain = dump(tmp_path, args, "plain.pcap")
    segs = seg_all(frames_of(plain), 1460)
    # --fragment 576: every 1514-B segment in three pieces (built frames carry no DF)
    r, got = dump(tmp_path, args + ["--segment", "1460", "--fragment", "576", "--verify"], "sf.pcap")
    want = [x for s in segs for x in pyfrag.fragment(s, 576)]
    assert frames_of(got) == want and len(want) > 2 * len(segs)
    assert TOTAL.findall(r.stdout) == [("1", "100", str(sum(len(f) for f in want)))]
    # --xlat6
    _, got = dump(tmp_path, args + ["--segment", "1460", "--xlat6", SRC6, "--verifywire"], "sx.pcap")
    want = pyxlat.xlat_all(segs, pyxlat.prefix96(SRC6))
    assert frames_of(got) == want and all(pyxlat.check6(g) for g in want)
    # --encap vxlan, through --pcapdump and through the loopback TX path
    want = [pyencap.vxlan(f, dst_mac=parse_mac(pc.DMAC), src_mac=parse_mac(pc.SMAC), src_ip=bytes([192, 0, 2, 1]),
                          dst_ip=bytes([198, 51, 100, 2]), vni=5000) for f in segs]
    r, got = dump(tmp_path, args + ["--segment", "1460", "--encap", VXSPEC, "--verifywire"], "se.pcap")
    assert frames_of(got) == want
    assert TOTAL.findall(r.stdout) == [("1", "100", str(sum(len(f) for f in want)))]
    sent = tmp_path / "sent.pcap"
    r = run(args + ["--segment", "1460", "--encap", VXSPEC, "--pcap", str(sent), "--delay", "0", "--threads", "1",
                    "--track", "1", "--umemslot", "2048"])
    assert frames_of(sent.read_bytes()) == want
    assert TOTAL.findall(r.stdout) == [("1", "700", str(sum(len(f) for f in want)))]
    # all of them at once on the TX path: segments, fragmented, then encapsulated
    sent2 = tmp_path / "sent2.pcap"
    run(args + ["--segment", "1460", "--fragment", "576", "--encap", VXSPEC, "--pcap", str(sent2), "--delay", "0",
                "--threads", "1", "--track", "1", "--umemslot", "1024"])
    want = [pyencap.vxlan(x, dst_mac=parse_mac(pc.DMAC), src_mac=parse_mac(pc.SMAC), src_ip=bytes([192, 0, 2, 1]),
                          dst_ip=bytes([198, 51, 100, 2]), vni=5000) for s in segs for x in pyfrag.fragment(s, 576)]
    assert frames_of(sent2.read_bytes()) == want


@pytest.mark.parametrize("proto", ["udp", "tcp"])
def test_l4csum_0_keeps_the_source_checksum_bytes(tmp_path, proto):
    args = PROTO[proto] + ["--pps", "1000000", "--maxpckts", "50", "--gpubatch", "32", "--seed", "9", "--l4csum", "0"]
    _, plain = dump(tmp_path, args, "plain.pcap")
    frames = frames_of(plain)
    _, got = dump(tmp_path, args + ["--segment", "1460", "--verify", "--verifywire"], "nc.pcap")
    out = frames_of(got)
    assert out == seg_all(frames, 1460, pyseg.NO_L4_CSUM)
    at = 40 if proto == "udp" else 50
    assert all(out[7 * j + i][at:at + 2] == frames[j][at:at + 2] for j in range(50) for i in range(7))


def test_maxpckts_counts_packets_and_maxbytes_counts_sent_bytes():
    """--maxpckts 10 builds 10 packets (70 frames on the ring); --maxbytes 92950 is 10 packets' segments."""
    base = UDP + ["--delay", "0", "--seed", "3", "--threads", "1", "--gpubatch", "8", "--track", "1", "--segment", "1472",
                  "--umemslot", "2048"]
    per = 9043 + 6 * 42
    r = run(base + ["--maxpckts", "10"])
    assert TOTAL.findall(r.stdout) == [("1", "70", str(10 * per))]
    r = run(base + ["--maxbytes", str(10 * per)])
    assert TOTAL.findall(r.stdout) == [("1", "70", str(10 * per))]
    r = run(base + ["--maxbytes", "3000"])  # ends inside the first packet: two segments
    assert TOTAL.findall(r.stdout) == [("1", "2", "3028")]
