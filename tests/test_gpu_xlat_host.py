"""pcktbatch-gpu --xlat6 on the GPU: what --pcapdump writes and what the loopback TX path sends are
tests/pyxlat.py applied to the oracle's frames for the same arguments and seed; beside --stamp,
--verify and --encap; the totals count the translated bytes; a UMEM slot that just fits, and one
that does not."""
import os
import re
import subprocess

import pytest

import oracle_binding as ob
import pb_configs as pc
import pyencap
import pypcap
import pystamp
import pyxlat
from pbgpu import Sequence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pb-af-xdp_amd", "bin", "pcktbatch-gpu")
T0 = 1_700_000_000_000_000_000
COMMON = ["-z", "--interface", "pbnodev0", "--smac", pc.SMAC, "--dmac", pc.DMAC, "--dip", pc.DIP, "--sip",
          "10.20.0.0/16", "--protocol", "udp", "--udport", "27015"]
TOTAL = re.compile(r"^\[(\d+)\] Completed sequence with a total of (\d+) packets and (\d+) bytes\.", re.M)
SENT = re.compile(r"^\[1\]\[1\] Sent (\d+) bytes of data from (\S+) to (\S+)\.$", re.M)
SRC6, DST6 = "2001:db8:ffff:ffff:ffff:ffff::/96", "64:ff9b::/96"


def udp_frames(pmin, pmax, n, seed):
    cfg = pc.c2_udp_64()  # what COMMON gives
    cfg["payloads"] = [{"length": {"min": pmin, "max": pmax}}]
    return ob.frames(Sequence.from_config(cfg), 0, 0, n, seed)


def run(args, ok=True):
    r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr
    return r


def dump(tmp_path, args, name="out.pcap"):
    out = tmp_path / name
    r = run(args + ["--pcapdump", str(out), "--pcapt0", str(T0)])
    return r, out.read_bytes()


@pytest.mark.parametrize("spec,kw", [
    (SRC6, dict(src_prefix=pyxlat.prefix96(SRC6))),
    (SRC6 + "," + DST6, dict(src_prefix=pyxlat.prefix96(SRC6), dst_prefix=pyxlat.prefix96(DST6))),
    (DST6 + ":hashflow", dict(src_prefix=pyxlat.prefix96(DST6), hash_flow=True)),
], ids=["one", "two", "hashflow"])
@pytest.mark.parametrize("pmin,pmax", [(22, 22), (0, 900)])
def test_pcapdump_with_xlat6(tmp_path, pmin, pmax, spec, kw):
    """1000 frames in batches of 256 (four, the last partial) at 1 Mpps."""
    args = COMMON + ["--pmin", str(pmin), "--pmax", str(pmax), "--pps", "1000000", "--maxpckts", "1000", "--gpubatch",
                     "256", "--seed", "7", "--xlat6", spec]
    r, got = dump(tmp_path, args)
    want = pyxlat.xlat_all(udp_frames(pmin, pmax, 1000, 7), **kw)
    assert all(pyxlat.check6(g) for g in want)
    assert got == pypcap.pcap_stream(want, T0, 10**6, 0, True, False)
    assert TOTAL.findall(r.stdout) == [("1", "1000", str(sum(len(f) for f in want)))]


def test_pcapdump_with_stamp_and_verify(tmp_path):
    """The stamp goes into the IPv4 frame, --verify checks it there, then the frame is translated."""
    args = COMMON + ["--pmin", "0", "--pmax", "500", "--pps", "1000000", "--maxpckts", "1000", "--gpubatch", "256",
                     "--seed", "11", "--stamp", "head", "--verify", "--xlat6", SRC6]
    r, got = dump(tmp_path, args)
    frames = udp_frames(0, 500, 1000, 11)
    stamped = [pystamp.stamp(f, j, pystamp.stamp_time(j, T0, 10**6))[0] for j, f in enumerate(frames)]
    assert stamped != frames
    want = pyxlat.xlat_all(stamped, pyxlat.prefix96(SRC6))
    assert got == pypcap.pcap_stream(want, T0, 10**6, 0, True, False)
    assert all(pyxlat.check6(g) for g in want)
    assert r.stdout.splitlines()[-1] == "Verified 1000 frames on the GPU: 0 bad."


@pytest.mark.parametrize("enc", ["vlan:100", "vxlan:5000:192.0.2.1:198.51.100.2"])
def test_pcapdump_with_encap(tmp_path, enc):
    args = COMMON + ["--pmin", "0", "--pmax", "900", "--maxpckts", "1000", "--gpubatch", "256", "--seed", "7", "--xlat6",
                     SRC6 + "," + DST6, "--encap", enc]
    r, got = dump(tmp_path, args)
    x6 = pyxlat.xlat_all(udp_frames(0, 900, 1000, 7), pyxlat.prefix96(SRC6), pyxlat.prefix96(DST6))
    if enc.startswith("vlan"):
        want = [pyencap.vlan(f, 100) for f in x6]
    else:
        from pbgpu import parse_mac
        want = [pyencap.vxlan(f, dst_mac=parse_mac(pc.DMAC), src_mac=parse_mac(pc.SMAC), src_ip=bytes([192, 0, 2, 1]),
                              dst_ip=bytes([198, 51, 100, 2]), vni=5000) for f in x6]
    assert got == pypcap.pcap_stream(want, T0, 0, 0, True, False)
    assert TOTAL.findall(r.stdout) == [("1", "1000", str(sum(len(f) for f in want)))]


def test_loopback_tx_path_slot_that_just_fits(tmp_path):
    """One TX thread through the loopback ring into --pcap.  108-B frames become 128 B: 128-B slots
    take them, and the totals count the translated bytes; 109-B frames are one byte too long for the
    slot and are refused with a message before anything is sent."""
    base = COMMON + ["--maxpckts", "3000", "--delay", "0", "--gpubatch", "1000", "--seed", "4242", "--threads", "1",
                     "--track", "1", "--umemslot", "128", "--xlat6", SRC6]
    out = tmp_path / "x6.pcap"
    r = run(base + ["--pmin", "66", "--pmax", "66", "--pcap", str(out)])
    want = pyxlat.xlat_all(udp_frames(66, 66, 3000, 4242), pyxlat.prefix96(SRC6))
    assert {len(f) for f in want} == {128}
    assert [f for _, _, f in pypcap.read_pcap(out.read_bytes())[1]] == want
    assert TOTAL.findall(r.stdout) == [("1", "3000", str(128 * 3000))]
    none = tmp_path / "none.pcap"
    r = run(base + ["--pmin", "67", "--pmax", "67", "--pcap", str(none)], ok=False)
    assert r.returncode != 0 and "--xlat6" in r.stderr and "128-B UMEM slot" in r.stderr
    assert pypcap.read_pcap(none.read_bytes())[1] == []
    # and with a tag the 108-B frames are 132 B
    r = run(base + ["--pmin", "66", "--pmax", "66", "--encap", "vlan:5", "--pcap", str(none)], ok=False)
    assert r.returncode != 0 and "128-B UMEM slot" in r.stderr
    assert pypcap.read_pcap(none.read_bytes())[1] == []


def test_verbose_line_reports_the_ipv6_addresses():
    args = COMMON + ["--pmin", "22", "--pmax", "22", "--maxpckts", "50", "--delay", "0", "--seed", "5", "--threads", "1",
                     "-v", "--xlat6", DST6]
    sent = SENT.findall(run(args).stdout)
    frames = udp_frames(22, 22, 50, 5)
    assert len(sent) == 50
    for (n, src, dst), f in zip(sent, frames):
        assert n == "84" and dst == "64:ff9b::a3c:c3:27015"
        assert src == "64:ff9b::a14:%x:%d" % (f[28] << 8 | f[29], f[34] << 8 | f[35])
