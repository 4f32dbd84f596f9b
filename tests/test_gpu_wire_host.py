"""pcktbatch-gpu --verifywire on the GPU, through --pcapdump and through the loopback TX path: beside
every repack the run exits 0, prints the new line with the counts the capture's own frames give
under tests/pywire.py, and writes byte for byte the capture it writes without the option; without
the option nothing of the output changes."""
import os
import re
import subprocess

import pytest

import pb_configs as pc
import pypcap
import pywire as pw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pb-af-xdp_amd", "bin", "pcktbatch-gpu")
T0 = 1_700_000_000_000_000_000
COMMON = ["-z", "--interface", "pbnodev0", "--smac", pc.SMAC, "--dmac", pc.DMAC, "--dip", pc.DIP, "--sip",
          "10.20.0.0/16", "--protocol", "udp", "--udport", "27015", "--seed", "7", "--pps", "1000000"]
LINE = re.compile(r"^Verified (\d+) frames as sent on the GPU: (\d+) bad \((\d+) IPv4, (\d+) IPv6, (\d+) with an inner "
                  r"frame, (\d+) without an L4 checksum to check, (\d+) not IP\)\.$")
VXLAN = "vxlan:5000:192.0.2.1:198.51.100.2"
SMALL = ["--pmin", "0", "--pmax", "900", "--maxpckts", "1000", "--gpubatch", "256"]
JUMBO = ["--pmin", "9001", "--pmax", "9001", "--maxpckts", "100", "--gpubatch", "32"]
# name: (arguments, VXLAN port for the reference)
COMBOS = {
    "alone": (SMALL, 0),
    "vlan": (SMALL + ["--encap", "vlan:100"], 0),
    "vxlan": (SMALL + ["--encap", VXLAN], 4789),
    "vxlan-port": (SMALL + ["--encap", VXLAN + ":4790"], 4790),
    "xlat6": (SMALL + ["--xlat6", "2001:db8:ffff:ffff:ffff:ffff::/96"], 0),
    "xlat6-vxlan": (SMALL + ["--xlat6", "64:ff9b::/96", "--encap", VXLAN], 4789),
    "fragment": (JUMBO + ["--fragment", "1500"], 0),
    "stamp-verify": (SMALL + ["--stamp", "head", "--verify"], 0),
    "no-l4csum": (SMALL + ["--l4csum", "0"], 0),
}


def run(args):
    r = subprocess.run([BIN] + COMMON + args, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PB_SEQ_GAP_MS="10"))  # the second's pause after a sequence is not the subject
    assert r.returncode == 0, r.stderr
    return r


def stable(stdout):
    """The lines that do not hold a duration."""
    return [x for x in stdout.splitlines() if "Total seconds" not in x]


def expected_line(frames, port):
    _, r = pw.result(frames, pw.ALL, port)
    assert r["n_bad"] == 0
    return ("Verified %d frames as sent on the GPU: 0 bad (%d IPv4, %d IPv6, %d with an inner frame, %d without an L4 "
            "checksum to check, %d not IP)." % (len(frames), r["n_ipv4"], r["n_ipv6"], r["n_inner"], r["n_nol4"], r["n_other"]))


@pytest.mark.parametrize("path", ["pcapdump", "tx"])
@pytest.mark.parametrize("name", list(COMBOS))
def test_verifywire_beside(tmp_path, name, path):
    args, port = COMBOS[name]
    if path == "pcapdump":
        tail = lambda f: ["--pcapdump", str(f), "--pcapt0", str(T0)]
    else:
        tail = lambda f: ["--pcap", str(f), "--delay", "0", "--threads", "1", "--track", "1", "--pcapt0", str(T0)]
    plain_file, wire_file = tmp_path / "plain.pcap", tmp_path / "wire.pcap"
    plain = run(args + tail(plain_file))
    wire = run(args + ["--verifywire"] + tail(wire_file))
    frames = [f for _, _, f in pypcap.read_pcap(wire_file.read_bytes())[1]]
    assert len(frames) >= 100
    if path == "pcapdump":
        assert wire_file.read_bytes() == plain_file.read_bytes()
    else:  # the TX hook stamps the wall clock: the frames and their order are the run's
        assert frames == [f for _, _, f in pypcap.read_pcap(plain_file.read_bytes())[1]]
    # without the option no line of the output changes; with it there is one more
    got = [x for x in wire.stdout.splitlines() if LINE.match(x)]
    assert len(got) == 1 and not any("as sent" in x for x in plain.stdout.splitlines())
    assert [x for x in stable(wire.stdout) if x != got[0]] == stable(plain.stdout)
    assert wire.stderr == plain.stderr
    assert got[0] == expected_line(frames, port)
    m = [int(x) for x in LINE.match(got[0]).groups()]
    if name in ("vxlan", "vxlan-port", "xlat6-vxlan"):
        assert m[4] == len(frames)
    if name == "xlat6":
        assert m[3] == len(frames) and m[2] == 0
    if name == "xlat6-vxlan":  # counted by the outermost L3
        assert m[2] == len(frames) and m[3] == 0
    if name == "fragment":
        assert m[0] == 700 and m[5] == 700
    if name == "no-l4csum":
        assert m[5] == len(frames)  # UDP over IPv4 with 00 00: nothing to evaluate, and no failure
    if name == "stamp-verify":
        assert "Verified 1000 frames on the GPU: 0 bad." in wire.stdout.splitlines()
