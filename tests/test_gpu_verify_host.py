"""pcktbatch-gpu --verify on the GPU: every built batch is checked on the device before it lands;
the run ends with the verified count, and sends exactly what a run without --verify sends."""
import os
import subprocess

import pytest

import pb_configs as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pb-af-xdp_amd", "bin", "pcktbatch-gpu")

CASES = {
    "udp64": ["--protocol", "udp", "--udport", "27015", "--pmin", "22", "--pmax", "22"],
    "tcp_syn": ["--protocol", "tcp", "--tdport", "80", "--syn", "1", "--pmin", "6", "--pmax", "6"],
    "icmp": ["--protocol", "icmp", "--pmin", "56", "--pmax", "56"],
    "udp64_no_l4csum": ["--protocol", "udp", "--udport", "27015", "--pmin", "22", "--pmax", "22", "--l4csum", "0"],
}


def run(tmp_path, args, name, verify):
    pcap = tmp_path / name
    cmd = [BIN, "-z", "--interface", "pbnodev0", "--smac", pc.SMAC, "--dmac", pc.DMAC, "--dip", pc.DIP,
           "--sip", "10.20.0.0/16"] + args + ["--maxpckts", "100000", "--delay", "0", "--gpubatch", "32768",
                                              "--seed", "4242", "--track", "1", "--pcap", str(pcap)]
    r = subprocess.run(cmd + (["--verify"] if verify else []), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r, pcap.read_bytes()


def frames_of(pcap):
    """The capture's frames without their timestamps."""
    out, pos = [], 24
    while pos < len(pcap):
        incl = int.from_bytes(pcap[pos + 8:pos + 12], "little")
        out.append(pcap[pos + 16:pos + 16 + incl])
        pos += 16 + incl
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_verify_flag(tmp_path, case):
    plain, cap0 = run(tmp_path, CASES[case], "plain.pcap", False)
    ver, cap1 = run(tmp_path, CASES[case], "verify.pcap", True)
    line = "Verified 100000 frames on the GPU: 0 bad."
    lines = ver.stdout.splitlines()
    assert line in lines and "Verified" not in plain.stdout
    # one extra line, after the reference's (the average-rate line depends on the run's seconds)
    assert lines[-1] == line and len(lines) == len(plain.stdout.splitlines()) + 1
    assert "total of 100000 packets" in ver.stdout
    assert ver.stderr == plain.stderr
    f0, f1 = frames_of(cap0), frames_of(cap1)
    assert len(f0) == 100000 and f0 == f1
