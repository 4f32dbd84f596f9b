"""pcktbatch-gpu --pcapdump on the GPU: the file equals tests/pypcap.py over the oracle's frames
with the timestamp rule (frame j of a sequence at t0 + floor(j * 10^12 / pps / 1000) ns), batch
after batch, sequence after sequence; and its frames are the ones the --pcap run records."""
import json
import os
import re
import subprocess

import pytest

import oracle_binding as ob
import pb_configs as pc
import pypcap
from pbgpu import Sequence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pb-af-xdp_amd", "bin", "pcktbatch-gpu")
T0 = 1_700_000_000_000_000_000
COMMON = ["-z", "--interface", "pbnodev0", "--smac", pc.SMAC, "--dmac", pc.DMAC, "--dip", pc.DIP, "--sip",
          "10.20.0.0/16", "--protocol", "udp", "--udport", "27015"]
TOTAL = re.compile(r"^\[(\d+)\] Completed sequence with a total of (\d+) packets and (\d+) bytes\.", re.M)


def dump(tmp_path, args, name="out.pcap"):
    out = tmp_path / name
    r = subprocess.run([BIN] + args + ["--pcapdump", str(out), "--pcapt0", str(T0)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    return r, out.read_bytes()


def udp_cfg(pmin, pmax):
    cfg = pc.c2_udp_64()  # what COMMON gives
    cfg["payloads"] = [{"length": {"min": pmin, "max": pmax}}]
    return cfg


@pytest.mark.parametrize("verify", [False, True])
@pytest.mark.parametrize("pmin,pmax", [(22, 22), (0, 900)])
def test_cli_dump_equals_reference(tmp_path, pmin, pmax, verify):
    """1000 frames in batches of 256 (four, the last partial) at 1 Mpps: 10^6 ps apart."""
    args = COMMON + ["--pmin", str(pmin), "--pmax", str(pmax), "--pps", "1000000", "--maxpckts", "1000", "--gpubatch",
                     "256", "--seed", "7"] + (["--verify"] if verify else [])
    r, got = dump(tmp_path, args)
    frames = ob.frames(Sequence.from_config(udp_cfg(pmin, pmax)), 0, 0, 1000, 7)
    assert got == pypcap.pcap_stream(frames, T0, 10**6, 0, True, False)
    assert "Completed 1 sequences!" in r.stdout
    assert TOTAL.findall(r.stdout) == [("1", "1000", str(sum(len(f) for f in frames)))]
    if verify:
        assert r.stdout.splitlines()[-1] == "Verified 1000 frames on the GPU: 0 bad."
    else:
        assert "Verified" not in r.stdout


def test_cli_dump_two_sequences(tmp_path):
    """UDP then TCP SYN from a JSON config: the second sequence's records follow the first's, its
    index restarts at 0 and its t0 is the first's t0 + floor(N * step / 1000)."""
    seqs = []
    for name, n, pps in (("c2_udp_64", 700, 3_000_000), ("c4_tcp_syn", 500, 0)):
        c = dict(pc.get(name))
        c.update({"maxpckts": n, "delay": 0, "block": 1, "pps": pps})
        seqs.append(c)
    path = tmp_path / "conf.json"
    path.write_text(json.dumps({"interface": "pbnodev0", "sequences": seqs}))
    out = tmp_path / "two.pcap"
    r = subprocess.run([BIN, "-c", str(path), "--gpubatch", "256", "--seed", "99", "--pcapdump", str(out), "--pcapt0",
                        str(T0)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    f0 = ob.frames(Sequence.from_config(seqs[0]), 0, 0, 700, 99)
    f1 = ob.frames(Sequence.from_config(seqs[1]), 1, 0, 500, 99)
    step0 = 10**12 // 3_000_000  # 333333 ps
    t1 = T0 + (700 * step0) // 1000
    want = pypcap.pcap_stream(f0, T0, step0, 0, True, False) + pypcap.pcap_stream(f1, t1, 0, 0, False, False)
    assert out.read_bytes() == want
    assert "Completed 2 sequences!" in r.stdout
    assert TOTAL.findall(r.stdout) == [("1", "700", str(64 * 700)), ("2", "500", str(60 * 500))]


def test_cli_dump_frames_equal_the_pcap_run(tmp_path):
    """The same arguments through the existing --pcap path (one thread): the same frames in the
    same order; the timestamps are each path's own."""
    args = COMMON + ["--pmin", "0", "--pmax", "300", "--maxpckts", "3000", "--delay", "0", "--gpubatch", "1000",
                     "--seed", "4242", "--threads", "1"]
    _, got = dump(tmp_path, args)
    ref = tmp_path / "ref.pcap"
    r = subprocess.run([BIN] + args + ["--pcap", str(ref)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    a = [f for _, _, f in pypcap.read_pcap(got)[1]]
    b = [f for _, _, f in pypcap.read_pcap(ref.read_bytes())[1]]
    assert len(a) == 3000 and a == b
    # no pps: every frame of the dump at t0
    assert all((s, u) == (T0 // 10**9, 0) for s, u, _ in pypcap.read_pcap(got)[1])
