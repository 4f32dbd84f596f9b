"""pcktbatch-gpu --stamp on the GPU: the dumped capture equals tests/pystamp.py over the oracle's
frames and scripts/stamp_read.py finds every index once and on time; the loopback TX path with two
threads stamps disjoint, whole batches; --stamp twice and a malformed position are refused."""
import json
import os
import subprocess
import sys

import pytest

import oracle_binding as ob
import pb_configs as pc
import pypcap
import pystamp
from pbgpu import Sequence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pb-af-xdp_amd", "bin", "pcktbatch-gpu")
READER = os.path.join(ROOT, "scripts", "stamp_read.py")
T0 = 1_700_000_000_000_000_000
COMMON = ["-z", "--interface", "pbnodev0", "--smac", pc.SMAC, "--dmac", pc.DMAC, "--dip", pc.DIP, "--sip",
          "10.20.0.0/16", "--protocol", "udp", "--udport", "27015"]


def read_back(path, spec):
    r = subprocess.run([sys.executable, READER, str(path), spec], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


@pytest.mark.parametrize("spec,tail,offset,pmin,pmax", [("head", False, 0, 22, 22), ("tail:3", True, 3, 40, 300),
                                                        ("head:5", False, 5, 0, 60)])
def test_dump_stamped_verified_and_read_back(tmp_path, spec, tail, offset, pmin, pmax):
    """1000 frames in batches of 256 at 1 Mpps: the stamp takes the pack's t0, step and first index, so
    the reader sees indices 0..999, nothing missing and every record on its stamp's time; frames too
    short for the stamp (pmin 0) stay as the oracle built them."""
    out = tmp_path / "s.pcap"
    n, pps = 1000, 1_000_000
    r = subprocess.run([BIN] + COMMON + ["--pmin", str(pmin), "--pmax", str(pmax), "--pps", str(pps), "--maxpckts", str(n),
                                         "--gpubatch", "256", "--seed", "7", "--stamp", spec, "--verify", "--pcapdump",
                                         str(out), "--pcapt0", str(T0)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines()[-1] == "Verified 1000 frames on the GPU: 0 bad."
    cfg = pc.c2_udp_64()
    cfg["payloads"] = [{"length": {"min": pmin, "max": pmax}}]
    frames = ob.frames(Sequence.from_config(cfg), 0, 0, n, 7)
    step = 10**12 // pps
    refs = [pystamp.stamp(f, j, pystamp.stamp_time(j, T0, step), offset, tail) for j, f in enumerate(frames)]
    assert out.read_bytes() == pypcap.pcap_stream([f for f, _ in refs], T0, step, 0, True, False)
    stamped = [j for j, (_, cls) in enumerate(refs) if cls == "stamped"]
    got = read_back(out, spec)
    assert got["frames"] == n and got["stamped"] == len(stamped) > 0
    assert (got["min_index"], got["max_index"]) == (stamped[0], stamped[-1])
    assert got["missing"] == (stamped[-1] - stamped[0] + 1) - len(stamped)
    assert (got["duplicates"], got["out_of_order"]) == (0, 0)
    assert (got["delta_ns_min"], got["delta_ns_median"], got["delta_ns_max"]) == (0, 0.0, 0)
    if pmin >= 22:
        assert len(stamped) == n and got["missing"] == 0 and (got["min_index"], got["max_index"]) == (0, n - 1)


def test_loopback_tx_two_threads(tmp_path):
    """--threads 2 through the loopback ring into --pcap: thread t's batch `step` carries the indices
    from (step * 2 + t) * 1000 on, so no two frames share one, every batch that was sent is there whole,
    and t0 is --pcapt0 although nothing is dumped.  Which thread claims how many of the six batches is
    the threads' race: the indices lie in [0, 12000)."""
    pcap = tmp_path / "t2.pcap"
    pps = 2_000_000_000
    cmd = [BIN] + COMMON + ["--pmin", "22", "--pmax", "22", "--maxpckts", "6000", "--delay", "0", "--threads", "2",
                            "--gpubatch", "1000", "--seed", "4242", "--stamp", "head:2", "--pcapt0", str(T0), "--pps",
                            str(pps), "--verify", "--pcap", str(pcap)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    _, recs = pypcap.read_pcap(pcap.read_bytes())
    assert len(recs) == 6000
    universe = ob.frames(Sequence.from_config(pc.c2_udp_64()), 0, 0, 12000, 4242)
    step = 10**12 // pps
    seen = set()
    for _, _, f in recs:
        idx = int.from_bytes(f[44:52], "big")
        assert idx < 12000 and idx not in seen
        seen.add(idx)
        assert f == pystamp.stamp(universe[idx], idx, pystamp.stamp_time(idx, T0, step), 2, False)[0]
    blocks = {i // 1000 for i in seen}
    assert len(blocks) == 6 and all(b * 1000 + k in seen for b in blocks for k in range(1000))
    got = read_back(pcap, "head:2")
    assert (got["frames"], got["stamped"], got["duplicates"]) == (6000, 6000, 0)
    assert got["missing"] == got["max_index"] - got["min_index"] + 1 - 6000


def test_stamp_twice_is_refused(tmp_path):
    out = tmp_path / "o.pcap"
    r = subprocess.run([BIN] + COMMON + ["--maxpckts", "10", "--stamp", "head", "--stamp", "tail", "--pcapdump", str(out)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--stamp given more than once" in r.stderr and not out.exists()


@pytest.mark.parametrize("spec", ["middle", "head:65536", "tail:x"])
def test_bad_position_is_refused(tmp_path, spec):
    out = tmp_path / "o.pcap"
    r = subprocess.run([BIN] + COMMON + ["--maxpckts", "10", "--stamp", spec, "--pcapdump", str(out)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--stamp " + spec in r.stderr and not out.exists()
