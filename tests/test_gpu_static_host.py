"""pcktbatch-gpu with a payload file (--pexact FILE --pfile 1 [--pstring 1], JSON "isfile") on the
GPU: the --pcapdump stream equals tests/pypcap.py over the oracle's frames, for a hex file with
line breaks and for a string file, UDP and TCP.  The oracle reads the same file by its own
load_exact, which tests/test_static_payload_cpu.py holds against pyspec and host libc."""
import json
import os
import subprocess

import pytest

import oracle_binding as ob
import pb_configs as pc
import pypcap
import static_cases as sc
from pbgpu import Sequence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pb-af-xdp_amd", "bin", "pcktbatch-gpu")
T0 = 1_700_000_000_000_000_000
N = 1000
DATA = bytes(b or 0x55 for b in sc.pattern("ramp", 1400))  # a string holds no NUL
L4 = {"udp": (["--udport", "27015"], {"udp": {"dport": 27015}}),
      "tcp": (["--tdport", "80", "--psh", "1", "--ack", "1"], {"tcp": {"dport": 80, "psh": 1, "ack": 1}})}
ENV = dict(os.environ, PB_SEQ_GAP_MS="0")  # no pause after a sequence


def payload_file(tmp_path, source):
    """The 1400 bytes as a hex file (16 tokens per line, LF and CRLF breaks, a space after each so
    that no token is lost) or verbatim; returns the payload's config entry."""
    if source == "hex":
        toks = ["%02x" % b for b in DATA]
        path = tmp_path / "payload.hex"
        path.write_text("".join(" ".join(toks[i:i + 16]) + ("\n " if i % 32 else "\r\n ") for i in range(0, len(toks), 16)))
        return {"exact": str(path), "isfile": 1}
    path = tmp_path / "payload.bin"
    path.write_bytes(DATA)
    return {"exact": str(path), "isfile": 1, "isstring": 1}


def seq_cfg(proto, payload):
    cfg = {"eth": {"smac": pc.SMAC, "dmac": pc.DMAC}, "ip": {"dip": pc.DIP, "ranges": ["10.20.0.0/16"], "protocol": proto},
           "payloads": [payload]}
    cfg.update(L4[proto][1])
    return cfg


def want_stream(cfgs, seed):
    out = b""
    for i, cfg in enumerate(cfgs):
        frames = ob.frames(Sequence.from_config(cfg), i, 0, N, seed)
        hl = sc.HL[cfg["ip"]["protocol"]]
        assert len(frames) == N and all(f[hl:] == DATA for f in frames)
        out += pypcap.pcap_stream(frames, T0, 0, 0, i == 0, False)
    return out


@pytest.mark.parametrize("source", ["hex", "string"])
@pytest.mark.parametrize("proto", ["udp", "tcp"])
def test_cli_payload_file_equals_oracle(tmp_path, proto, source):
    pl = payload_file(tmp_path, source)
    out = tmp_path / "out.pcap"
    cmd = [BIN, "-z", "--interface", "pbnodev0", "--smac", pc.SMAC, "--dmac", pc.DMAC, "--dip", pc.DIP, "--sip",
           "10.20.0.0/16", "--protocol", proto] + L4[proto][0] + ["--pexact", pl["exact"], "--pfile", "1"] + (
           ["--pstring", "1"] if source == "string" else []) + [
           "--maxpckts", str(N), "--delay", "0", "--gpubatch", "256", "--seed", "77", "--pcapdump", str(out),
           "--pcapt0", str(T0)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stderr
    assert "total of %d packets and %d bytes" % (N, N * (sc.HL[proto] + 1400)) in r.stdout
    assert out.read_bytes() == want_stream([seq_cfg(proto, pl)], 77)


@pytest.mark.parametrize("proto", ["udp", "tcp"])
def test_json_isfile_equals_oracle(tmp_path, proto):
    """Two sequences, the hex file and the string file, "isfile": true as the README writes it."""
    cfgs = []
    for source in ("hex", "string"):
        c = seq_cfg(proto, {k: (v if k == "exact" else True) for k, v in payload_file(tmp_path, source).items()})
        c.update({"maxpckts": N, "delay": 0, "block": 1})
        cfgs.append(c)
    path = tmp_path / "conf.json"
    path.write_text(json.dumps({"interface": "pbnodev0", "sequences": cfgs}))
    out = tmp_path / "out.pcap"
    r = subprocess.run([BIN, "-c", str(path), "--gpubatch", "256", "--seed", "78", "--pcapdump", str(out), "--pcapt0",
                        str(T0)], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stderr
    assert "Completed 2 sequences!" in r.stdout
    assert out.read_bytes() == want_stream(cfgs, 78)
