"""The static payload's text rules (sequence.c:264-361), CPU only.

1. Hex tokens: tests/pyspec.py::scan_2hhx against host libc's sscanf(tok, "%2hhx", &b) from b = 0,
   the call the reference, the oracle and the library all make (authority: the reference's text,
   then libc, as rand_r is pinned in test_oracle.py).
2. Whole payloads: the C oracle and pyspec, frame for frame, for hex, string and file sources,
   line breaks, an embedded NUL, empty and missing files, bytes >= 0x80, the longest payloads
   and one byte past them (refused).
3. Static-random payloads (isstatic) at lengths from 1 B to the longest, both payload rules.
4. The GPU file's case tables name every kernel form the static paths have."""
import copy
import ctypes
import ctypes.util
import re

import pytest

import oracle_binding as ob
import pb_configs as pc
import pyspec
import static_cases as sc
from pbgpu import Sequence

N_ITER = 3
FIRST = 1001

# the issue's table, plus tokens at the width's other edges
TOKENS = [b"DE", b"de", b"D", b"DEAD", b"0G", b"G0", b"zz", b"\nBE", b"\tBE", b"EF\n", b"-1", b"+a", b"-", b"0x",
          b"0x1f", b"\n", b"\r\n",
          b"7", b"f\n", b"\r\nAb", b" \t\v\f\r\n9c", b"+", b"-f", b"+0", b"-0", b"0X", b"0xF", b"00", b"0", b"x1", b"-x",
          b"--1", b"+-1", b"1-", b"g", b"\x801", b"ff\xff", b"EF\n-1", b"zz\t7\n"]


@pytest.fixture(scope="module")
def libc():
    lib = ctypes.CDLL(ctypes.util.find_library("c"))
    lib.sscanf.restype = ctypes.c_int
    return lib


@pytest.mark.parametrize("tok", TOKENS, ids=[repr(t)[2:-1] for t in TOKENS])
def test_hex_token_equals_libc_sscanf(libc, tok):
    b = ctypes.c_ubyte(0)
    libc.sscanf(ctypes.c_char_p(tok), ctypes.c_char_p(b"%2hhx"), ctypes.byref(b))
    assert pyspec.scan_2hhx(tok) == b.value
    if b" " not in tok:  # one token: the payload is that byte
        assert pyspec.exact_bytes({"exact": tok}) == bytes([b.value])


def test_issue_example_file(tmp_path):
    """The file of the issue: line breaks inside tokens, a sign, 0x, an unparsable token."""
    path = tmp_path / "p.hex"
    path.write_bytes(b"DE AD \nBE EF\n-1 +a 0x1f  zz\t7\n")
    assert pyspec.exact_bytes({"exact": str(path), "isfile": 1}) == bytes.fromhex("deadbeef0a0000")


def _cfg(proto, payloads):
    cfg = copy.deepcopy(pc.get({"udp": "c2_udp_64", "tcp": "c4_tcp_syn", "icmp": "c5_icmp_echo"}[proto]))
    cfg["payloads"] = payloads
    return cfg


def _same(cfg, rule=0, n=N_ITER, first=FIRST):
    """Oracle (lean and faithful) == pyspec, frame for frame; returns the frames."""
    seq = Sequence.from_config(cfg)
    want = pyspec.build(cfg, 3, first, n, pc.SEED_BASE, literal=bool(rule))
    for faithful in (False, True):
        got = ob.frames(seq, 3, first, n, pc.SEED_BASE, payload_rule=rule, faithful=faithful)
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, f"frame {i} (faithful={faithful}): lengths {len(g)} / {len(w)}"
    return want


def _hex(data, sep=" "):
    return sep.join("%02x" % b for b in data)


RAMP = bytes((7 * i + 3) & 255 for i in range(1400))
HL = {"udp": 42, "tcp": 54, "icmp": 42}
LONGEST = {"udp": 65493, "tcp": 65481, "icmp": 65493}  # PB_MAX_PCKT_LEN - headers


@pytest.mark.parametrize("proto", ["udp", "tcp", "icmp"])
def test_sources_build_the_same_frames(tmp_path, proto):
    """One payload as inline hex, as a hex file and as a string file (bytes that a string can
    hold: no NUL): three sources, one set of frames."""
    data = bytes(b or 0x55 for b in RAMP)
    hexf, strf = tmp_path / "p.hex", tmp_path / "p.bin"
    hexf.write_text(_hex(data))
    strf.write_bytes(data)
    a = _same(_cfg(proto, [{"exact": _hex(data)}]))
    b = _same(_cfg(proto, [{"exact": str(hexf), "isfile": 1}]))
    c = _same(_cfg(proto, [{"exact": str(strf), "isfile": 1, "isstring": 1}]))
    assert a == b == c
    assert all(f[HL[proto]:] == data for f in a)


@pytest.mark.parametrize("brk,kind", [
    ("\n", "glued"), ("\r\n", "glued"), ("\n ", "same"), (" \n", "end0"), (" \r\n ", "each0"), (" \n\n ", "each0"),
], ids=["lf", "crlf", "lf_sp", "sp_lf", "sp_crlf_sp", "sp_lf_lf_sp"])
def test_hex_file_line_breaks(tmp_path, brk, kind):
    """16 tokens per line, the break after every line (strtok_r splits at ' ' only).  A bare break
    glues the line's last token to the next line's first, which is lost.  A space after the break
    leaves it at the end of a token, where sscanf ignores it; a space before it puts it in front
    of the next token, where sscanf skips it, but the last break then is a token of its own and
    gives a 0x00 byte, as does every break with spaces on both sides."""
    data = RAMP[:100]
    toks = ["%02X" % b for b in data]
    lines = [" ".join(toks[i:i + 16]) for i in range(0, len(toks), 16)]
    path = tmp_path / "p.hex"
    path.write_text(brk.join(lines) + brk)
    frames = _same(_cfg("udp", [{"exact": str(path), "isfile": 1}]))
    exp = {"glued": bytes(b for i, b in enumerate(data) if i % 16 or i == 0),
           "same": data,
           "end0": data + b"\0",
           "each0": b"".join(data[i:i + 16] + b"\0" for i in range(0, len(data), 16))}[kind]
    assert frames[0][42:] == exp


def test_file_embedded_nul_stops_both(tmp_path):
    path = tmp_path / "p.bin"
    path.write_bytes(b"GET / HTTP/1.1\r\n\0Host: never sent\r\n")
    frames = _same(_cfg("tcp", [{"exact": str(path), "isfile": 1, "isstring": 1}]))
    assert frames[0][54:] == b"GET / HTTP/1.1\r\n"
    path.write_bytes(b"01 02 03\0 04 05")
    frames = _same(_cfg("udp", [{"exact": str(path), "isfile": 1}]))
    assert frames[0][42:] == b"\x01\x02\x03"


@pytest.mark.parametrize("isstring", [0, 1])
@pytest.mark.parametrize("proto", ["udp", "tcp", "icmp"])
def test_empty_and_missing_files_are_empty_payloads(tmp_path, proto, isstring):
    """sequence.c:282-290: a file that cannot be opened is an empty text, not an error."""
    empty = tmp_path / "empty"
    empty.write_bytes(b"")
    for path in (empty, tmp_path / "no_such_file"):
        frames = _same(_cfg(proto, [{"exact": str(path), "isfile": 1, "isstring": isstring}]))
        assert all(len(f) == HL[proto] for f in frames)


def test_string_with_high_bytes(tmp_path):
    """Bytes >= 0x80 (chars are signed in C: no sign extension may reach the sums)."""
    data = bytes(range(0x80, 0x100)) + b"\xff\xff\xff" + bytes(range(0xFF, 0x7F, -1))
    path = tmp_path / "hi.bin"
    path.write_bytes(data)
    for proto in ("udp", "tcp", "icmp"):
        frames = _same(_cfg(proto, [{"exact": str(path), "isfile": 1, "isstring": 1}]))
        assert frames[0][HL[proto]:] == data
    text = "naïve café ÿ"  # the loaders pass a config string as UTF-8
    frames = _same(_cfg("udp", [{"exact": text, "isstring": 1}]))
    assert frames[0][42:] == text.encode()


@pytest.mark.parametrize("form", ["hex", "string"])
@pytest.mark.parametrize("proto", ["udp", "tcp", "icmp"])
def test_longest_payload_and_one_more(proto, form):
    """PB_MAX_PCKT_LEN - headers bytes build a 65,535-B frame; one byte more is refused."""
    n = LONGEST[proto]
    data = bytes(((7 * i + 3) & 255) or 1 for i in range(n + 1))

    def payload(k):
        return {"exact": _hex(data[:k])} if form == "hex" else {"exact": data[:k].decode("latin-1"), "isstring": 1}

    if form == "string":  # the config string travels as UTF-8: keep its bytes below 0x80
        data = bytes((b & 0x7F) or 1 for b in data)
    frames = _same(_cfg(proto, [payload(n)]), n=2)
    assert len(frames[0]) == 65535 and frames[0][HL[proto]:] == data[:n]
    with pytest.raises(RuntimeError, match=r"pbo_build -> -22$"):
        ob.frames(Sequence.from_config(_cfg(proto, [payload(n + 1)])), 3, FIRST, 1, pc.SEED_BASE)


def test_more_tokens_than_any_frame_are_refused():
    with pytest.raises(RuntimeError, match=r"pbo_build -> -22$"):
        ob.frames(Sequence.from_config(_cfg("udp", [{"exact": "1 " * 70000}])), 3, FIRST, 1, pc.SEED_BASE)


@pytest.mark.parametrize("rule", [0, 1], ids=["stream", "literal"])
@pytest.mark.parametrize("lo,hi", [(1, 1), (129, 129), (1458, 1458), (9000, 60000), (65493, 65493)])
def test_static_random_lengths(lo, hi, rule):
    """isstatic: length and bytes drawn once at setup (sequence.c:339-353); under the literal rule
    the shadowed index stops the fill at the first j with data_len[j] <= j (quirk B8)."""
    frames = _same(_cfg("udp", [{"isstatic": 1, "length": {"min": lo, "max": hi}}]), rule=rule)
    assert lo <= len(frames[0]) - 42 <= hi
    assert len({f[42:] for f in frames}) == 1  # one draw for every iteration
    if rule == 0 and hi > 64:
        assert len(set(frames[0][42:])) > 32  # and it is a drawn payload, not a constant


@pytest.mark.parametrize("rule", [0, 1], ids=["stream", "literal"])
def test_static_random_after_other_payloads(rule):
    """The static seed advances through every static-random payload in turn."""
    pls = [{"isstatic": 1, "length": {"min": 300, "max": 400}}, {"exact": _hex(RAMP[:77])},
           {"isstatic": 1, "length": {"min": 2000, "max": 2100}}, {"length": {"min": 0, "max": 50}},
           {"isstatic": 1, "length": {"min": 1, "max": 2}}]
    for proto in ("udp", "tcp"):
        _same(_cfg(proto, pls), rule=rule)


# ------------------------------------------------------------------ the GPU file's tables
def test_gpu_case_tables_name_every_static_kernel_form():
    """tests/test_gpu_static_payloads.py asserts each case's kernel by these expected names; the
    forms the static paths have must all be among them."""
    names = sc.expected_kernel_names()
    for kern in ("pb_xsmall_kernel", "pb_xpage_kernel", "pb_small_kernel<"):
        for proto in (17, 6):
            assert any(re.match(re.escape(kern) + r".*\b%d, false" % proto, n) for n in names), (kern, proto)
    for g in (8, 16, 32, 64):
        assert "pb_stage_kernel<%d, 0>" % g in names
    assert any(re.fullmatch(r"pb_stage_kernel<\d+, 2>", n) for n in names)
    assert any(re.fullmatch(r"pb_gpf_kernel<\d+, 0>", n) for n in names)
    assert any(re.fullmatch(r"pb_gpf_kernel<\d+, 2>", n) for n in names)
    assert not any(", true" in n or n.endswith(", 1>") for n in names)  # no random-only kernel among them


def test_gpu_case_tables_name_the_planned_kernels():
    """Every case's expected kernel name in static_cases against the library's planner
    (pbgpu_plan_describe, no GPU): the name the GPU file will assert is the one the load chooses."""
    import plan_cases as plc

    want = plc.static_expectations()
    cases = {c[0]: c for c in plc.cases() if c[0] in want}
    assert len(cases) == len(want) == len(sc.small_cases()) + len(sc.stage_cases()) + len(sc.gpf_cases()) + \
        len(sc.mixed_cases())
    for cid, (name, exact) in want.items():
        _, cfg, env, rule, fold = cases[cid]
        got = plc.parse(plc.describe(cfg, env, rule, fold))[0]
        assert got == name if exact else got.startswith(name), (cid, got, name)


def test_gpu_case_tables_follow_test_gpu_kernels():
    """The small-frame lengths and counts and the forced stage shapes are test_gpu_kernels' own."""
    import test_gpu_kernels as tk

    assert sc.XS_LENS == tk.XS_LENS and sc.XS_COUNTS == tk.XS_COUNTS
    shapes = {s[0]: s[1] for s in tk.SHAPES}
    for name, (env, _) in sc.STAGE_SHAPES.items():
        assert shapes[name] == env
    # every table entry is there, none skipped: lengths that cannot hold a payload byte are left out
    assert {c[2] for c in sc.small_cases() if c[1] == "udp"} == {n for n in tk.XS_LENS if n > 42}
    assert {c[2] for c in sc.small_cases() if c[1] == "tcp"} == {n for n in tk.XS_LENS if n > 54}
