"""The verify surface without a GPU: the --verify option, the header and the library's exports,
the result struct's size, and the NULL-context refusals."""
import ctypes as C
import os
import re
import subprocess

import cmdline_binding as cb
import pbgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pb-af-xdp_amd")
BIN = os.path.join(PKG, "bin", "pcktbatch-gpu")


class VerifyCmd(C.Structure):
    """struct cmd_line_af_xdp with its new last member (host/cmd_line.h): `verify` takes the four
    bytes that were padding after umem_slot, so the struct keeps its size."""

    _fields_ = cb.OurCmd._fields_ + [("verify", C.c_int)]


def host():
    return C.CDLL(os.path.join(PKG, "lib", "libpbhost.so"))


def test_verify_option_parses():
    lib = host()
    assert C.sizeof(VerifyCmd) == C.sizeof(cb.OurCmd) and VerifyCmd.verify.offset == 92
    got = cb.parse(lib, VerifyCmd, ["--gpus", "2", "--verify", "--umemslot", "64"],
                   defaults=lib.cmd_line_af_xdp_defaults)
    assert (got.verify, got.gpus, got.umem_slot) == (1, 2, 64)
    got = cb.parse(lib, VerifyCmd, ["--gpus", "2"], defaults=lib.cmd_line_af_xdp_defaults)
    assert got.verify == 0


def test_verify_is_written_only_when_given():
    """Neither the defaults nor a parse without --verify store to the field."""
    lib = host()
    C.c_int.in_dll(cb._libc, "optind").value = 0
    obj = VerifyCmd()
    obj.verify = 0x5A5A5A5A
    lib.cmd_line_af_xdp_defaults(C.byref(obj))
    args = [b"pcktbatch", b"--queue", b"3", b"--umemframes", b"128"]
    arr = (C.c_char_p * (len(args) + 1))(*args, None)
    lib.parse_cmd_line_af_xdp(C.byref(obj), len(args), arr)
    assert obj.verify == 0x5A5A5A5A and obj.queue == 3 and obj.umem_frames == 128


def test_help_names_verify():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--verify" in r.stdout


def test_verify_with_list_needs_no_gpu():
    r = subprocess.run([BIN, "-z", "--dip", "10.0.0.2", "--verify", "--gpus", "3", "-l"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0 and "gpus=3" in r.stdout


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "pbgpu.h")).read()
    lib = pbgpu.load_library()
    for fn in ("pbgpu_verify", "pbgpu_frames_upload", "pbgpu_read_probe_at"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, hdr), fn
        assert hasattr(lib, fn), fn
    for name, val in (("IP_CSUM", 1), ("TOT_LEN", 2), ("L4_CSUM", 4), ("ALL", 7), ("SHORT", 8)):
        assert re.search(r"#define\s+PBGPU_VERIFY_%s\s+%du\b" % (name, val), hdr), name
        assert getattr(pbgpu, "VERIFY_" + name) == val


def test_result_struct_size():
    lib = pbgpu.load_library()
    assert lib.pbgpu_abi_size(7) == C.sizeof(pbgpu.VerifyResult) == 64
    assert pbgpu.VerifyResult.first_bad.offset == 48 and pbgpu.VerifyResult.device_ms.offset == 56
    assert lib.pbgpu_abi_size(2) == C.sizeof(pbgpu.Frames)  # unchanged by this


def test_null_context_is_refused():
    lib = pbgpu.load_library()
    res = pbgpu.VerifyResult()
    frames = pbgpu.Frames()
    ms = C.c_double()
    data = (C.c_uint8 * 64)()
    assert lib.pbgpu_verify(None, C.byref(frames), 0, 0, 7, C.byref(res), None) == -22
    assert lib.pbgpu_frames_upload(None, C.byref(frames), data, None, 64, 1) == -22
    assert lib.pbgpu_read_probe_at(None, data, 64, 1, C.byref(ms)) == -22
