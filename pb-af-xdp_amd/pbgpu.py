"""pbgpu — Python binding of libpbgpu.so (include/pbgpu.h) and of the
sequence/config surface (include/pb_config.h).

`Sequence.from_config(dict)` accepts a sequence object in the reference's JSON
schema (README.md:216-575: "eth", "ip", "udp", "tcp", "icmp", "payloads", ...)
with the reference's documented defaults, so a PB-AF-XDP config drives the GPU
build unchanged.  `GpuContext` wraps one device context.

The frame builder only exists on the GPU: if libpbgpu.so is missing, or was
built without a usable device at run time, every build call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Iterable, Optional, Sequence as Seq

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libpbgpu.so")

MAX_PAYLOADS = 64
MAX_RANGES = 64
MAX_SEQUENCES = 256

PAYLOAD_STREAM = 0
PAYLOAD_LITERAL = 1
FOLD_FULL = 0
FOLD_SINGLE = 1

ERRORS = {
    0: "ok",
    -2: "ENOENT",
    -5: "EIO",
    -12: "ENOMEM",
    -19: "ENODEV",
    -22: "EINVAL",
    -28: "ENOSPC",
    -95: "ENOTSUP",
}


class PbError(RuntimeError):
    def __init__(self, code: int, what: str):
        super().__init__(f"{what}: {ERRORS.get(code, code)} ({code})")
        self.code = code


# ---------------------------------------------------------------- ABI types
class PayloadOpt(C.Structure):
    _fields_ = [
        ("exact", C.c_char_p),
        ("is_static", C.c_uint8),
        ("is_file", C.c_uint8),
        ("is_string", C.c_uint8),
        ("min_len", C.c_uint16),
        ("max_len", C.c_uint16),
    ]


class _Eth(C.Structure):
    _fields_ = [("src_mac", C.c_char_p), ("dst_mac", C.c_char_p)]


class _Ip(C.Structure):
    _fields_ = [
        ("src_ip", C.c_char_p),
        ("dst_ip", C.c_char_p),
        ("protocol", C.c_char_p),
        ("tos", C.c_uint8),
        ("csum", C.c_uint8),
        ("min_ttl", C.c_uint8),
        ("max_ttl", C.c_uint8),
        ("min_id", C.c_uint16),
        ("max_id", C.c_uint16),
        ("ranges", C.c_char_p * MAX_RANGES),
        ("range_count", C.c_uint16),
    ]


class _Udp(C.Structure):
    _fields_ = [("src_port", C.c_uint16), ("dst_port", C.c_uint16)]


class _Tcp(C.Structure):
    _fields_ = [("src_port", C.c_uint16), ("dst_port", C.c_uint16)] + [
        (n, C.c_uint8) for n in ("syn", "ack", "psh", "fin", "rst", "urg", "ece", "cwr")
    ]


class _Icmp(C.Structure):
    _fields_ = [("code", C.c_uint8), ("type", C.c_uint8)]


class SequenceT(C.Structure):
    """pb_sequence_t (include/pb_config.h)."""

    _fields_ = [
        ("interface", C.c_char_p),
        ("block", C.c_uint8),
        ("track", C.c_uint8),
        ("max_pckts", C.c_uint64),
        ("max_bytes", C.c_uint64),
        ("pps", C.c_uint64),
        ("bps", C.c_uint64),
        ("time", C.c_uint64),
        ("threads", C.c_uint16),
        ("delay", C.c_uint64),
        ("l4_csum", C.c_uint8),
        ("eth", _Eth),
        ("ip", _Ip),
        ("udp", _Udp),
        ("tcp", _Tcp),
        ("icmp", _Icmp),
        ("pls", PayloadOpt * MAX_PAYLOADS),
        ("pl_cnt", C.c_uint16),
    ]


class Rules(C.Structure):
    _fields_ = [("payload_rule", C.c_uint8), ("iph_fold", C.c_uint8)]


class Frames(C.Structure):
    """pbgpu_frames (include/pbgpu.h)."""

    _fields_ = [
        ("data", C.c_void_p),
        ("offsets", C.c_void_p),
        ("reserved", C.c_void_p),
        ("scan_tmp", C.c_void_p),
        ("capacity_frames", C.c_uint64),
        ("capacity_bytes", C.c_uint64),
        ("seq_idx", C.c_uint16),
        ("first_iter", C.c_uint64),
        ("n_frames", C.c_uint64),
        ("fixed_len", C.c_uint32),
        ("total_bytes", C.c_uint64),
    ]


VERIFY_IP_CSUM = 1
VERIFY_TOT_LEN = 2
VERIFY_L4_CSUM = 4
VERIFY_ALL = 7
VERIFY_SHORT = 8  # code bit only: a frame shorter than 34 B
NO_BAD_FRAME = 0xFFFFFFFFFFFFFFFF  # VerifyResult.first_bad when every frame is good


class VerifyResult(C.Structure):
    """pbgpu_verify_result (include/pbgpu.h)."""

    _fields_ = [
        ("n_checked", C.c_uint64),
        ("n_bad", C.c_uint64),
        ("bad_short", C.c_uint64),
        ("bad_ip_csum", C.c_uint64),
        ("bad_tot_len", C.c_uint64),
        ("bad_l4_csum", C.c_uint64),
        ("first_bad", C.c_uint64),
        ("device_ms", C.c_double),
    ]


PCAP_FILE_HEADER = 1  # the stream starts with the 24-B pcap file header
PCAP_NSEC = 2  # nanosecond magic and ts_frac in ns (else microseconds)


class PcapOpts(C.Structure):
    """pbgpu_pcap_opts (include/pbgpu.h)."""

    _fields_ = [
        ("t0_ns", C.c_uint64),
        ("step_ps", C.c_uint64),
        ("first_index", C.c_uint64),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


ENCAP_VLAN = 1  # an 802.1Q tag after the MAC addresses (4 B)
ENCAP_VXLAN = 2  # outer Ethernet + IPv4 + UDP + VXLAN in front of the frame (50 B, RFC 7348)


class EncapOpts(C.Structure):
    """pbgpu_encap_opts (include/pbgpu.h)."""

    _fields_ = [
        ("mode", C.c_uint32),
        ("flags", C.c_uint32),
        ("tpid", C.c_uint16),
        ("tci", C.c_uint16),
        ("src_port", C.c_uint16),
        ("dst_port", C.c_uint16),
        ("vni", C.c_uint32),
        ("dst_mac", C.c_uint8 * 6),
        ("src_mac", C.c_uint8 * 6),
        ("src_ip", C.c_uint8 * 4),
        ("dst_ip", C.c_uint8 * 4),
        ("ttl", C.c_uint8),
        ("tos", C.c_uint8),
        ("reserved", C.c_uint16),
    ]

    @classmethod
    def make(cls, mode: int, **fields) -> "EncapOpts":
        """mode and any of the struct's fields; addresses as bytes in wire order."""
        o = cls()
        o.mode = mode
        for k, v in fields.items():
            if k in ("dst_mac", "src_mac", "src_ip", "dst_ip"):
                v = type(getattr(o, k)).from_buffer_copy(bytes(v))
            elif k not in dict(cls._fields_):
                raise TypeError(f"EncapOpts has no field {k!r}")
            setattr(o, k, v)
        return o


FRAG_IGNORE_DF = 1  # split frames whose DF bit is set too


class FragOpts(C.Structure):
    """pbgpu_frag_opts (include/pbgpu.h)."""

    _fields_ = [
        ("mtu", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint64),
    ]


class FragResult(C.Structure):
    """pbgpu_frag_result (include/pbgpu.h)."""

    _fields_ = [
        ("n_in", C.c_uint64),
        ("n_out", C.c_uint64),
        ("n_split", C.c_uint64),
        ("n_df", C.c_uint64),
        ("n_other", C.c_uint64),
        ("out_bytes", C.c_uint64),
        ("out_min_len", C.c_uint32),
        ("out_max_len", C.c_uint32),
        ("device_ms", C.c_double),
    ]


SEG_NO_L4_CSUM = 1  # the L4 checksum field is copied from the source; no payload byte is summed
SEG_FIXED_ID = 2    # every segment keeps the source's IPv4 ID


class SegOpts(C.Structure):
    """pbgpu_seg_opts (include/pbgpu.h)."""

    _fields_ = [
        ("mss", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint64),
    ]


class SegResult(C.Structure):
    """pbgpu_seg_result (include/pbgpu.h)."""

    _fields_ = [
        ("n_in", C.c_uint64),
        ("n_out", C.c_uint64),
        ("n_split_tcp", C.c_uint64),
        ("n_split_udp", C.c_uint64),
        ("n_other", C.c_uint64),
        ("out_bytes", C.c_uint64),
        ("out_min_len", C.c_uint32),
        ("out_max_len", C.c_uint32),
        ("device_ms", C.c_double),
    ]


def _seg_flags(no_l4_csum: bool, fixed_id: bool) -> int:
    return (SEG_NO_L4_CSUM if no_l4_csum else 0) | (SEG_FIXED_ID if fixed_id else 0)


STAMP_TAIL = 1     # position counted back from the frame's end
STAMP_NO_CSUM = 2  # leave the L4 checksum as it is


class StampOpts(C.Structure):
    """pbgpu_stamp_opts (include/pbgpu.h)."""

    _fields_ = [
        ("t0_ns", C.c_uint64),
        ("step_ps", C.c_uint64),
        ("first_index", C.c_uint64),
        ("offset", C.c_uint32),
        ("flags", C.c_uint32),
    ]


class StampResult(C.Structure):
    """pbgpu_stamp_result (include/pbgpu.h)."""

    _fields_ = [
        ("n_in", C.c_uint64),
        ("n_stamped", C.c_uint64),
        ("n_short", C.c_uint64),
        ("n_other", C.c_uint64),
        ("device_ms", C.c_double),
    ]


XLAT_HASH_FLOW = 1  # the flow label hashed per frame from the addresses and ports


class XlatOpts(C.Structure):
    """pbgpu_xlat_opts (include/pbgpu.h)."""

    _fields_ = [
        ("src_prefix", C.c_uint8 * 12),
        ("dst_prefix", C.c_uint8 * 12),
        ("flow_label", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint64),
    ]

    @classmethod
    def make(cls, src_prefix: bytes, dst_prefix: Optional[bytes] = None, flow_label: int = 0,
             hash_flow: bool = False) -> "XlatOpts":
        """The two /96 prefixes as 12 bytes in wire order (dst_prefix None: the source's)."""
        o = cls()
        if dst_prefix is None:
            dst_prefix = src_prefix
        if len(src_prefix) != 12 or len(dst_prefix) != 12:
            raise ValueError("a /96 prefix is 12 bytes")
        o.src_prefix = (C.c_uint8 * 12).from_buffer_copy(bytes(src_prefix))
        o.dst_prefix = (C.c_uint8 * 12).from_buffer_copy(bytes(dst_prefix))
        o.flow_label = flow_label
        o.flags = XLAT_HASH_FLOW if hash_flow else 0
        return o


class XlatResult(C.Structure):
    """pbgpu_xlat_result (include/pbgpu.h)."""

    _fields_ = [
        ("n_in", C.c_uint64),
        ("n_udp", C.c_uint64),
        ("n_tcp", C.c_uint64),
        ("n_icmp", C.c_uint64),
        ("n_other", C.c_uint64),
        ("first_other", C.c_uint64),
        ("device_ms", C.c_double),
    ]


WIRE_L3_CSUM = 1  # every IPv4 header parsed folds to 0xFFFF
WIRE_L3_LEN = 2  # IPv4 tot_len / IPv6 payload length agree with the frame's length
WIRE_L4_CSUM = 4  # UDP / TCP / ICMP / ICMPv6 checksum
WIRE_UDP_LEN = 8  # a UDP header's length field
WIRE_ALL = 15
WIRE_MALFORMED = 16  # code bit only, always checked
WIRE_NOL4 = 32  # info bit: IP, but no L4 checksum that can be evaluated
WIRE_INNER = 64  # info bit: a VXLAN inner frame was parsed
WIRE_OTHER = 128  # info bit: not IP, nothing checked


class WireOpts(C.Structure):
    """pbgpu_wire_opts (include/pbgpu.h)."""

    _fields_ = [
        ("checks", C.c_uint32),
        ("flags", C.c_uint32),
        ("vxlan_port", C.c_uint16),
        ("reserved", C.c_uint16 * 3),
    ]


class WireResult(C.Structure):
    """pbgpu_wire_result (include/pbgpu.h)."""

    _fields_ = [
        ("n_checked", C.c_uint64),
        ("n_bad", C.c_uint64),
        ("bad_malformed", C.c_uint64),
        ("bad_l3_csum", C.c_uint64),
        ("bad_l3_len", C.c_uint64),
        ("bad_l4_csum", C.c_uint64),
        ("bad_udp_len", C.c_uint64),
        ("first_bad", C.c_uint64),
        ("n_ipv4", C.c_uint64),
        ("n_ipv6", C.c_uint64),
        ("n_inner", C.c_uint64),
        ("n_nol4", C.c_uint64),
        ("n_other", C.c_uint64),
        ("device_ms", C.c_double),
    ]


# ------------------------------------------------------------- sequences
def _b(s: Optional[str]) -> Optional[bytes]:
    return None if s is None else s.encode()


class Sequence:
    """Owns a SequenceT plus the byte strings its char* fields point at."""

    def __init__(self) -> None:
        self.c = SequenceT()
        self._keep: list = []
        self.set_defaults()

    def _str(self, s: Optional[str]) -> Optional[bytes]:
        b = _b(s)
        if b is not None:
            self._keep.append(b)
        return b

    def set_defaults(self) -> None:
        """Defaults documented in README.md:216-575 (PB-Common clear_sequence)."""
        c = self.c
        c.block = 1
        c.track = 0
        c.delay = 1000000
        c.l4_csum = 1
        c.ip.csum = 1
        c.ip.min_ttl = 64
        c.ip.max_ttl = 64
        c.ip.min_id = 0
        c.ip.max_id = 64000

    @classmethod
    def from_config(cls, cfg: dict) -> "Sequence":
        """A sequence object in the reference's JSON schema (README.md:216-575)."""
        s = cls()
        c = s.c
        c.interface = s._str(cfg.get("interface"))
        for key, field in (("block", "block"), ("track", "track"), ("maxpckts", "max_pckts"),
                           ("maxbytes", "max_bytes"), ("pps", "pps"), ("bps", "bps"), ("time", "time"),
                           ("threads", "threads"), ("delay", "delay"), ("l4csum", "l4_csum")):
            if key in cfg and cfg[key] is not None:
                setattr(c, field, int(cfg[key]))
        eth = cfg.get("eth", {}) or {}
        c.eth.src_mac = s._str(eth.get("smac"))
        c.eth.dst_mac = s._str(eth.get("dmac"))
        ip = cfg.get("ip", {}) or {}
        c.ip.src_ip = s._str(ip.get("sip"))
        c.ip.dst_ip = s._str(ip.get("dip"))
        c.ip.protocol = s._str(ip.get("protocol"))
        if "tos" in ip:
            c.ip.tos = int(ip["tos"])
        if "csum" in ip:
            c.ip.csum = int(ip["csum"])
        ttl = ip.get("ttl", {}) or {}
        if "min" in ttl:
            c.ip.min_ttl = int(ttl["min"])
        if "max" in ttl:
            c.ip.max_ttl = int(ttl["max"])
        idd = ip.get("id", {}) or {}
        if "min" in idd:
            c.ip.min_id = int(idd["min"])
        if "max" in idd:
            c.ip.max_id = int(idd["max"])
        ranges = ip.get("ranges", []) or []
        if len(ranges) > MAX_RANGES:
            raise ValueError("too many ranges")
        for i, r in enumerate(ranges):
            c.ip.ranges[i] = s._str(r)
        c.ip.range_count = len(ranges)
        udp = cfg.get("udp", {}) or {}
        c.udp.src_port = int(udp.get("sport", 0))
        c.udp.dst_port = int(udp.get("dport", 0))
        tcp = cfg.get("tcp", {}) or {}
        c.tcp.src_port = int(tcp.get("sport", 0))
        c.tcp.dst_port = int(tcp.get("dport", 0))
        for fl in ("syn", "ack", "psh", "fin", "rst", "urg", "ece", "cwr"):
            setattr(c.tcp, fl, int(tcp.get(fl, 0)))
        icmp = cfg.get("icmp", {}) or {}
        c.icmp.code = int(icmp.get("code", 0))
        c.icmp.type = int(icmp.get("type", 0))
        pls = cfg.get("payloads", []) or []
        if len(pls) > MAX_PAYLOADS:
            raise ValueError("too many payloads")
        for i, p in enumerate(pls):
            po = c.pls[i]
            po.exact = s._str(p.get("exact"))
            po.is_static = int(p.get("isstatic", 0))
            po.is_file = int(p.get("isfile", 0))
            po.is_string = int(p.get("isstring", 0))
            ln = p.get("length", {}) or {}
            po.min_len = int(ln.get("min", 0))
            po.max_len = int(ln.get("max", 0))
        c.pl_cnt = len(pls)
        return s

    @property
    def frames_per_iter(self) -> int:
        return max(1, int(self.c.pl_cnt))


def parse_mac(s: Optional[str]) -> bytes:
    if not s:
        return bytes(6)
    return bytes(int(x, 16) for x in s.split(":"))


# --------------------------------------------------------------- library
_libs = {}


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """Load libpbgpu.so (raises if it is absent: there is no CPU fallback).
    Other paths load other builds side by side (compile-time A/B probes)."""
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not built (run `make -C pb-af-xdp_amd`): the GPU path has no fallback")
    lib = C.CDLL(path)
    P, U8P, U64P = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    FP = C.POINTER(Frames)
    sig = {
        "pbgpu_open": (C.c_int, [C.c_int, C.POINTER(P)]),
        "pbgpu_close": (None, [P]),
        "pbgpu_strerror": (C.c_char_p, [C.c_int]),
        "pbgpu_device_count": (C.c_int, [C.POINTER(C.c_int)]),
        "pbgpu_load_sequence": (C.c_int, [P, C.c_uint16, C.POINTER(SequenceT), U8P, U8P, C.POINTER(Rules),
                                          C.c_uint64]),
        "pbgpu_build_size": (C.c_int, [P, C.c_uint16, C.c_uint64, U64P, U64P]),
        "pbgpu_frames_alloc": (C.c_int, [P, C.c_uint64, C.c_uint64, C.POINTER(FP)]),
        "pbgpu_frames_free": (None, [P, FP]),
        "pbgpu_build": (C.c_int, [P, C.c_uint16, C.c_uint64, C.c_uint64, FP]),
        "pbgpu_build_batch": (C.c_int, [P, C.c_uint32, C.POINTER(C.c_uint16), U64P, U64P, C.POINTER(FP)]),
        "pbgpu_sync": (C.c_int, [P]),
        "pbgpu_frames_total": (C.c_int, [P, FP, U64P]),
        "pbgpu_frames_offsets": (C.c_int, [P, FP]),
        "pbgpu_copy_packed": (C.c_int, [P, FP, P, C.c_uint64, C.c_uint64]),
        "pbgpu_copy_offsets": (C.c_int, [P, FP, U64P]),
        "pbgpu_copy_to_umem": (C.c_int, [P, FP, P, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32,
                                         C.POINTER(C.c_uint16)]),
        "pbgpu_host_register": (C.c_int, [P, P, C.c_size_t]),
        "pbgpu_host_unregister": (C.c_int, [P, P]),
        "pbgpu_counters": (C.c_int, [P, U64P, U64P, C.c_int]),
        "pbgpu_kernel_time": (C.c_int, [P, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
        "pbgpu_set_timing": (C.c_int, [P, C.c_int]),
        "pbgpu_kernel_times": (C.c_int, [P, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_uint32)]),
        "pbgpu_fill_probe": (C.c_int, [P, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]),
        "pbgpu_fill_probe_ex": (C.c_int, [P, C.c_uint64, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
        "pbgpu_fill_probe_at": (C.c_int, [P, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]),
        "pbgpu_fill_shape_name": (C.c_char_p, [C.c_int]),
        "pbgpu_verify": (C.c_int, [P, FP, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(VerifyResult), P]),
        "pbgpu_frames_upload": (C.c_int, [P, FP, P, U64P, C.c_uint32, C.c_uint64]),
        "pbgpu_read_probe_at": (C.c_int, [P, P, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]),
        "pbgpu_page_grid": (C.c_int, [P, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "pbgpu_pcap_size": (C.c_int, [P, FP, C.c_uint64, C.c_uint64, C.c_uint32, U64P]),
        "pbgpu_pcap_pack": (C.c_int, [P, FP, C.c_uint64, C.c_uint64, C.POINTER(PcapOpts), FP, U64P,
                                      C.POINTER(C.c_double)]),
        "pbgpu_encap_size": (C.c_int, [P, FP, C.c_uint64, C.c_uint64, C.POINTER(EncapOpts), U64P, U64P]),
        "pbgpu_encap": (C.c_int, [P, FP, C.c_uint64, C.c_uint64, C.POINTER(EncapOpts), FP, C.POINTER(C.c_double)]),
        "pbgpu_fragment_size": (C.c_int, [P, FP, C.c_uint64, C.c_uint64, C.POINTER(FragOpts), U64P, U64P]),
        "pbgpu_fragment_bound": (C.c_int, [P, FP, C.c_uint64, C.c_uint64, C.POINTER(FragOpts), U64P, U64P]),
        "pbgpu_fragment": (C.c_int, [P, FP, C.c_uint64, C.c_uint64, C.POINTER(FragOpts), FP, C.POINTER(FragResult)]),
        "pbgpu_segment_size": (C.c_int, [P, FP, C.c_uint64, C.c_uint64, C.POINTER(SegOpts), U64P, U64P]),
        "pbgpu_segment_bound": (C.c_int, [P, FP, C.c_uint64, C.c_uint64, C.POINTER(SegOpts), U64P, U64P]),
        "pbgpu_segment": (C.c_int, [P, FP, C.c_uint64, C.c_uint64, C.POINTER(SegOpts), FP, C.POINTER(SegResult)]),
        "pbgpu_stamp": (C.c_int, [P, FP, C.c_uint64, C.c_uint64, C.POINTER(StampOpts), C.POINTER(StampResult)]),
        "pbgpu_xlat46_size": (C.c_int, [P, FP, C.c_uint64, C.c_uint64, C.POINTER(XlatOpts), U64P, U64P]),
        "pbgpu_xlat46": (C.c_int, [P, FP, C.c_uint64, C.c_uint64, C.POINTER(XlatOpts), FP, C.POINTER(XlatResult)]),
        "pbgpu_verify_wire": (C.c_int, [P, FP, C.c_uint64, C.c_uint64, C.POINTER(WireOpts), C.POINTER(WireResult), P]),
        "pbgpu_abi_size": (C.c_size_t, [C.c_int]),
        "pbgpu_kernel_name": (C.c_int, [P, C.c_uint16, C.c_char_p, C.c_size_t]),
        "pbgpu_plan_describe": (C.c_int, [C.c_uint16, C.POINTER(SequenceT), C.POINTER(Rules), C.c_uint64, C.c_char_p,
                                          C.c_size_t]),
    }
    for name, (res, args) in sig.items():
        if path != LIB_PATH and not hasattr(lib, name):
            continue  # an older build loaded for an A/B lacks the newer entry points
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _libs[path] = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise PbError(rc, what)


def _u8(b: Optional[bytes]):
    if b is None:
        return None
    return (C.c_uint8 * 6).from_buffer_copy(b)


class FrameBuffer:
    """A device-resident pbgpu_frames allocation."""

    def __init__(self, ctx: "GpuContext", ptr):
        self.ctx = ctx
        self.ptr = ptr

    @property
    def f(self) -> Frames:
        return self.ptr.contents

    def total_bytes(self) -> int:
        t = C.c_uint64()
        _check(self.ctx.lib.pbgpu_frames_total(self.ctx.h, self.ptr, C.byref(t)), "frames_total")
        return int(t.value)

    def fill_offsets(self) -> None:
        """offsets[] on the device (variable length: expanded from the 4-B form on first use)."""
        _check(self.ctx.lib.pbgpu_frames_offsets(self.ctx.h, self.ptr), "frames_offsets")

    def offsets(self) -> np.ndarray:
        n = int(self.f.n_frames)
        out = np.empty(n + 1, dtype=np.uint64)
        _check(self.ctx.lib.pbgpu_copy_offsets(self.ctx.h, self.ptr, out.ctypes.data_as(C.POINTER(C.c_uint64))),
               "copy_offsets")
        return out

    def packed(self) -> np.ndarray:
        total = self.total_bytes()
        out = np.empty(total, dtype=np.uint8)
        if total:
            _check(self.ctx.lib.pbgpu_copy_packed(self.ctx.h, self.ptr, out.ctypes.data, 0, total), "copy_packed")
        return out

    def frames(self) -> list:
        data = self.packed()
        off = self.offsets()
        return [data[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(off) - 1)]

    def to_umem(self, umem: np.ndarray, slot: int, first_frame: int, n: int, first_slot: int = 0) -> np.ndarray:
        lens = np.empty(n, dtype=np.uint16)
        _check(self.ctx.lib.pbgpu_copy_to_umem(self.ctx.h, self.ptr, umem.ctypes.data, slot, first_slot,
                                               first_frame, n, lens.ctypes.data_as(C.POINTER(C.c_uint16))),
               "copy_to_umem")
        return lens

    def verify(self, first: int = 0, n: Optional[int] = None, checks: int = VERIFY_ALL, codes: bool = False):
        """Checks frames [first, first + n) on the GPU (n None: to the last frame).  Returns the
        VerifyResult, and with codes=True also each frame's failed-check bits (np.uint8)."""
        if n is None:
            n = int(self.f.n_frames) - first
        res = VerifyResult()
        out = np.zeros(n if codes else 0, dtype=np.uint8)
        _check(self.ctx.lib.pbgpu_verify(self.ctx.h, self.ptr, first, n, checks, C.byref(res),
                                         out.ctypes.data if codes and n else None), "verify")
        return (res, out) if codes else res

    def verify_wire(self, first: int = 0, n: Optional[int] = None, checks: int = WIRE_ALL, vxlan_port: int = 0,
                    codes: bool = False):
        """Checks frames [first, first + n) on the GPU as they would leave (n None: to the last frame):
        VLAN tags, IPv4 with options or IPv6, and behind UDP port vxlan_port a VXLAN inner frame are
        parsed from the frame's own bytes.  Returns the WireResult, and with codes=True also each
        frame's code (np.uint8, WIRE_* bits)."""
        if n is None:
            n = int(self.f.n_frames) - first
        opts = WireOpts(checks, 0, vxlan_port)
        res = WireResult()
        out = np.zeros(n if codes else 0, dtype=np.uint8)
        _check(self.ctx.lib.pbgpu_verify_wire(self.ctx.h, self.ptr, first, n, C.byref(opts), C.byref(res),
                                              out.ctypes.data if codes and n else None), "verify_wire")
        return (res, out) if codes else res

    def upload(self, data, offsets=None, fixed_len: int = 0) -> None:
        """Puts caller-supplied frames into the buffer, packed: `offsets` (n + 1 entries, frame j
        at data[offsets[j] - offsets[0]:]) or fixed_len-byte frames back to back."""
        data = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray))
                                    else data, dtype=np.uint8)
        if offsets is not None:
            off = np.ascontiguousarray(offsets, dtype=np.uint64)
            if len(off) < 1:
                raise ValueError("offsets needs n + 1 entries")
            n, offp = len(off) - 1, off.ctypes.data_as(C.POINTER(C.c_uint64))
        else:
            if fixed_len <= 0:
                raise ValueError("upload needs offsets or a fixed length")
            n, offp = len(data) // fixed_len, None
        _check(self.ctx.lib.pbgpu_frames_upload(self.ctx.h, self.ptr, data.ctypes.data if len(data) else None, offp,
                                                fixed_len, n), "frames_upload")

    def pcap_pack(self, dst: "FrameBuffer", first: int = 0, n: Optional[int] = None, t0_ns: int = 0,
                  step_ps: int = 0, first_index: int = 0, file_header: bool = True, nsec: bool = False):
        """Packs frames [first, first + n) (n None: to the last frame) into dst's device bytes as a
        pcap stream: frame j stamped t0_ns + (first_index + j) * step_ps / 1000 ns.  Returns
        (nbytes, device_ms); dst.stream(nbytes) fetches the bytes."""
        if n is None:
            n = int(self.f.n_frames) - first
        opts = PcapOpts(t0_ns, step_ps, first_index,
                        (PCAP_FILE_HEADER if file_header else 0) | (PCAP_NSEC if nsec else 0), 0)
        nbytes, ms = C.c_uint64(), C.c_double()
        _check(self.ctx.lib.pbgpu_pcap_pack(self.ctx.h, self.ptr, first, n, C.byref(opts), dst.ptr, C.byref(nbytes),
                                            C.byref(ms)), "pcap_pack")
        return int(nbytes.value), float(ms.value)

    def stream(self, nbytes: int, byte_offset: int = 0) -> np.ndarray:
        """nbytes of the buffer's device bytes from byte_offset (a packed pcap stream's window)."""
        out = np.empty(nbytes, dtype=np.uint8)
        if nbytes:
            _check(self.ctx.lib.pbgpu_copy_packed(self.ctx.h, self.ptr, out.ctypes.data, byte_offset, nbytes),
                   "copy_packed")
        return out

    def pcap_bytes(self, first: int = 0, n: Optional[int] = None, t0_ns: int = 0, step_ps: int = 0,
                   first_index: int = 0, file_header: bool = True, nsec: bool = False) -> np.ndarray:
        """The pcap stream of frames [first, first + n) as host bytes: allocates a buffer of the
        stream's size, packs into it, copies back and frees it."""
        if n is None:
            n = int(self.f.n_frames) - first
        flags = (PCAP_FILE_HEADER if file_header else 0) | (PCAP_NSEC if nsec else 0)
        dst = self.ctx.alloc_frames(1, max(16, self.ctx.pcap_size(self, first, n, flags)))
        try:
            nbytes, _ = self.pcap_pack(dst, first, n, t0_ns, step_ps, first_index, file_header, nsec)
            return dst.stream(nbytes)
        finally:
            dst.free()

    def encap(self, dst: "FrameBuffer", first: int = 0, n: Optional[int] = None, mode: int = ENCAP_VLAN,
              opts: Optional[EncapOpts] = None, **fields) -> float:
        """Encapsulates frames [first, first + n) (n None: to the last frame) into dst, which is then
        a frames buffer like a built one: mode ENCAP_VLAN (tci, tpid) or ENCAP_VXLAN (dst_mac, src_mac,
        src_ip, dst_ip, vni, src_port, dst_port, ttl, tos), or a ready EncapOpts.  Returns device ms."""
        if n is None:
            n = int(self.f.n_frames) - first
        if opts is None:
            opts = EncapOpts.make(mode, **fields)
        ms = C.c_double()
        _check(self.ctx.lib.pbgpu_encap(self.ctx.h, self.ptr, first, n, C.byref(opts), dst.ptr, C.byref(ms)), "encap")
        return float(ms.value)

    def fragment(self, dst: "FrameBuffer", first: int = 0, n: Optional[int] = None, mtu: int = 1500,
                 ignore_df: bool = False) -> FragResult:
        """Fragments frames [first, first + n) (n None: to the last frame) into dst so that no IPv4
        packet exceeds mtu; dst is then a frames buffer like a built one.  Returns the FragResult."""
        if n is None:
            n = int(self.f.n_frames) - first
        opts = FragOpts(mtu, FRAG_IGNORE_DF if ignore_df else 0, 0)
        res = FragResult()
        _check(self.ctx.lib.pbgpu_fragment(self.ctx.h, self.ptr, first, n, C.byref(opts), dst.ptr, C.byref(res)),
               "fragment")
        return res

    def segment(self, dst: "FrameBuffer", first: int = 0, n: Optional[int] = None, mss: int = 1460,
                no_l4_csum: bool = False, fixed_id: bool = False) -> SegResult:
        """Cuts the TCP and UDP frames among [first, first + n) (n None: to the last frame) into
        segments of at most mss payload bytes, each with its own headers and checksums, into dst; dst
        is then a frames buffer like a built one.  Returns the SegResult."""
        if n is None:
            n = int(self.f.n_frames) - first
        opts = SegOpts(mss, _seg_flags(no_l4_csum, fixed_id), 0)
        res = SegResult()
        _check(self.ctx.lib.pbgpu_segment(self.ctx.h, self.ptr, first, n, C.byref(opts), dst.ptr, C.byref(res)),
               "segment")
        return res

    def stamp(self, first: int = 0, n: Optional[int] = None, t0_ns: int = 0, step_ps: int = 0, first_index: int = 0,
              offset: int = 0, tail: bool = False, csum: bool = True, flags: Optional[int] = None) -> StampResult:
        """Stamps frames [first, first + n) (n None: to the last frame) in place: BE64(first_index + j)
        and BE64(t0_ns + (first_index + j) * step_ps / 1000) at `offset` bytes into the L4 payload (tail:
        back from the frame's end), the L4 checksum updated unless csum is False.  `flags` overrides
        tail and csum with raw PBGPU_STAMP_* bits.  Returns the StampResult."""
        if n is None:
            n = int(self.f.n_frames) - first
        if flags is None:
            flags = (STAMP_TAIL if tail else 0) | (0 if csum else STAMP_NO_CSUM)
        opts = StampOpts(t0_ns, step_ps, first_index, offset, flags)
        res = StampResult()
        _check(self.ctx.lib.pbgpu_stamp(self.ctx.h, self.ptr, first, n, C.byref(opts), C.byref(res)), "stamp")
        return res

    def xlat46(self, dst: "FrameBuffer", first: int = 0, n: Optional[int] = None, opts: Optional[XlatOpts] = None,
               res: Optional[XlatResult] = None) -> XlatResult:
        """Translates frames [first, first + n) (n None: to the last frame) to IPv6 into dst (RFC 7915
        under the /96 prefixes of opts, an XlatOpts), which is then a frames buffer like a built one.
        One frame that cannot be translated refuses the whole call (PbError -22), dst untouched; a
        caller's own `res` then still holds the counts.  Returns the XlatResult."""
        if n is None:
            n = int(self.f.n_frames) - first
        if opts is None:
            raise TypeError("xlat46 needs an XlatOpts")
        if res is None:
            res = XlatResult()
        _check(self.ctx.lib.pbgpu_xlat46(self.ctx.h, self.ptr, first, n, C.byref(opts), dst.ptr, C.byref(res)),
               "xlat46")
        return res

    def free(self) -> None:
        if self.ptr is not None:
            self.ctx.lib.pbgpu_frames_free(self.ctx.h, self.ptr)
            self.ptr = None


class GpuContext:
    """One pbgpu_ctx (one GPU)."""

    def __init__(self, device: int = 0, lib_path: str = LIB_PATH):
        self.lib = load_library(lib_path)
        h = C.c_void_p()
        _check(self.lib.pbgpu_open(device, C.byref(h)), f"pbgpu_open({device})")
        self.h = h
        self._seqs = {}

    def close(self) -> None:
        if self.h:
            self.lib.pbgpu_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def load_sequence(self, idx: int, seq: Sequence, seed_base: int, smac: Optional[bytes] = None,
                      dmac: Optional[bytes] = None, payload_rule: int = PAYLOAD_STREAM,
                      iph_fold: int = FOLD_FULL) -> None:
        rules = Rules(payload_rule, iph_fold)
        _check(self.lib.pbgpu_load_sequence(self.h, idx, C.byref(seq.c), _u8(smac), _u8(dmac), C.byref(rules),
                                            C.c_uint64(seed_base)), "load_sequence")
        self._seqs[idx] = seq

    def build_size(self, idx: int, n_iter: int):
        mf, mb = C.c_uint64(), C.c_uint64()
        _check(self.lib.pbgpu_build_size(self.h, idx, n_iter, C.byref(mf), C.byref(mb)), "build_size")
        return int(mf.value), int(mb.value)

    def alloc_frames(self, capacity_frames: int, capacity_bytes: int) -> FrameBuffer:
        p = C.POINTER(Frames)()
        _check(self.lib.pbgpu_frames_alloc(self.h, capacity_frames, capacity_bytes, C.byref(p)), "frames_alloc")
        return FrameBuffer(self, p)

    def build(self, idx: int, first_iter: int, n_iter: int, fb: FrameBuffer) -> None:
        _check(self.lib.pbgpu_build(self.h, idx, first_iter, n_iter, fb.ptr), "build")

    def build_batch(self, parts) -> None:
        """parts: (idx, first_iter, n_iter, FrameBuffer) tuples, built as one pbgpu_build_batch
        call (configs[4]'s three sequences: one fused launch)."""
        n = len(parts)
        idx = (C.c_uint16 * n)(*[p[0] for p in parts])
        fi = (C.c_uint64 * n)(*[p[1] for p in parts])
        ni = (C.c_uint64 * n)(*[p[2] for p in parts])
        outs = (C.POINTER(Frames) * n)(*[p[3].ptr for p in parts])
        _check(self.lib.pbgpu_build_batch(self.h, n, idx, fi, ni, outs), "build_batch")

    def sync(self) -> None:
        _check(self.lib.pbgpu_sync(self.h), "sync")

    def counters(self, n_seq: int):
        p = np.zeros(n_seq, dtype=np.uint64)
        b = np.zeros(n_seq, dtype=np.uint64)
        _check(self.lib.pbgpu_counters(self.h, p.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       b.ctypes.data_as(C.POINTER(C.c_uint64)), n_seq), "counters")
        return p, b

    TIMING_LAUNCH, TIMING_SPAN = 0, 1

    def set_timing(self, mode: int) -> None:
        """PBGPU_TIMING_LAUNCH: an event pair per launch; PBGPU_TIMING_SPAN: one
        span per kernel_time() call (no per-launch events)."""
        _check(self.lib.pbgpu_set_timing(self.h, mode), "set_timing")

    def kernel_time(self):
        ms, n = C.c_double(), C.c_uint32()
        _check(self.lib.pbgpu_kernel_time(self.h, C.byref(ms), C.byref(n)), "kernel_time")
        return float(ms.value), int(n.value)

    def kernel_times(self, cap: int = 4096) -> np.ndarray:
        """TIMING_LAUNCH: each launch's device time (ms) since the last call."""
        ms = np.zeros(cap, dtype=np.float64)
        n = C.c_uint32()
        _check(self.lib.pbgpu_kernel_times(self.h, ms.ctypes.data_as(C.POINTER(C.c_double)), cap, C.byref(n)),
               "kernel_times")
        return ms[:min(cap, int(n.value))]

    def fill_probe(self, nbytes: int, reps: int) -> float:
        ms = C.c_double()
        _check(self.lib.pbgpu_fill_probe(self.h, nbytes, reps, C.byref(ms)), "fill_probe")
        return float(ms.value)

    FILL_SHAPES = 15  # PBGPU_FILL_SHAPES

    def fill_probe_shapes(self, nbytes: int, reps: int):
        """Every write-probe shape's mean ms per launch {name: ms} and the fastest's name."""
        ms = (C.c_double * self.FILL_SHAPES)()
        best = C.c_int()
        _check(self.lib.pbgpu_fill_probe_ex(self.h, nbytes, reps, ms, C.byref(best)), "fill_probe_ex")
        names = [self.lib.pbgpu_fill_shape_name(i).decode() for i in range(self.FILL_SHAPES)]
        return {names[i]: float(ms[i]) for i in range(self.FILL_SHAPES)}, names[best.value]

    def fill_probe_at(self, fb: "FrameBuffer", nbytes: int, reps: int):
        """Every write-probe shape's mean ms per launch over a frame buffer's own memory."""
        ms = (C.c_double * self.FILL_SHAPES)()
        _check(self.lib.pbgpu_fill_probe_at(self.h, fb.f.data, nbytes, reps, ms), "fill_probe_at")
        names = [self.lib.pbgpu_fill_shape_name(i).decode() for i in range(self.FILL_SHAPES)]
        return {names[i]: float(ms[i]) for i in range(self.FILL_SHAPES)}

    def read_probe_at(self, fb: "FrameBuffer", nbytes: int, reps: int) -> float:
        """The read probe's mean ms per launch over the first nbytes of a frame buffer's own memory."""
        ms = C.c_double()
        _check(self.lib.pbgpu_read_probe_at(self.h, fb.f.data, nbytes, reps, C.byref(ms)), "read_probe_at")
        return float(ms.value)

    def page_grid(self, npages: int):
        """(pages per workgroup, workgroups) of this context's repack writers (pcap_pack, encap,
        fragment, segment, xlat46) over an output of npages 4-KiB pages; launches nothing."""
        per, grid = C.c_uint32(), C.c_uint32()
        _check(self.lib.pbgpu_page_grid(self.h, npages, C.byref(per), C.byref(grid)), "page_grid")
        return int(per.value), int(grid.value)

    def pcap_size(self, fb: "FrameBuffer", first: int = 0, n: Optional[int] = None, flags: int = PCAP_FILE_HEADER) -> int:
        """Bytes of the pcap stream of fb's frames [first, first + n) (n None: to the last frame)."""
        if n is None:
            n = int(fb.f.n_frames) - first
        nbytes = C.c_uint64()
        _check(self.lib.pbgpu_pcap_size(self.h, fb.ptr, first, n, flags, C.byref(nbytes)), "pcap_size")
        return int(nbytes.value)

    def xlat46_size(self, fb: "FrameBuffer", first: int, n: Optional[int], opts: XlatOpts):
        """(frames, bytes) of the IPv6 translation of fb's frames [first, first + n) (n None: to the last frame)."""
        if n is None:
            n = int(fb.f.n_frames) - first
        frames, nbytes = C.c_uint64(), C.c_uint64()
        _check(self.lib.pbgpu_xlat46_size(self.h, fb.ptr, first, n, C.byref(opts), C.byref(frames), C.byref(nbytes)),
               "xlat46_size")
        return int(frames.value), int(nbytes.value)

    def encap_size(self, fb: "FrameBuffer", first: int, n: Optional[int], opts: EncapOpts):
        """(frames, bytes) of the encapsulation of fb's frames [first, first + n) (n None: to the last frame)."""
        if n is None:
            n = int(fb.f.n_frames) - first
        frames, nbytes = C.c_uint64(), C.c_uint64()
        _check(self.lib.pbgpu_encap_size(self.h, fb.ptr, first, n, C.byref(opts), C.byref(frames), C.byref(nbytes)),
               "encap_size")
        return int(frames.value), int(nbytes.value)

    def _frag_sizes(self, fn, what: str, fb: "FrameBuffer", first: int, n: Optional[int], mtu: int, ignore_df: bool):
        if n is None:
            n = int(fb.f.n_frames) - first
        opts = FragOpts(mtu, FRAG_IGNORE_DF if ignore_df else 0, 0)
        frames, nbytes = C.c_uint64(), C.c_uint64()
        _check(fn(self.h, fb.ptr, first, n, C.byref(opts), C.byref(frames), C.byref(nbytes)), what)
        return int(frames.value), int(nbytes.value)

    def fragment_size(self, fb: "FrameBuffer", first: int = 0, n: Optional[int] = None, mtu: int = 1500,
                      ignore_df: bool = False):
        """The exact (frames, bytes) FrameBuffer.fragment would write (count and scan passes only)."""
        return self._frag_sizes(self.lib.pbgpu_fragment_size, "fragment_size", fb, first, n, mtu, ignore_df)

    def fragment_bound(self, fb: "FrameBuffer", first: int = 0, n: Optional[int] = None, mtu: int = 1500,
                       ignore_df: bool = False):
        """An upper bound of (frames, bytes) from fb's longest frame, with no device work."""
        return self._frag_sizes(self.lib.pbgpu_fragment_bound, "fragment_bound", fb, first, n, mtu, ignore_df)

    def _seg_sizes(self, fn, what: str, fb: "FrameBuffer", first: int, n: Optional[int], mss: int, flags: int):
        if n is None:
            n = int(fb.f.n_frames) - first
        opts = SegOpts(mss, flags, 0)
        frames, nbytes = C.c_uint64(), C.c_uint64()
        _check(fn(self.h, fb.ptr, first, n, C.byref(opts), C.byref(frames), C.byref(nbytes)), what)
        return int(frames.value), int(nbytes.value)

    def segment_size(self, fb: "FrameBuffer", first: int = 0, n: Optional[int] = None, mss: int = 1460,
                     no_l4_csum: bool = False, fixed_id: bool = False):
        """The exact (frames, bytes) FrameBuffer.segment would write (count and scan passes only)."""
        return self._seg_sizes(self.lib.pbgpu_segment_size, "segment_size", fb, first, n, mss,
                               _seg_flags(no_l4_csum, fixed_id))

    def segment_bound(self, fb: "FrameBuffer", first: int = 0, n: Optional[int] = None, mss: int = 1460,
                      no_l4_csum: bool = False, fixed_id: bool = False):
        """An upper bound of (frames, bytes) from fb's longest frame, with no device work."""
        return self._seg_sizes(self.lib.pbgpu_segment_bound, "segment_bound", fb, first, n, mss,
                               _seg_flags(no_l4_csum, fixed_id))

    def kernel_name(self, idx: int) -> str:
        buf = C.create_string_buffer(96)
        _check(self.lib.pbgpu_kernel_name(self.h, idx, buf, 96), "kernel_name")
        return buf.value.decode()

    def build_frames(self, idx: int, first_iter: int, n_iter: int) -> list:
        """Convenience: build into a fresh buffer and return the frames as bytes."""
        mf, mb = self.build_size(idx, n_iter)
        fb = self.alloc_frames(mf, mb)
        try:
            self.build(idx, first_iter, n_iter, fb)
            self.sync()
            return fb.frames()
        finally:
            fb.free()


def plan_describe(idx: int, seq: Sequence, seed_base: int, payload_rule: int = PAYLOAD_STREAM,
                  iph_fold: int = FOLD_FULL) -> str:
    """What load_sequence would choose for seq under the present PBGPU_* environment, as one line:
    the kernel's name, " | ", then key=value pairs.  Needs no GPU and no context."""
    rules = Rules(payload_rule, iph_fold)
    buf = C.create_string_buffer(1024)
    _check(load_library().pbgpu_plan_describe(idx, C.byref(seq.c), C.byref(rules), C.c_uint64(seed_base), buf,
                                              len(buf)), "plan_describe")
    return buf.value.decode()


def device_count() -> int:
    lib = load_library()
    n = C.c_int()
    lib.pbgpu_device_count(C.byref(n))
    return int(n.value)
