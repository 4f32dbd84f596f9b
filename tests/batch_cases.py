"""pbgpu_build_batch's fused launch (pb_batch_kernel): which sequences it admits, the page arithmetic
of each part, and the table of cases tests/test_gpu_batch_family.py runs; no GPU here
(tests/test_batch_cases_cpu.py checks this file against itself and the oracle).

The rule, restated from the comments of the planner (pb_make_plan) and pbk_batch_kind, and held
against the planner itself in tests/test_batch_cases_cpu.py.  A sequence has a
fused form when it has one payload and one frame length of at most 128 B, was not loaded under
PBGPU_BATCH=0 or PBGPU_KERNEL=linear, and is one of
  kind 1  UDP, random payload, 64 B, on the whole-frame page kernel (so not under PBGPU_XP_FORCE=1,
          which moves every even length to the cut-frame page kernel);
  kind 2  TCP, random payload, a multiple of 4 from 52 to 64 B on the cut-frame page kernel: 56 and
          60 B (54 B of headers: no 52), and 64 B only under PBGPU_XP_FORCE=1 (without it 64 B divides
          the page and takes the whole-frame kernel); not under PBGPU_KERNEL=nopage unless forced;
  kind 3  ICMP, static payload, 2 mod 4 and over 64 B (66 ... 126) on the cut-frame page kernel, which
          static payloads get unless PBGPU_XP_STATIC=0 or PBGPU_KERNEL=nopage (PBGPU_XP_FORCE=1
          overrides both).  Its part copies the stream's image (pb_ximg_body) unless the sequence was
          loaded under PBGPU_XP_IMG=0, PBGPU_XP_FORCE=1 or a PBGPU_KERNEL value the library
          recognises (gpf, stage, vstage, vpage keep the kind; an unknown value is the default).
A call fuses three distinct sequences, one of each kind."""
import collections
import math

import pb_configs as pc

HL = {"udp": 42, "tcp": 54, "icmp": 42}
PAGE = 4096
MAX_PART_BYTES = 1500000
ICMP_LENS = tuple(range(66, 127, 4))
TCP_LENS = (56, 60, 64)
WGTS = (512, 256)
BIG_FIRST = 2 ** 40 + 7
KERNEL_CHOICES = ("gpf", "stage", "vstage", "nopage", "linear", "vpage")  # the values PBGPU_KERNEL recognises


# ------------------------------------------------------------------ the rule
def payload_form(p):
    """(static, bytes) of a payload object; bytes None: the length varies or is drawn at load."""
    ln = p.get("length") or {}
    if "exact" in p:
        return True, len(p["exact"]) if p.get("isstring") else len(p["exact"].split())
    lo, hi = int(ln.get("min", 0)), int(ln.get("max", 0))
    return bool(p.get("isstatic")), lo if lo == hi else None


def frame_length(cfg):
    pls = cfg.get("payloads") or []
    if len(pls) != 1:
        return None
    n = payload_form(pls[0])[1]
    return None if n is None else HL[cfg["ip"]["protocol"]] + n


def page_kernel(cfg, env):
    """None, "whole" (pages of whole frames) or "cut" (frames cut at the page edges): the page
    kernel a one-payload sequence is given when it is loaded under env."""
    flen = frame_length(cfg)
    if flen is None or flen > 128 or env.get("PBGPU_KERNEL") == "linear":
        return None
    static = payload_form(cfg["payloads"][0])[0]
    force = env.get("PBGPU_XP_FORCE") == "1"
    if flen in (64, 128) and not force:
        return "whole"
    if flen % 2:
        return None
    if force:
        return "cut"
    if env.get("PBGPU_KERNEL") == "nopage" or not 52 <= flen <= 128:
        return None
    if flen % 4 == 0 and flen <= 64:
        return "cut"
    return "cut" if static and env.get("PBGPU_XP_STATIC") != "0" else None


def batch_kind(cfg, env):
    """0, or the kind (1, 2, 3) of the fused launch's part this sequence can be."""
    if env.get("PBGPU_BATCH") == "0":
        return 0
    pk = page_kernel(cfg, env)
    if pk is None:
        return 0
    flen, proto = frame_length(cfg), cfg["ip"]["protocol"]
    static = payload_form(cfg["payloads"][0])[0]
    if proto == "udp" and not static and pk == "whole" and flen == 64:
        return 1
    if proto == "tcp" and not static and pk == "cut" and flen <= 64 and flen % 4 == 0:
        return 2
    if proto == "icmp" and static and pk == "cut" and flen > 64 and flen % 4 == 2:
        return 3
    return 0


def has_image(cfg, env):
    """A kind-3 sequence's part runs pb_ximg_body: the image is built at load unless PBGPU_XP_IMG=0,
    PBGPU_XP_FORCE=1 or PBGPU_KERNEL names one of its kernels (any other value is the default).
    (The load also skips it for random ports, which an ICMP sequence cannot have.)  The load builds
    it for every static-payload ICMP sequence on the cut-frame page kernel, so also at the multiples
    of 4 (100 B), which have no fused form and use it only under PBGPU_XP_IMG=2, and under
    PBGPU_BATCH=0 (the planner, held against this in tests/test_batch_cases_cpu.py)."""
    static = page_kernel(cfg, env) == "cut" and payload_form(cfg["payloads"][0])[0]
    return (static and cfg["ip"]["protocol"] == "icmp" and env.get("PBGPU_XP_IMG") != "0"
            and env.get("PBGPU_XP_FORCE") != "1" and env.get("PBGPU_KERNEL") not in KERNEL_CHOICES)


# ------------------------------------------------------------------ page arithmetic
def page_params(flen, wgt, img, whole=False):
    """(slots per page, pages per workgroup, image period in pages) of a part at block size wgt;
    whole: kind 1 (a page holds 4096 / flen whole frames, one page per wave)."""
    period = flen // math.gcd(flen, PAGE)
    if whole:
        return PAGE // flen, wgt // 64, period
    slots = -(-PAGE // flen) + 1  # a frame that straddles the page's front edge, and one its back edge
    if img:
        return slots, wgt // 64, period
    return slots, min(9 if flen % 4 == 2 else 7, 512 // slots), period


def pages(flen, n):
    return -(-n * flen // PAGE)


def part_grid(flen, n, ppw, img):
    """(pages, workgroups in full groups of 8, tail workgroups, grid) of a part of n frames: full
    groups of 8 workgroups take 8 * ppw pages each, the tail workgroups the rest in order, ppw pages
    each; the image path rounds its grid up to whole groups instead."""
    nch = pages(flen, n)
    full = nch // (8 * ppw) * 8
    tail = -(-(nch - full * ppw) // ppw)
    if img:
        return nch, full, tail, -(-nch // (8 * ppw)) * 8
    return nch, full, tail, full + tail


def counts(flen, ppw, few=1):
    """The four count classes of a part, from page targets:
    a  less than one page (few: 1 or 5 frames);
    b  exactly one full group of 8 workgroups (8 ppw pages), ending inside the last page;
    c  one frame past that group's last page: the first tail workgroup, with one page;
    d  three full groups, 5 tail pages and a partial page."""
    g = 8 * ppw
    b = -(-g * PAGE // flen) - 1
    c = g * PAGE // flen + 1
    d = -(-(3 * g + 5) * PAGE // flen) + 1
    return few, b, c, d


# ------------------------------------------------------------------ configs
def udp_cfg(flen=64):
    cfg = pc.get("c2_udp_64")
    cfg["payloads"] = [{"length": {"min": flen - 42, "max": flen - 42}}]
    return cfg


def tcp_cfg(flen):
    cfg = pc.get("c4_tcp_syn")
    cfg["payloads"] = [{"length": {"min": flen - 54, "max": flen - 54}}]
    return cfg


def icmp_cfg(flen):
    cfg = pc.get("c5_icmp_echo")
    cfg["payloads"] = [{"exact": " ".join("%02x" % ((i * 29 + flen) & 255) for i in range(flen - 42))}]
    return cfg


def tcp_env(flen):
    return {"PBGPU_XP_FORCE": "1"} if flen == 64 else {}


# ------------------------------------------------------------------ the case table
# parts: ((cfg, env), ...) of slots 0, 1, 2 (kinds 1, 2, 3); lens, ppw: per part
Case = collections.namedtuple("Case", "id index wgt img tcp_len icmp_len parts lens ppw")
# one batch: order: the parts' order in the call; sizes[k] = (first_iter, n_iter) of slot k
Batch = collections.namedtuple("Batch", "order sizes")
ORDERS = ((2, 0, 1), (1, 2, 0), (0, 2, 1), (2, 1, 0))


def make_case(index, wgt, img, tcp_len, icmp_len):
    parts = ((udp_cfg(), {}), (tcp_cfg(tcp_len), tcp_env(tcp_len)),
             (icmp_cfg(icmp_len), {} if img else {"PBGPU_XP_IMG": "0"}))
    ppw = (page_params(64, wgt, False, whole=True)[1], page_params(tcp_len, wgt, False)[1],
           page_params(icmp_len, wgt, img)[1])
    return Case("w%d_%s_tcp%d_icmp%d" % (wgt, "img" if img else "noimg", tcp_len, icmp_len), index, wgt, img, tcp_len,
                icmp_len, parts, (64, tcp_len, icmp_len), ppw)


def _table():
    out = []
    for wgt in WGTS:
        for img in (True, False):
            for li, icmp_len in enumerate(ICMP_LENS):
                out.append(make_case(len(out), wgt, img, TCP_LENS[li % 3], icmp_len))
    return out


CASES = _table()


def batches(case):
    """Four batches: in batch r part k takes count class (r + k + index) mod 4, so a part sees each
    class once and the parts of a batch differ.  First iterations are odd and differ per part;
    batch 2 starts at 2^40 + 7."""
    out = []
    for r in range(4):
        sizes = []
        for k in range(3):
            few = 1 if (case.index + k) % 2 else 5
            n = counts(case.lens[k], case.ppw[k], few)[(r + k + case.index) % 4]
            first = BIG_FIRST + 2 * k if r == 2 else 2 * (1009 * r + 37 * k + case.index) + 1
            sizes.append((first, n))
        out.append(Batch(ORDERS[(r + case.index) % 4], tuple(sizes)))
    return out


# ------------------------------------------------------------------ near misses
# (name, slot it replaces, cfg, env): each has no fused form next to two valid partners
def _two_payloads():
    cfg = udp_cfg()
    cfg["payloads"] = [{"length": {"min": 22, "max": 22}}, {"length": {"min": 22, "max": 22}}]
    return cfg


def _icmp_random(flen):
    cfg = pc.get("c5_icmp_echo")
    cfg["payloads"] = [{"length": {"min": flen - 42, "max": flen - 42}}]
    return cfg


NEAR_MISSES = [
    ("udp60", 0, udp_cfg(60), {}),
    ("udp64_forced", 0, udp_cfg(64), {"PBGPU_XP_FORCE": "1"}),
    ("tcp58", 1, tcp_cfg(58), {}),
    ("tcp64_unforced", 1, tcp_cfg(64), {}),
    ("icmp100", 2, icmp_cfg(100), {}),
    ("icmp64", 2, icmp_cfg(64), {}),
    ("icmp98_random", 2, _icmp_random(98), {}),
    ("icmp98_nostatic", 2, icmp_cfg(98), {"PBGPU_XP_STATIC": "0"}),
    ("two_payloads", 0, _two_payloads(), {}),
]
