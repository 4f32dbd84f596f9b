"""Cases that take pb_scan_blocks (csrc/pbgpu_kernels.hip) past its first pass, shared by
test_gpu_scan_passes.py (which runs them on the GPU) and test_scan_cases_cpu.py (which holds the
arithmetic and the references here against the sources, the planner, the oracle, pyfrag and pyseg).

pb_scan_blocks is one workgroup that scans its entries in place in passes of PASS = 1024 * IT entries
and carries a running sum from pass to pass.  Its callers and what one entry is:

  pbk_launch_vst_lengths   the group sum of PB_VL_GRP build workgroups of wgf frames each
  pbk_launch_lengths       PB_SCAN_FRAMES_PER_BLOCK frames (the 3-pass scan)
  pbk_launch_frag, _seg    a row of PB_FG_WT source frames (segment: two scans, records and bytes)

Every case here has PASS + 1025 entries: 1,025 of them in the second pass, the last one ragged (5
frames of a build, 77 frames of a cut's last row); each cut runs a second time without its source's
first 129 frames, over PASS + 1024 rows that start between the source's, the last of 204 frames.
The constants are read from the sources, and the frame counts are written out, so a changed
constant changes entries() and fails test_scan_cases_cpu.py; no case falls back into one pass
unnoticed.

Not covered: pb_vpage_kernel's length pass has wgf = 256 fixed, so a second pass needs more than
PASS * PB_VL_GRP * 256 = 2^26 frames (about 5 GB of 74-B frames); and no case reaches a third pass.

No GPU code here.  The references are numpy: a frame's length is 42 + lo + r0 % (hi - lo + 1) with r0
the first draw of its iteration (field_cases.np_seed / np_rand_r), and the fragmenter's and the
segmenter's records follow from the lengths alone for these sources (UDP over IPv4 without options,
DF clear, not a fragment), per the definitions in include/pbgpu.h."""
import collections
import copy
import functools
import os
import re

import numpy as np

import field_cases as fc
import pb_configs as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pb-af-xdp_amd", "csrc")
SLOT = 5
FIRST_ITER = 1000003  # odd, non-zero
WINDOW = 64           # frames of a byte-compared window
IN_PASS_2 = 1025      # entries of a case past the first pass (1024 in a cut's second run)


# ------------------------------------------------------------------ the sources' constants
def _int(expr):
    """A C integer expression of literals (u suffixes, + - * / and parentheses)."""
    expr = re.sub(r"\b(\d+)[uU]?[lL]{0,2}\b", r"\1", expr).replace("/", "//")
    assert re.fullmatch(r"[\d\s()+\-*/]+", expr), expr
    return int(eval(expr, {"__builtins__": {}}))


def _define(text, name, where):
    m = re.search(r"^#define[ \t]+%s[ \t]+([^/\n]+?)[ \t]*(?://.*)?$" % name, text, re.M)
    assert m, "%s: no #define %s" % (where, name)
    return _int(m.group(1))


def read_constants(csrc=CSRC):
    """PASS and the PB_* sizes the launch arithmetic uses, from the sources under `csrc`."""
    def text(name):
        with open(os.path.join(csrc, name)) as f:
            return f.read()

    kernels, device, plan, host = (text(n) for n in ("pbgpu_kernels.hip", "pb_device.h", "pb_plan.h", "pbgpu.cpp"))
    m = re.search(r"void pb_scan_blocks\(.*?\{\s*constexpr uint32_t IT = (\d+), PASS = 1024 \* IT;", kernels, re.S)
    assert m, "pb_scan_blocks: no `constexpr uint32_t IT = ..., PASS = 1024 * IT;`"
    out = {"IT": int(m.group(1)), "PASS": 1024 * int(m.group(1))}
    out["PB_SCAN_FRAMES_PER_BLOCK"] = _define(host, "PB_SCAN_FRAMES_PER_BLOCK", "pbgpu.cpp")
    # (the kernels of the 3-pass scan take 256 * PB_SCAN_ITEMS frames per workgroup: the same number)
    out["PB_SCAN_ITEMS"] = _define(kernels, "PB_SCAN_ITEMS", "pbgpu_kernels.hip")
    for name in ("PB_VL_GRP", "PB_FG_WT", "PB_FG_CB"):
        out[name] = _define(device, name, "pb_device.h")
    out["PB_VST_SCAN_MIN_WGF"] = _define(plan, "PB_VST_SCAN_MIN_WGF", "pb_plan.h")
    return out


@functools.lru_cache(maxsize=None)
def constants():
    return read_constants()


# ------------------------------------------------------------------ the cases
# scan: "l2" (pbk_launch_vst_lengths) or "3pass" (pbk_launch_lengths); wgf: the build workgroup's
# frames, which is also the length pass's (pb_plan_len_wgf) unless the scan is the 3-pass one
Build = collections.namedtuple("Build", "id lo hi env kernel scan wgf frames")
BUILDS = [
    Build("vline_wgf32", 32, 33, {"PBGPU_VL_WGF": "32"}, "pb_vline_kernel", "l2", 32, (1 << 23) + (1 << 20) + 5),
    Build("vstage_wgf32", 0, 40, {"PBGPU_KERNEL": "vstage", "PBGPU_WGF": "32"}, "pb_vstage_kernel", "l2", 32,
          (1 << 23) + (1 << 20) + 5),
    Build("vstage_3pass", 0, 40, {"PBGPU_KERNEL": "vstage", "PBGPU_VST_SCAN": "3pass"}, "pb_vstage_kernel", "3pass", 252,
          (1 << 24) + (1 << 21) + 5),
]
BUILD = {b.id: b for b in BUILDS}

# the cut source: one pb_vline_kernel build in its default shape, 74..138-B frames
SRC = Build("cut_source", 32, 96, {}, "pb_vline_kernel", "l2", 252, (1 << 21) + (1 << 18) + 77)
SKIP = 129  # the second run of each cut leaves out this many frames: its rows start between the source's
Cut = collections.namedtuple("Cut", "id kind opt first n")
CUTS = [Cut("%s_%s" % (name, run), kind, opt, first, SRC.frames - first)
        for name, kind, opt in (("frag_mtu68", "frag", 68), ("seg_mss32", "seg", 32))
        for run, first in (("whole", 0), ("first%d" % SKIP, SKIP))]
CUT = {c.id: c for c in CUTS}


def _ceil(a, b):
    return -(-a // b)


def entries(case, frames=None):
    """The entries pb_scan_blocks gets for a case (of `frames` frames instead of the case's own):
    the launch arithmetic of pbgpu_build (csrc/pbgpu.cpp) and cut_count, restated."""
    k = constants()
    if isinstance(case, Cut):
        return _ceil(case.n if frames is None else frames, k["PB_FG_WT"])  # rows
    nf = case.frames if frames is None else frames
    if case.scan == "3pass":
        return _ceil(nf, k["PB_SCAN_FRAMES_PER_BLOCK"])  # nblocks
    return _ceil(_ceil(nf, case.wgf), k["PB_VL_GRP"])  # n_l2


def in_pass_2(case):
    """The entries a case must have past the first pass: 1,025, the last one ragged (a cut that leaves
    out its source's first SKIP frames: 1,024, the last row 204 frames)."""
    return IN_PASS_2 - (1 if isinstance(case, Cut) and case.first else 0)


def frames_per_entry(case):
    k = constants()
    if isinstance(case, Cut):
        return k["PB_FG_WT"]
    return k["PB_SCAN_FRAMES_PER_BLOCK"] if case.scan == "3pass" else case.wgf * k["PB_VL_GRP"]


def boundary(case):
    """The first frame (of the case's own range) of scan entry PASS, the second pass's first."""
    return constants()["PASS"] * frames_per_entry(case)


def windows(case):
    """The frame ranges (first, count) whose bytes are compared: from frame 0, WINDOW / 2 on either
    side of the second pass's first frame (of the middle frame where one pass does, as in the cut
    source), and the last WINDOW frames."""
    n, b = (case.n if isinstance(case, Cut) else case.frames), boundary(case)
    if entries(case) <= constants()["PASS"]:
        b = n // 2
    assert WINDOW < b - WINDOW // 2 and b + WINDOW // 2 < n - WINDOW
    return [(0, WINDOW), (b - WINDOW // 2, WINDOW), (n - WINDOW, WINDOW)]


def config(case):
    """c3_udp_var with one random payload of lo..hi bytes."""
    cfg = copy.deepcopy(pc.get("c3_udp_var"))
    cfg["payloads"] = [{"length": {"min": case.lo, "max": case.hi}}]
    return cfg


# ------------------------------------------------------------------ references
def lengths(lo, hi, first_iter, n, slot=SLOT, seed_base=pc.SEED_BASE):
    """The lengths of the n frames from iteration first_iter of a UDP sequence with one random payload
    of lo..hi bytes (int64)."""
    with np.errstate(over="ignore"):
        r0 = fc.np_rand_r(fc.np_seed(seed_base, slot, np.arange(first_iter, first_iter + n, dtype=np.uint64)))[0]
    return (42 + lo + r0 % np.uint32(hi - lo + 1)).astype(np.int64)


def offsets_of(lens):
    """n + 1 offsets of packed records of these lengths (uint64)."""
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    return off


def build_lengths(case, frames=None, first_iter=FIRST_ITER):
    return lengths(case.lo, case.hi, first_iter, case.frames if frames is None else frames)


CutRef = collections.namedtuple("CutRef", "K first_rec out_len off counts")


def cut_reference(kind, opt, L):
    """The fragmenter's (kind "frag", opt = mtu) or the segmenter's (kind "seg", opt = mss) output for
    source frames of lengths L, every one UDP over IPv4 without options, DF clear: K records per
    frame, each frame's first record, every record's length, the n_out + 1 offsets, and the result
    struct's fields."""
    L = np.asarray(L, dtype=np.int64)
    if kind == "frag":
        cut, hdr = (opt - 20) & ~7, 34   # C; a fragment is src[0:34] and its data
        split = L - 14 > opt
    else:
        cut, hdr = opt, 42               # mss; a segment is Ethernet, IPv4, UDP and its payload
        split = L - 42 > opt
    data = L - hdr
    K = np.where(split, -(-data // cut), 1)
    first_rec = np.zeros(len(L) + 1, dtype=np.int64)
    np.cumsum(K, out=first_rec[1:])
    n_out = int(first_rec[-1])
    i = np.arange(n_out, dtype=np.int64) - np.repeat(first_rec[:-1], K)  # a record's index within its frame
    out_len = np.where(np.repeat(split, K), hdr + np.minimum(cut, np.repeat(data, K) - i * cut), np.repeat(L, K))
    counts = dict(n_in=len(L), n_out=n_out, n_other=0, out_bytes=int(out_len.sum()),
                  out_min_len=int(out_len.min()) if n_out else 0, out_max_len=int(out_len.max()) if n_out else 0)
    if kind == "frag":
        counts.update(n_split=int(split.sum()), n_df=0)
    else:
        counts.update(n_split_tcp=0, n_split_udp=int(split.sum()))
    return CutRef(K, first_rec, out_len, offsets_of(out_len), counts)


@functools.lru_cache(maxsize=None)
def source_lengths():
    L = build_lengths(SRC)
    L.setflags(write=False)
    return L


def cut_case_reference(case):
    return cut_reference(case.kind, case.opt, source_lengths()[case.first:case.first + case.n])


# ------------------------------------------------------------------ the comparison the GPU tests use
def assert_offsets(got, want, what):
    """got == want, entry by entry; the failure names the first entry that differs."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: %d offsets, want %d" % (what, len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert not len(bad), "%s: %d offsets differ, the first at entry %d: %d, want %d" % (
        what, len(bad), bad[0], got[bad[0]], want[bad[0]])


def drop_carry(off, at):
    """What a scan that lost its carry into the second pass would give: every offset from entry `at`
    on (the second pass's first frame or record) less the sum of all before it."""
    out = np.array(off, dtype=np.uint64)
    out[at:] -= out[at]
    return out
