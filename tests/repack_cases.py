"""The cases of the repack writers' several-pages-per-workgroup tests, shared by
test_gpu_repack_pages.py (which runs them on the GPU under PBGPU_RP_PER) and test_repack_pages_cpu.py
(which shows from the references' record offsets that they reach the page loop's carries).

A case is a source (frames built here from a plan, or one of the existing zoos), a writer with one
option set, a sub-range and the pages per workgroup it runs at.  `geometry()` walks a launch of `per`
pages per workgroup over the reference's records the way the kernels' page loops do and counts what
that launch meets: window moves, carried pages, pages in which no record starts, record edges on page
edges and where the output ends."""
import collections
import functools
import os
import re

import numpy as np

import pyencap
import pyfrag
import pypcap
import pyseg
import pyxlat
import seg_frames as sf
import test_gpu_encap as tge
import test_gpu_frag as tgf
import test_gpu_pcap as tgp
import test_gpu_seg as tgs
import test_gpu_xlat as tgx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGE = 4096
PERS = (2, 3, 32)  # the smallest with a carry, one that divides no page count here, production's
WRITERS = ("pcap", "encap", "frag", "seg", "xlat")

# the option sets: what each writer's check helper takes
OPTS = {
    "pcap": {"hdr": dict(t0_ns=tgp.T0, step_ps=tgp.STEP, file_header=True),
             "nohdr": dict(t0_ns=tgp.T0, step_ps=tgp.STEP, file_header=False, nsec=True)},
    "encap": dict(tge.MODES),  # vlan, vxlan
    "frag": {"1500": (1500, False), "576df": (576, True), "576": (576, False), "1500df": (1500, True)},  # mtu, ignore_df
    "seg": {"8": (8, 0), "536f1": (536, 1), "1460f2": (1460, 2), "1460f3": (1460, 3), "536": (536, 0),
            "1460": (1460, 0)},  # mss, flags
    "xlat": dict(tgx.OPTS),  # label, hash
}
SHORT = {"pcap": 1, "encap": 14, "frag": 14, "seg": 14, "xlat": 42}  # the source frame of the shortest record
WIN_OF = {"pcap": "PB_PC_WIN", "encap": "PB_EN_WIN", "frag": "PB_FG_WIN", "seg": "PB_FG_WIN", "xlat": "PB_XL_WIN"}
HREC_OF = {"pcap": None, "encap": "PB_EN_HREC", "frag": "PB_FG_HREC", "seg": "PB_FG_HREC", "xlat": "PB_XL_HREC"}


# ------------------------------------------------------------------ the device's sizes
@functools.lru_cache(maxsize=None)
def device_sizes():
    """The PB_* object-like macros of csrc/pb_device.h that evaluate to integers, by name."""
    text = open(os.path.join(ROOT, "pb-af-xdp_amd", "csrc", "pb_device.h")).read()
    defs = dict(re.findall(r"^#define[ \t]+(PB_\w+)[ \t]+([^/\n]+?)[ \t]*(?://.*)?$", text, re.M))
    out = {}

    def val(name):
        if name not in out:
            expr = re.sub(r"\bPB_\w+\b", lambda m: str(val(m.group(0))), defs[name])
            out[name] = int(eval(re.sub(r"\b(\d+)u\b", r"\1", expr), {"__builtins__": {}}))
        return out[name]

    return {n: val(n) for n in set(WIN_OF.values()) | {h for h in HREC_OF.values() if h}}


def biggest(writer, oname):
    """The longest source frame the writer takes under the option set."""
    if writer == "encap":
        return 65535 - tge.P_OF[tge.MODES[oname][0]]
    return 65515 if writer == "xlat" else 65535


# ------------------------------------------------------------------ frames
@functools.lru_cache(maxsize=None)
def make(writer, kind, L, i):
    """Source frame i of a plan, L bytes.  kind "s": one of 61 short frames; "ip": a frame the writer
    transforms; "df": the same with DF set (the fragmenter); "copy": one the fragmenter and the
    segmenter copy whole whatever its length (no IPv4 ethertype)."""
    if writer in ("pcap", "encap"):
        return np.random.default_rng(100000 + i).integers(0, 256, L, dtype=np.uint8).tobytes()
    if writer == "frag":
        if kind == "copy":
            return tgf.ip_frame(L, i, ethertype=b"\x88\xb5")
        return tgf.ip_frame(L, i, fo=0x4000 if kind == "df" else 0)
    if writer == "seg":
        if kind == "copy" or L < 42:
            f = bytearray(sf.payload(L, i))
            f[12:14] = b"\x88\xb5"
            return bytes(f)
        H = (0, 20, 24, 60)[i % 4]  # UDP, and TCP with 20, 24 and 60 header bytes
        if H == 0 or L < 34 + H:
            return tgs.frame_of("udp", L, i)
        return sf.tcp(L - 34 - H, i, ident=i, seq=0xFFFFFF00 + i if i % 5 == 0 else i * 977, flags=i & 0xFF, H=H)
    kinds = ("udp", "tcp", "icmp") if L >= 54 else ("udp", "icmp")
    return pyxlat.frame4(kinds[i % len(kinds)], L, np.random.default_rng(100000 + i), icmp_type=8 * (i & 1))


def records(writer, oname, frames):
    """The writer's output records of `frames` under the option set, from its Python definition (a
    pcap record is a frame's 16-B header and its bytes; the file header is no record)."""
    o = OPTS[writer][oname]
    if writer == "pcap":
        return [pypcap.pcap_stream([f], 0, 0, 0, False) for f in frames]  # for their lengths: the stamps are not these
    if writer == "encap":
        return [tge.ref_frame(f, *o) for f in frames]
    if writer == "frag":
        return pyfrag.fragment_all(frames, *o)[0]
    if writer == "seg":
        return pyseg.segment_all(frames, *o)[0]
    return tgx.ref_frames(frames, o)


def header_bytes(writer, oname):
    return 24 if writer == "pcap" and OPTS["pcap"][oname]["file_header"] else 0


def build(writer, oname, plan):
    """The frames of a plan: ("s", count) short frames, ("f", L, count[, kind]) frames of L bytes,
    ("out", B) one frame that gives a record of B bytes, ("page", k), ("total", T) and ("wg", k) filler
    frames up to output byte 4096 k, byte T, and the next page whose index is a multiple of k, exactly
    (filler and "out" frames are ones the writer does not split: each adds its own length and a
    constant)."""
    frames, done, pos = [], 0, header_bytes(writer, oname)
    add = {"pcap": 16, "encap": tge.P_OF[tge.MODES[oname][0]] if writer == "encap" else 0, "frag": 0, "seg": 0,
           "xlat": 20}[writer]
    lo, hi = max(SHORT[writer], 14) + add, 1000 + add
    for item in plan:
        if item[0] == "s":
            frames += [make(writer, "s", SHORT[writer], i % 61) for i in range(item[1])]
        elif item[0] == "f":
            kind = item[3] if len(item) > 3 else "ip"
            frames += [make(writer, kind, item[1], len(frames) + i) for i in range(item[2])]
        elif item[0] == "out":
            frames.append(make(writer, "copy", item[1] - add, len(frames)))
        else:
            pos += sum(len(r) for r in records(writer, oname, frames[done:]))
            target = item[1] * PAGE if item[0] == "page" else item[1]
            if item[0] == "wg":
                target = -(-(pos + lo) // (item[1] * PAGE)) * item[1] * PAGE
            done, left = len(frames), target - pos
            assert left >= lo, (writer, oname, item, pos)
            while left:
                take = hi if left - hi >= lo else left
                frames.append(make(writer, "copy", take - add, len(frames)))
                left -= take
            pos += sum(len(r) for r in records(writer, oname, frames[done:]))
            done = len(frames)
            assert pos == target, (writer, oname, item, pos)
    return frames


def runs_plan(writer, oname):
    """Runs of the shortest records between long ones.  A record starts on page 5's first byte and one
    ends on page 11's last (5 and 11 are no multiples of 2, 3 or 32, so neither page is a workgroup's
    first); 6,000 short records cover 20 pages and more; records of 1514 B and 9 KB straddle page
    ends; records longer than a page come before short runs of several lengths, so that a window
    runs out on the page after one; the longest frame covers 15 whole pages."""
    plan = [("s", 200), ("page", 5), ("s", 100), ("f", 9043, 1, "copy"), ("page", 12), ("f", 1514, 3),
            ("s", 6000), ("f", 9043, 1, "copy"), ("s", 700), ("f", 9043, 1), ("s", 350), ("f", 3000, 4, "df"),
            ("f", 1514, 60), ("f", 9043, 6), ("s", 330), ("f", biggest(writer, oname), 1), ("s", 3000)]
    for i, c in enumerate((150, 290, 310, 500, 800, 260, 330, 420)):
        plan += [("f", 4200 + 517 * i, 1, "copy"), ("s", c)]
    # a record of a page and 100 B from the first byte of a workgroup of 3 pages, then short ones: the
    # window runs out on the workgroup's third page, the one after the page the record ends in
    return plan + [("f", 1621, 30), ("wg", 3), ("out", PAGE + 100), ("s", 400), ("f", 1621, 2), ("s", 100)]


RAGGED = ("exact", "minus16", "plus16", "middle")


def ragged_total(per, how):
    """Output bytes: whole workgroups of `per` pages (48 KiB at least, and two workgroups), 16 B less,
    16 B more (a last workgroup of one page), and one page and 1005 B more (the output ends in the
    next workgroup's second page: a middle one from 3 pages per workgroup on)."""
    m = max(2, -(-12 // per))
    return m * per * PAGE + {"exact": 0, "minus16": -16, "plus16": 16, "middle": PAGE + 1005}[how]


RAGGED_BASE = [("s", 200), ("f", 1514, 4), ("f", 9043, 1), ("s", 100)]

# fixed-length sources: (length or None for the writer's longest, option set, first frame)
FIXED = {
    "pcap": [(14, "hdr", 0), (60, "nohdr", 0), (60, "hdr", 3), (64, "hdr", 0), (1500, "nohdr", 0), (1621, "hdr", 0),
             (1621, "nohdr", 3), (9043, "hdr", 0), (None, "nohdr", 0), (None, "hdr", 1)],
    "encap": [(14, "vlan", 0), (14, "vxlan", 0), (60, "vxlan", 0), (60, "vlan", 3), (64, "vlan", 0), (1500, "vxlan", 0),
              (1621, "vlan", 0), (1621, "vxlan", 3), (9043, "vxlan", 0), (None, "vlan", 0), (None, "vxlan", 1)],
    # 14 to 1500 B at mtu 1500 and 14 to 64 B at mtu 576 take pb_frag_copy_kernel
    "frag": [(14, "1500", 0), (60, "576", 0), (60, "1500", 3), (64, "1500df", 0), (1500, "1500", 0), (1500, "576df", 0),
             (1621, "1500", 0), (1621, "576", 3), (9043, "1500df", 0), (9043, "576", 0), (None, "1500", 0),
             (None, "576df", 1)],
    # 14 to 1500 B at mss 1460 and 14 B at any mss take the copy; 60 B at mss 8 is three segments
    "seg": [(14, "1460", 0), (14, "8", 0), (60, "1460f2", 0), (60, "1460", 3), (60, "8", 0), (64, "536", 0),
            (1500, "1460f3", 0), (1500, "536f1", 0), (1621, "1460", 0), (1621, "536", 3), (9043, "1460f2", 0),
            (9043, "536f1", 0), (None, "1460", 0), (None, "8", 1)],
    "xlat": [(60, "label", 0), (60, "hash", 3), (64, "hash", 0), (1500, "label", 0), (1621, "hash", 0), (1621, "label", 3),
             (9043, "label", 0), (None, "hash", 0), (None, "label", 1)],
}
RUNS_OPTS = {"pcap": ("hdr", "nohdr"), "encap": ("vlan", "vxlan"), "frag": ("1500", "576df"),
             "seg": ("8", "536f1", "1460f2"), "xlat": ("label", "hash")}
ZOO_OPTS = {"pcap": ("hdr", "nohdr"), "encap": ("vlan", "vxlan"), "frag": ("576", "1500df"), "seg": ("1460f3", "536"),
            "xlat": ("label", "hash")}

Case = collections.namedtuple("Case", "writer kind oname arg first pers")


def case_id(c):
    return "-".join(str(x) for x in (c.writer, c.kind, c.oname) + (() if c.arg is None else (c.arg,)) +
                    (("first%d" % c.first,) if c.first else ()))


def _cases():
    out = []
    for w in WRITERS:
        out += [Case(w, "runs", o, None, 0, PERS) for o in RUNS_OPTS[w]]
        out += [Case(w, "zoo", o, None, 0, PERS) for o in ZOO_OPTS[w]]
        out += [Case(w, "fixed", o, L or biggest(w, o), first, PERS) for L, o, first in FIXED[w]]
        ragged_opts = RUNS_OPTS[w][-2:] if w == "seg" else RUNS_OPTS[w]  # the ragged base at mss 8 is 7 times as long
        for per in PERS:
            out += [Case(w, "ragged%d" % per, ragged_opts[i % len(ragged_opts)], how, 0, (per,))
                    for i, how in enumerate(RAGGED)]
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def source(c):
    """(frames, fixed length or 0, first, n) of a case: the buffer's frames and the range that runs."""
    w = c.writer
    if c.kind == "runs":
        frames = build(w, c.oname, runs_plan(w, c.oname))
    elif c.kind == "zoo":
        if w == "pcap":
            frames = tgp.split(*tgp.random3000_frames())
        elif w == "encap":
            frames = tge.split(*tge.random3000_frames())
        elif w == "frag":
            frames = tgf._mixed_frames()
        elif w == "seg":
            frames = tgs._mixed_frames()
        else:
            frames = tgx.mixed1000_frames()
    elif c.kind == "fixed":
        L = c.arg
        n = max(3, -(-40 * PAGE // L)) + c.first + 1  # 40 pages and more; the range leaves out the last frame too
        frames = [make(w, "s", L, i % 61) if L == SHORT[w] else make(w, "ip", L, i) for i in range(n)]
        return frames, L, c.first, n - c.first - (1 if c.first else 0)
    else:
        per = int(c.kind[len("ragged"):])
        frames = build(w, c.oname, RAGGED_BASE + [("total", ragged_total(per, c.arg))])
    return frames, 0, 0, len(frames)


@functools.lru_cache(maxsize=None)
def reference(c):
    """The output records of the case's range."""
    frames, _, first, n = source(c)
    return records(c.writer, c.oname, frames[first:first + n])


def windowed(c):
    """Whether the case's launch keeps a window of record positions in LDS: every variable-length
    source; a fixed-length one only in the fragmenter and the segmenter, where some frame splits."""
    flen = source(c)[1]
    if not flen:
        return True
    if c.writer == "frag":
        return flen > OPTS["frag"][c.oname][0] + 14
    if c.writer == "seg":
        return flen - 42 > OPTS["seg"][c.oname][0]
    return False


def copy_path(c):
    """A fixed-length source of the fragmenter or the segmenter none of whose frames can split."""
    return c.writer in ("frag", "seg") and bool(source(c)[1]) and not windowed(c)


# ------------------------------------------------------------------ what a launch meets
Geometry = collections.namedtuple(
    "Geometry", "total npages grid multi moves move_pages moves_after_long carried nostart start0 end4095 "
    "end_page last_pages max_touch")


def geometry(rec_lens, hdr, per, win):
    """A launch of `per` pages per workgroup over records of these lengths behind `hdr` header bytes,
    with a window of `win` record positions (None: no window), as the page loops run it.

    multi: workgroups with two pages and more; moves: window moves per workgroup; move_pages: the
    pages' indices; moves_after_long: the moves on a page in whose predecessor a record longer than a
    page ends; carried: lengths of the records that hold the first byte of a page that is no
    workgroup's first, started before it, and met no move there; nostart: such pages in which no
    record starts; start0 / end4095: records that start on the first / end on the last byte of such a
    page; end_page: the page of its workgroup in which the output ends; last_pages: the last
    workgroup's pages; max_touch: the most records with a byte in one page."""
    lens = np.asarray(rec_lens, dtype=np.int64)
    P = hdr + np.concatenate([[0], np.cumsum(lens)])  # record j starts at P[j]; P[m] is the output's end
    m, total = len(lens), int(P[-1])
    end16 = (total + 15) & ~15
    npages = (end16 + PAGE - 1) // PAGE
    grid = -(-npages // per)
    starts, ends = P[:-1], P[1:] - 1  # first and last byte of each record
    later = lambda page: page % per != 0  # no workgroup's first page
    has_start = np.zeros(npages, dtype=bool)
    has_start[starts // PAGE] = True
    nostart = [k for k in range(npages) if later(k) and not has_start[k] and k * PAGE < total]
    start0 = int(sum(1 for s in starts[starts % PAGE == 0] if later(int(s) // PAGE)))
    end4095 = int(sum(1 for e in ends[ends % PAGE == PAGE - 1] if later(int(e) // PAGE)))
    touch = np.searchsorted(starts, (np.arange(npages) + 1) * PAGE - 1, "right") - \
        np.searchsorted(ends, np.arange(npages) * PAGE, "left")
    holder = lambda p: max(0, int(np.searchsorted(P, p, "right")) - 1)  # the record holding byte p
    moves, move_pages, after_long, carried = [], [], 0, []
    for g in range(grid):
        j0, have, mv = holder(g * per * PAGE), False, 0
        for it in range(per):
            p = (g * per + it) * PAGE
            if p >= end16:
                break
            moved = False
            if win is not None:
                last = j0 + win - 1  # past the output's end the window holds no position: it never runs out there
                if not have or (last <= m and int(P[last]) <= p + PAGE - 1):
                    if have:
                        moved, mv, j0 = True, mv + 1, holder(p)
                        move_pages.append(g * per + it)
                        a, b = np.searchsorted(ends, [p - PAGE, p])
                        after_long += bool((lens[a:b] > PAGE).any())
                    have = True
            if it and not moved and p < total:
                j = holder(p)
                if int(P[j]) < p:
                    carried.append(int(lens[j]))
        moves.append(mv)
    multi = sum(1 for g in range(grid) if min(npages, (g + 1) * per) - g * per >= 2)
    return Geometry(total, npages, grid, multi, moves, move_pages, after_long, carried, nostart, start0, end4095,
                    (npages - 1) % per, npages - (grid - 1) * per, int(touch.max()) if npages else 0)


@functools.lru_cache(maxsize=None)
def case_geometry(c, per):
    win = device_sizes()[WIN_OF[c.writer]] if windowed(c) else None
    return geometry([len(r) for r in reference(c)], header_bytes(c.writer, c.oname), per, win)
