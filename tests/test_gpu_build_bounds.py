"""What a build may write (the contract next to pbgpu_build in include/pbgpu.h), a buffer's state
across every kind of use, and iteration numbers at the edges of their range; everything bit-exact
against the CPU oracle.

1. Guarded windows.  A backing buffer B is painted 0xA5 and the build goes through an alias of its
   pbgpu_frames struct whose data starts a 64-KiB guard into B and whose capacities are the least
   build_check accepts: capacity_frames == n_frames, capacity_bytes == round16(n_frames * max_flen).
   B is then read back whole: the front guard, the stream, the pad bytes up to the next multiple of
   16 (zeros or untouched), and 0xA5 in every byte after that, the rest of the window and the back
   guard.  B's offsets hold a ramp: a variable-length build keeps the entries past
   offsets[n_frames], a fixed-length one all of them.  One case per build kernel family, at frame
   counts around its store unit (16-B chunk, 128-B line, 4-KiB page) and one frame past a full
   group of 8 workgroups.  test_case_table_keeps_its_edges (no GPU) pins that the table still
   holds those edges.
2. One buffer through a packed build, a fixed build, a 64-bit-offsets build, an upload, another
   packed shape, an encapsulation, the page writer and an empty build, checked after every step.
3. Builds whose iteration range straddles 2^32 (2^33) and ends at the top of the legal range, and
   the refusal one past it."""
import collections
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_binding as ob
import pb_configs as pc
import pbgpu
import pyencap
from pbgpu import ENCAP_VXLAN, FrameBuffer, Frames, GpuContext, Sequence

gpu = pytest.mark.gpu

GUARD = 64 << 10  # bytes of B before and after the window (a multiple of 4096: the page kernels keep their page path)
PAINT = 0xA5
TAIL = 64  # offsets entries of B past offsets[n_frames], holding a ramp
SLOT = 5
FIRST = 1000003
SEED_K = (1 << 48) - 1  # PB_STATIC_SEED_K (include/pb_config.h): first_iter + n_iter stays below it
EINVAL = -22
VX = dict(dst_mac=bytes.fromhex("0200000000a2"), src_mac=bytes.fromhex("0200000000a1"), src_ip=bytes([192, 0, 2, 1]),
          dst_ip=bytes([198, 51, 100, 2]), vni=0x123456)


def r16(x):
    return (x + 15) & ~15


# ------------------------------------------------------------------ the case table
def _pl(base, lo, hi=None):
    """Config `base` with one random payload of lo..hi bytes."""
    cfg = copy.deepcopy(pc.get(base))
    cfg["payloads"] = [{"length": {"min": lo, "max": lo if hi is None else hi}}]
    return cfg


def _udp(flen):
    return _pl("c2_udp_64", flen - 42)


def _static(base, nbytes):
    cfg = copy.deepcopy(pc.get(base))
    cfg["payloads"] = [{"exact": " ".join("%02X" % (i * 7 & 255) for i in range(nbytes))}]
    return cfg


# counts: iterations per build, or (first_iter, iterations); unit: the family's store unit in bytes
Case = collections.namedtuple("Case", "id family cfg env rule counts")
UNIT = {"pb_xsmall_kernel": 4096, "pb_xpage_kernel": 4096, "pb_ximg_kernel": 4096, "pb_small_kernel": 16,
        "pb_fstage_kernel": 128, "pb_stage_kernel": 16, "pb_vstage_kernel": 16, "pb_vline_kernel": 128,
        "pb_vpage_kernel": 4096, "pb_gpf_kernel": 16}
VPAGE, VSTAGE = {"PBGPU_KERNEL": "vpage"}, {"PBGPU_KERNEL": "vstage"}
TCP60 = (1, 4, 5, 68, 69, 1024, 1025, 3822, 3823)  # 68 | 69 frames: the first page's edge; 1024: 15 pages; 3822 | 3823: 8 x 7 pages
ICMP98 = (1, 5, 8, 41, 42, 1337, 1338, 2048, 2049, 3009, 3010)  # 2048: 49 pages; 1337 | 1338: 32 pages; 3009 | 3010: 8 x 9 pages
# (first_iter, n) of 74..75-B frames whose stream is exactly 7 lines (896 B) and exactly 1 and 2 pages
# (found with the oracle; test_case_table_keeps_its_edges checks them)
V33_LINES = (1000152, 12)
V33_PAGE = (1000004, 55)
V33_PAGES = (1000247, 110)
CASES = [
    # pages of whole frames, one wave per page; 2048 frames: a full group of 8 workgroups
    Case("xsmall_udp64", "pb_xsmall_kernel", _udp(64), {}, 0, (1, 5, 64, 65, 2048, 2049)),
    Case("xsmall_udp128", "pb_xsmall_kernel", _udp(128), {}, 0, (1, 2, 32, 33, 2048, 2049)),
    # pages of frames cut at the page edges
    Case("xpage_tcp60", "pb_xpage_kernel", pc.get("c4_tcp_syn"), {}, 0, TCP60),
    Case("xpage_tcp60_fa64", "pb_xpage_kernel", pc.get("c4_tcp_syn"), {"PBGPU_XP_FA64": "1"}, 0, TCP60),
    Case("xpage_tcp60_static", "pb_xpage_kernel", _static("c4_tcp_syn", 6), {}, 0, TCP60),
    Case("xpage_icmp98", "pb_xpage_kernel", pc.get("c5_icmp_echo"), {}, 0, ICMP98),
    # (106-B static UDP takes the page kernel's 2-mod-4 form, not pb_stage_kernel; 2048 frames: 53 pages)
    Case("xpage_udp_static106", "pb_xpage_kernel", pc.get("c1_udp_static_106"), {}, 0,
         (1, 5, 8, 38, 39, 2048, 2049, 2782, 2783)),
    Case("ximg_icmp98", "pb_ximg_kernel", pc.get("c5_icmp_echo"), {"PBGPU_XP_IMG": "2"}, 0, ICMP98),
    # the linear small kernel: 256 frames per workgroup at odd lengths, 64 at even ones
    Case("small_udp43", "pb_small_kernel", _udp(43), {}, 0, (1, 3, 16, 253, 256, 257, 2049)),
    Case("small_udp127", "pb_small_kernel", _udp(127), {}, 0, (1, 3, 16, 253, 256, 257, 2049)),
    Case("small_linear64", "pb_small_kernel", _udp(64), {"PBGPU_KERNEL": "linear"}, 0, (1, 3, 64, 65, 253, 513, 2049)),
    # 64 frames per workgroup; 32 frames end on a 128-B line at each length
    Case("fstage_132", "pb_fstage_kernel", _udp(132), {}, 0, (1, 15, 17, 32, 65, 513)),
    Case("fstage_1500", "pb_fstage_kernel", _udp(1500), {}, 0, (1, 15, 17, 32, 65, 513)),
    Case("fstage_1508", "pb_fstage_kernel", _udp(1508), {}, 0, (1, 15, 17, 32, 65, 513)),
    Case("stage_static242", "pb_stage_kernel", _static("c1_udp_static_106", 200), {}, 0, (1, 3, 8, 17, 65, 513)),
    # a static payload gathered from the device blob: 1500 B is 12 mod 16, four frames end on a chunk
    Case("stage_static1500", "pb_stage_kernel", _static("c2_udp_64", 1458), {}, 0, (1, 3, 4, 17, 65, 513)),
    Case("stage_literal1500", "pb_stage_kernel", _udp(1500), {}, 1, (1, 4, 15, 17, 65, 513)),
    Case("stage_multi_payload", "pb_stage_kernel", pc.get("udp_multi_payload"), {}, 0, (1, 3, 64, 65, 513)),
    Case("vstage_fixed1501", "pb_vstage_kernel", _udp(1501), {}, 0, (1, 7, 16, 33, 129, 513)),
    Case("vstage_0_40", "pb_vstage_kernel", _pl("c3_udp_var", 0, 40), VSTAGE, 0, (1, 3, 253, 2017)),
    Case("vstage_0_40_3pass", "pb_vstage_kernel", _pl("c3_udp_var", 0, 40), dict(VSTAGE, PBGPU_VST_SCAN="3pass"), 0,
         (1, 3, 253, 2017)),
    # 252 frames per workgroup (32 with PBGPU_VL_WGF=32)
    Case("vline_32_33", "pb_vline_kernel", _pl("c3_udp_var", 32, 33), {}, 0, (1, 3, V33_LINES, 253, 2017)),
    Case("vline_64_1500", "pb_vline_kernel", _pl("c3_udp_var", 64, 1500), {}, 0, (1, 3, 253, 2017)),
    Case("vline_32_33_wgf32", "pb_vline_kernel", _pl("c3_udp_var", 32, 33), {"PBGPU_VL_WGF": "32"}, 0,
         (1, 3, V33_LINES, 33, 253, 257)),
    Case("vline_64_1500_wgf32", "pb_vline_kernel", _pl("c3_udp_var", 64, 1500), {"PBGPU_VL_WGF": "32"}, 0, (1, 3, 33, 257)),
    # 4 pages per workgroup; 1740 | 1772 frames of 74..75 B: inside the 32nd page | inside the 33rd
    Case("vpage_32_33", "pb_vpage_kernel", _pl("c3_udp_var", 32, 33), VPAGE, 0,
         (1, 3, V33_PAGE, V33_PAGES, 253, 1740, 1772)),
    Case("vpage_64_1500", "pb_vpage_kernel", _pl("c3_udp_var", 64, 1500), VPAGE, 0, (1, 3, 160, 253)),
    Case("gpf_65042", "pb_gpf_kernel", _udp(65042), {}, 0, (1, 3, 8)),
    # the longest frame there is (PB_MAX_PCKT_LEN), its payload static
    Case("gpf_static65535", "pb_gpf_kernel", _static("c2_udp_64", 65493), {}, 0, (1, 3, 8)),
]
BY_ID = {c.id: c for c in CASES}
# families whose every frame length is a multiple of 16
ALWAYS_16 = {"pb_xsmall_kernel"}


def _seq(case):
    return Sequence.from_config(copy.deepcopy(case.cfg))


def _run(count):
    return count if isinstance(count, tuple) else (FIRST, count)


@functools.lru_cache(maxsize=None)
def _oracle(case_id, first, n_iter, idx=SLOT):
    """The oracle's (bytes, offsets) of a case's build, computed once and kept read-only."""
    case = BY_ID[case_id]
    data, off = ob.build(_seq(case), idx, first, n_iter, pc.SEED_BASE, payload_rule=case.rule)
    data.setflags(write=False)
    off.setflags(write=False)
    return data, off


def _window(case, off):
    """round16(n_frames * max_flen) from the config and the oracle's offsets: a random payload's
    longest length is the config's, any other payload has one length, seen in the oracle's frames."""
    pls = case.cfg.get("payloads") or [{}]
    hl = 54 if case.cfg["ip"]["protocol"] == "tcp" else 42
    lens = np.diff(off.astype(np.int64))
    mx, variable = 0, len(pls) > 1
    for i, p in enumerate(pls):
        ln = p.get("length", {})
        if "exact" not in p and not p.get("isstatic"):
            mx = max(mx, hl + int(ln.get("max", 0)))
            variable = variable or ln.get("min", 0) != ln.get("max", 0)
        else:
            mx = max(mx, int(lens[i::len(pls)].max()))
    return r16(len(lens) * mx), variable


def test_case_table_keeps_its_edges():
    """The table above against the oracle alone: each family has a stream that is not a multiple of
    16 B (where its lengths allow one), a stream that ends exactly on its store unit, and every
    variable-length build leaves part of its window unused."""
    odd, exact = set(), set()
    for case in CASES:
        for count in case.counts:
            first, n = _run(count)
            data, off = _oracle(case.id, first, n)
            total = len(data)
            window, variable = _window(case, off)
            if total % 16:
                odd.add(case.family)
            if total % UNIT[case.family] == 0:
                exact.add(case.family)
            if variable:
                assert total < window, (case.id, count)
            else:
                assert r16(total) == window, (case.id, count)
    families = {c.family for c in CASES}
    assert families == set(UNIT)
    assert odd == families - ALWAYS_16
    assert exact == families
    for first, n, want in ((V33_LINES + (896,)), (V33_PAGE + (4096,)), (V33_PAGES + (8192,))):
        assert len(_oracle("vline_32_33", first, n)[0]) == want


# ------------------------------------------------------------------ 1. guarded windows
@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


class Guarded:
    """A backing buffer B of guard + window + guard bytes, all 0xA5, and W: an alias of its struct
    whose data is the window and whose capacities are exactly (n_frames, window).  B has TAIL more
    offsets entries than W; its offsets hold the ramp 0, 1, 2, ..."""

    def __init__(self, ctx, n_frames, window):
        self.ctx, self.n, self.window = ctx, n_frames, window
        self.cap = GUARD + window + GUARD
        capf = n_frames + TAIL
        self.B = ctx.alloc_frames(capf, self.cap)
        self._keep = []
        # the ramp: an upload of 1-byte frames; it goes through B itself and creates the state that every alias shares
        self.B.upload(np.zeros(capf, dtype=np.uint8), offsets=np.arange(capf + 1, dtype=np.uint64))
        assert self.B.f.reserved
        # a fixed-length upload writes no offsets: the paint goes through an alias with room for cap / 16 frames
        self.view(capacity_frames=self.cap // 16).upload(np.full(self.cap, PAINT, dtype=np.uint8), fixed_len=16)
        assert self.B.f.data % 4096 == 0
        self.W = self.view(data=self.B.f.data + GUARD, capacity_bytes=window, capacity_frames=n_frames)

    def view(self, **fields):
        a = Frames.from_buffer_copy(self.B.f)
        for k, v in fields.items():
            setattr(a, k, v)
        self._keep.append(a)
        return FrameBuffer(self.ctx, C.pointer(a))

    def whole(self):
        return self.B.stream(self.cap)

    def all_offsets(self):
        """B's n_frames + TAIL + 1 offsets (after W's offsets were read: nothing is left to expand)."""
        return self.view(n_frames=self.n + TAIL, fixed_len=0).offsets()

    def free(self):
        self.B.free()


def _first_bad(mask):
    return int(np.nonzero(mask)[0][0])


def _check_window(g, o_data, o_off, what):
    """B whole after a build through g.W; returns what the pad bytes hold."""
    W, total = g.W, len(o_data)
    assert int(W.f.n_frames) == len(o_off) - 1, what
    assert W.total_bytes() == total, what
    assert np.array_equal(W.offsets(), o_off), what
    whole = g.whole()
    front, win = whole[:GUARD], whole[GUARD:]
    assert (front == PAINT).all(), (what, "front guard written at byte %d" % (_first_bad(front != PAINT) - GUARD))
    if not np.array_equal(win[:total], o_data):
        pytest.fail("%s: first mismatch at byte %d" % (what, _first_bad(win[:total] != o_data)))
    end = r16(total)
    pad = win[total:end]
    assert ((pad == 0) | (pad == PAINT)).all(), (what, "pad bytes", pad.tobytes().hex())
    rest = win[end:]
    assert (rest == PAINT).all(), (what, "written %d bytes past round16(total) = %d (window %d)" %
                                   (_first_bad(rest != PAINT), end, g.window))
    # a fixed-length build writes no offsets; a variable-length one offsets[0 .. n_frames]
    keeps = 0 if int(W.f.fixed_len) else g.n + 1
    assert np.array_equal(g.all_offsets()[keeps:], np.arange(keeps, g.n + 1 + TAIL, dtype=np.uint64)), what
    return "none" if not len(pad) else "zeros" if not pad.any() else "untouched" if (pad == PAINT).all() else "mixed"


@gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_build_writes_its_stream_and_nothing_else(ctx, monkeypatch, case):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    seq = _seq(case)
    ctx.load_sequence(SLOT, seq, pc.SEED_BASE, payload_rule=case.rule)
    assert ctx.kernel_name(SLOT).startswith(case.family), ctx.kernel_name(SLOT)
    pads = []
    for count in case.counts:
        first, n_iter = _run(count)
        o_data, o_off = _oracle(case.id, first, n_iter)
        window, variable = _window(case, o_off)
        nf, mb = ctx.build_size(SLOT, n_iter)
        assert (nf, mb) == (len(o_off) - 1, window + 16)  # the least build_check accepts, from the config
        assert window <= 8 << 20
        g = Guarded(ctx, nf, window)
        try:
            p0, b0 = ctx.counters(SLOT + 1)
            ctx.build(SLOT, first, n_iter, g.W)
            ctx.sync()
            assert bool(g.W.f.fixed_len) != variable
            pads.append(_check_window(g, o_data, o_off, "%s n_iter=%d" % (case.id, n_iter)))
            p1, b1 = ctx.counters(SLOT + 1)
            assert (int(p1[SLOT] - p0[SLOT]), int(b1[SLOT] - b0[SLOT])) == (nf, len(o_data))
        finally:
            g.free()
    print("PAD %s (%s): %s" % (case.id, ctx.kernel_name(SLOT).split("<")[0], " ".join(pads)))


MIX = ("c2_udp_64", "c4_tcp_syn", "c5_icmp_echo")
MIX_SIZES = ((7, 70001), (100, 5003), (3, 64))  # (first_iter, n_iter) per part: ragged tails


@gpu
def test_batch_writes_its_streams_and_nothing_else(ctx):
    """pbgpu_build_batch's fused launch (pb_batch_kernel) into three guarded windows."""
    seqs = [Sequence.from_config(pc.get(nm)) for nm in MIX]
    for i, s in enumerate(seqs):
        ctx.load_sequence(i, s, pc.SEED_BASE)
    gs = []
    try:
        for i, (first, n) in enumerate(MIX_SIZES):
            nf, mb = ctx.build_size(i, n)
            gs.append(Guarded(ctx, nf, mb - 16))
        ctx.sync()
        ctx.kernel_time()
        p0, b0 = ctx.counters(3)
        ctx.build_batch([(i, MIX_SIZES[i][0], MIX_SIZES[i][1], gs[i].W) for i in (2, 0, 1)])
        ctx.sync()
        assert ctx.kernel_time()[1] == 1, "one fused launch"
        pads = []
        for i, (first, n) in enumerate(MIX_SIZES):
            o_data, o_off = ob.build(seqs[i], i, first, n, pc.SEED_BASE)
            pads.append(_check_window(gs[i], o_data, o_off, MIX[i]))
        p1, b1 = ctx.counters(3)
        assert [int(x) for x in p1 - p0] == [n for _, n in MIX_SIZES]
        assert [int(x) for x in b1 - b0] == [n * int(g.W.f.fixed_len) for (_, n), g in zip(MIX_SIZES, gs)]
        print("PAD batch (pb_batch_kernel): %s" % " ".join(pads))
    finally:
        for g in gs:
            g.free()


# ------------------------------------------------------------------ 2. one buffer, every kind of use
def _check_state(fb, want_frames, fixed_len, checks=pbgpu.VERIFY_ALL, offsets=True):
    """The buffer's metadata, offsets and frames, a landing of its last 64 frames and a verify."""
    n = len(want_frames)
    total = sum(len(f) for f in want_frames)
    assert (int(fb.f.n_frames), int(fb.f.fixed_len)) == (n, fixed_len)
    assert fb.total_bytes() == total
    if not offsets:
        return
    want_off = np.concatenate([[0], np.cumsum([len(f) for f in want_frames])]).astype(np.uint64)
    assert np.array_equal(fb.offsets(), want_off)
    assert fb.frames() == want_frames
    m = min(64, n)
    if m:
        umem = np.full(m * 4096, 0xEE, dtype=np.uint8)
        lens = fb.to_umem(umem, 4096, n - m, m)
        for j in range(m):
            f, slot = want_frames[n - m + j], umem[j * 4096:(j + 1) * 4096]
            assert int(lens[j]) == len(f) and slot[:len(f)].tobytes() == f and (slot[len(f):] == 0xEE).all(), j
    res = fb.verify(checks=checks)
    assert (int(res.n_checked), int(res.n_bad)) == (n, 0)


@gpu
def test_one_buffer_through_every_kind_of_use(ctx, monkeypatch):
    var = Sequence.from_config(pc.get("c3_udp_var"))
    fix = Sequence.from_config(pc.get("c2_udp_64"))
    for slot, seq, env, kern in ((0, var, {}, "pb_vline_kernel"), (1, fix, {}, "pb_xsmall_kernel"),
                                 (2, var, VSTAGE, "pb_vstage_kernel"), (3, var, {"PBGPU_VL_WGF": "100"}, "pb_vline_kernel"),
                                 (4, var, VPAGE, "pb_vpage_kernel")):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            ctx.load_sequence(slot, seq, pc.SEED_BASE)
        assert ctx.kernel_name(slot).startswith(kern)
    fb = ctx.alloc_frames(8192, 16 << 20)
    src = ctx.alloc_frames(*ctx.build_size(0, 2500))
    try:
        # 1. packed build (4-B offsets pending), the offsets never read
        ctx.build(0, 11, 5000, fb)
        _check_state(fb, ob.frames(var, 0, 11, 5000, pc.SEED_BASE), 0, offsets=False)
        # 2. fixed 64-B build, fewer frames
        ctx.build(1, 22, 3000, fb)
        _check_state(fb, ob.frames(fix, 1, 22, 3000, pc.SEED_BASE), 64)
        # 3. 64-bit offsets written by the build
        ctx.build(2, 33, 4500, fb)
        _check_state(fb, ob.frames(var, 2, 33, 4500, pc.SEED_BASE), 0)
        # 4. variable-length upload
        up = ob.frames(Sequence.from_config(pc.get("tcp_all_flags_var")), 7, 44, 3500, pc.SEED_BASE)
        fb.upload(b"".join(up), offsets=np.concatenate([[0], np.cumsum([len(f) for f in up])]))
        _check_state(fb, up, 0)
        # 5. packed build again, another shape from another slot
        ctx.build(3, 55, 6000, fb)
        _check_state(fb, ob.frames(var, 3, 55, 6000, pc.SEED_BASE), 0)
        # 6. an encapsulation into it
        ctx.build(0, 66, 2500, src)
        src.encap(fb, mode=ENCAP_VXLAN, **VX)
        enc = [pyencap.vxlan(f, **VX) for f in ob.frames(var, 0, 66, 2500, pc.SEED_BASE)]
        _check_state(fb, enc, 0, checks=pbgpu.VERIFY_IP_CSUM | pbgpu.VERIFY_TOT_LEN)  # (the outer UDP checksum is 0)
        # 7. the page writer
        ctx.build(4, 77, 4000, fb)
        _check_state(fb, ob.frames(var, 4, 77, 4000, pc.SEED_BASE), 0)
        # 8. an empty build
        ctx.build(0, 88, 0, fb)
        _check_state(fb, [], 0)
        ctx.build(1, 99, 0, fb)
        _check_state(fb, [], 64)
    finally:
        src.free()
        fb.free()


# ------------------------------------------------------------------ 3. iteration-number edges
# one case per family and the iterations of each build
EDGE = [("xsmall_udp64", 3000), ("xpage_tcp60", 3000), ("ximg_icmp98", 3000), ("small_udp43", 3000),
        ("fstage_1500", 600), ("stage_literal1500", 600), ("stage_multi_payload", 750), ("vstage_0_40", 3000),
        ("vline_64_1500", 1500), ("vpage_64_1500", 1500), ("gpf_65042", 200)]


def _edge_firsts(case_id, n):
    straddle = (1 << 33) if case_id == "stage_multi_payload" else (1 << 32)
    return (straddle - n // 2, SEED_K - 1 - n)


@gpu
@pytest.mark.parametrize("case_id,n", EDGE, ids=[e[0] for e in EDGE])
def test_iteration_numbers_at_the_edges(ctx, monkeypatch, case_id, n):
    case = BY_ID[case_id]
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    seq = _seq(case)
    ctx.load_sequence(SLOT, seq, pc.SEED_BASE, payload_rule=case.rule)
    assert ctx.kernel_name(SLOT).startswith(case.family), ctx.kernel_name(SLOT)
    fb = ctx.alloc_frames(*ctx.build_size(SLOT, n))
    try:
        for first in _edge_firsts(case_id, n):
            assert first < first + n < SEED_K
            ctx.build(SLOT, first, n, fb)
            ctx.sync()
            o_data, o_off = ob.build(seq, SLOT, first, n, pc.SEED_BASE, payload_rule=case.rule)
            assert np.array_equal(fb.offsets(), o_off), first
            g_data = fb.packed()
            if not np.array_equal(g_data, o_data):
                pytest.fail("first_iter %d: first mismatch at byte %d" % (first, _first_bad(g_data != o_data)))
        # one past the top: refused, the buffer's metadata and the counters as they were
        meta = bytes(fb.f)
        p0, b0 = ctx.counters(SLOT + 1)
        for first, k in ((SEED_K - n, n), (SEED_K - 1, 1), (SEED_K, 0)):
            assert ctx.lib.pbgpu_build(ctx.h, SLOT, first, k, fb.ptr) == EINVAL
        assert bytes(fb.f) == meta
        p1, b1 = ctx.counters(SLOT + 1)
        assert np.array_equal(p0, p1) and np.array_equal(b0, b1)
        assert np.array_equal(fb.packed(), g_data)
    finally:
        fb.free()


@gpu
def test_batch_iteration_numbers_at_the_edges(ctx):
    seqs = [Sequence.from_config(pc.get(nm)) for nm in MIX]
    for i, s in enumerate(seqs):
        ctx.load_sequence(i, s, pc.SEED_BASE)
    sizes = (4099, 3001, 2049)
    bufs = [ctx.alloc_frames(*ctx.build_size(i, n)) for i, n in enumerate(sizes)]
    try:
        for firsts in ([(1 << 32) - n // 2 for n in sizes], [SEED_K - 1 - n for n in sizes]):
            ctx.sync()
            ctx.kernel_time()
            ctx.build_batch([(i, firsts[i], sizes[i], bufs[i]) for i in range(3)])
            ctx.sync()
            assert ctx.kernel_time()[1] == 1, "one fused launch"
            for i in range(3):
                o_data, o_off = ob.build(seqs[i], i, firsts[i], sizes[i], pc.SEED_BASE)
                assert np.array_equal(bufs[i].packed(), o_data), (i, firsts[i])
        p0, b0 = ctx.counters(3)
        with pytest.raises(pbgpu.PbError) as e:
            ctx.build_batch([(0, 5, sizes[0], bufs[0]), (1, SEED_K - sizes[1], sizes[1], bufs[1]), (2, 5, sizes[2], bufs[2])])
        assert e.value.code == EINVAL
        p1, b1 = ctx.counters(3)
        assert np.array_equal(p0, p1) and np.array_equal(b0, b1)
        assert [int(fb.f.first_iter) for fb in bufs] == [SEED_K - 1 - n for n in sizes]
    finally:
        for fb in bufs:
            fb.free()
