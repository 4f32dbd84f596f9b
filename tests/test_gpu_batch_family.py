"""pbgpu_build_batch's fused launch (pb_batch_kernel) on every sequence shape it admits
(tests/batch_cases.py): each ICMP length of 66 ... 126 B with the stream image and without it
(the non-image branch of pb_batch_part), TCP parts of 56, 60 and 64 B, both block sizes, frame
counts that end inside the first page, fill exactly one group of 8 workgroups, start the first
tail workgroup and leave a ragged tail, with and without padding workgroups between the parts.
Every output is compared bit-exact with the CPU oracle, part by part; TIMING_LAUNCH's launch count
tells a fused call (1) from one launch per part.

a. the family sweep, with pbgpu_verify as a second judge and the counters;
b. header fields inside the batch: all random, none random, checksums off, the alternative rules,
   the static payload's other forms;
c. guard bands around each part's window;
d. state between calls: a reloaded ICMP slot's image, single builds around a batch on other
   streams, the 64-bit first-frame path, a count ring that folds between batches;
e. near misses: sets the rule does not admit build one launch per part, with the same bytes."""
import contextlib
import functools
import os

import numpy as np
import pytest

import batch_cases as bc
import oracle_binding as ob
import pb_configs as pc
import pbgpu
from pbgpu import GpuContext, Sequence
from test_gpu_build_bounds import GUARD, Guarded, _check_window

pytestmark = pytest.mark.gpu

# the load-time and open-time environment this file sets; cleared around every load and open
ENV = ("PBGPU_XP_FORCE", "PBGPU_XP_STATIC", "PBGPU_XP_IMG", "PBGPU_XP_FA64", "PBGPU_XP_WGT", "PBGPU_XP_NP",
       "PBGPU_KERNEL", "PBGPU_BATCH", "PBGPU_BATCH_WGT", "PBGPU_CTR_RING", "PBGPU_CTR_ATOMIC")


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.pop(k, None) for k in ENV}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in ENV:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


@pytest.fixture(scope="module")
def ctxs():
    """One context per block size (PBGPU_BATCH_WGT is read when a context is opened)."""
    made = {}

    def get(wgt):
        if wgt not in made:
            with _env({"PBGPU_BATCH_WGT": str(wgt)}):
                made[wgt] = GpuContext(0)
        return made[wgt]

    yield get
    for c in made.values():
        c.close()


def _load(ctx, slot, cfg, env, rule=pbgpu.PAYLOAD_STREAM, fold=pbgpu.FOLD_FULL):
    seq = Sequence.from_config(cfg)
    with _env(env):
        ctx.load_sequence(slot, seq, pc.SEED_BASE, payload_rule=rule, iph_fold=fold)
    return seq


def _load_parts(ctx, parts):
    return [_load(ctx, k, cfg, env) for k, (cfg, env) in enumerate(parts)]


def _same(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = int(np.nonzero(got != want)[0][0])
        pytest.fail("%s: first mismatch at byte %d of %d" % (what, bad, len(want)))


def _check(seq, slot, first, n, fb, what, rule=0, fold=0):
    o_data, o_off = ob.build(seq, slot, first, n, pc.SEED_BASE, payload_rule=rule, iph_fold=fold)
    assert int(fb.f.n_frames) == len(o_off) - 1, what
    assert np.array_equal(fb.offsets(), o_off), what
    _same(fb.packed(), o_data, "%s slot %d first %d n %d" % (what, slot, first, n))
    return len(o_off) - 1, len(o_data)


def _bufs(ctx, batches):
    return [ctx.alloc_frames(*ctx.build_size(k, max(b.sizes[k][1] for b in batches))) for k in range(3)]


def _launches(ctx):
    ctx.sync()
    return ctx.kernel_time()[1]


def _image_named(ctx, slot=2):
    return "pb_ximg_body" in ctx.kernel_name(slot)


# ------------------------------------------------------------------ a. the family sweep
@pytest.mark.parametrize("case", bc.CASES, ids=[c.id for c in bc.CASES])
def test_family_matches_oracle(ctxs, case):
    ctx = ctxs(case.wgt)
    seqs = _load_parts(ctx, case.parts)
    assert _image_named(ctx) == case.img, ctx.kernel_name(2)
    ctx.set_timing(ctx.TIMING_LAUNCH)
    batches = bc.batches(case)
    bufs = _bufs(ctx, batches)
    try:
        _launches(ctx)
        p0, b0 = ctx.counters(3)
        frames, nbytes = [0, 0, 0], [0, 0, 0]
        for r, b in enumerate(batches):
            ctx.build_batch([(k, b.sizes[k][0], b.sizes[k][1], bufs[k]) for k in b.order])
            # (no sync: the verify launches follow the batch through the buffers' own ordering)
            res = [bufs[k].verify(checks=pbgpu.VERIFY_ALL) for k in range(3)]
            assert _launches(ctx) == 1, "%s batch %d: one fused launch" % (case.id, r)
            for k, (first, n) in enumerate(b.sizes):
                assert (int(res[k].n_checked), int(res[k].n_bad)) == (n, 0), (case.id, r, k)
                nf, nb = _check(seqs[k], k, first, n, bufs[k], "%s batch %d" % (case.id, r))
                frames[k] += nf
                nbytes[k] += nb
        p1, b1 = ctx.counters(3)
        assert [int(x) for x in p1 - p0] == frames
        assert [int(x) for x in b1 - b0] == nbytes
    finally:
        for fb in bufs:
            fb.free()


# ------------------------------------------------------------------ b. fields inside the batch
RANGES = ["10.20.0.0/16", "172.16.0.1/32", "0.0.0.0/0"]


def _all_random(cfg):
    cfg["ip"].update(ttl={"min": 3, "max": 250}, id={"min": 7, "max": 65000}, ranges=list(RANGES), tos=0x2E)
    for proto in ("udp", "tcp"):
        if proto in cfg:
            cfg[proto].update(sport=0, dport=0)
    return cfg


def _none_random(cfg):
    cfg["ip"].pop("ranges", None)
    cfg["ip"].update(sip="10.0.0.1", ttl={"min": 77, "max": 77}, id={"min": 4242, "max": 4242})
    for proto in ("udp", "tcp"):
        if proto in cfg:
            cfg[proto].update(sport=1234, dport=80)
    return cfg


def _no_csums(cfg):
    cfg["l4csum"] = 0
    cfg["ip"]["csum"] = 0
    return cfg


def _as_string(cfg):
    n = bc.frame_length(cfg) - 42
    cfg["payloads"] = [{"exact": "".join(chr(33 + (5 * i) % 94) for i in range(n)), "isstring": 1}]
    return cfg


def _as_static_random(cfg):
    n = bc.frame_length(cfg) - 42
    cfg["payloads"] = [{"isstatic": 1, "length": {"min": n, "max": n}}]
    return cfg


def _keep(cfg):
    return cfg


# name: (change of the UDP and TCP configs, change of the ICMP config, rules of the two random parts, IPv4 fold of all)
FIELDS = {
    "all_random": (_all_random, _all_random, 0, 0),
    "none_random": (_none_random, _none_random, 0, 0),
    "no_csums": (_no_csums, _no_csums, 0, 0),
    # (the folds differ only in a frame whose header sum carries twice, about one in 30,000 with every
    # field random: the test adds a batch around such a frame of each part, _fold_edge)
    "rules": (_all_random, _all_random, pbgpu.PAYLOAD_LITERAL, pbgpu.FOLD_SINGLE),
    "icmp_string": (_keep, _as_string, 0, 0),
    "icmp_static_random": (_keep, _as_static_random, 0, 0),
}


@functools.lru_cache(maxsize=None)
def _fold_edge(tcp_len, icmp_len, k):
    """The first iteration from 1 on at which part k's frame, every field random, differs between
    the single and the full fold of the IPv4 checksum (the oracle's; the first 2^20 searched)."""
    cfg = _all_random(bc.make_case(0, 512, True, tcp_len, icmp_len).parts[k][0])
    seq, flen, step = Sequence.from_config(cfg), bc.frame_length(cfg), 1 << 16
    for first in range(1, 1 << 20, step):
        full, _ = ob.build(seq, k, first, step, pc.SEED_BASE, payload_rule=pbgpu.PAYLOAD_LITERAL, iph_fold=pbgpu.FOLD_FULL)
        single, _ = ob.build(seq, k, first, step, pc.SEED_BASE, payload_rule=pbgpu.PAYLOAD_LITERAL,
                             iph_fold=pbgpu.FOLD_SINGLE)
        bad = np.nonzero(full != single)[0]
        if len(bad):
            return first + int(bad[0]) // flen
    raise AssertionError("no frame whose header sum carries twice")


def _fold_edge_batch(case):
    """A batch whose every part holds its _fold_edge frame about 100 frames in (count class c)."""
    sizes = []
    for k in range(3):
        first = max(1, _fold_edge(case.tcp_len, case.icmp_len, k) - 100) | 1
        sizes.append((first, bc.counts(case.lens[k], case.ppw[k])[2]))
    return bc.Batch((1, 0, 2), tuple(sizes))


@pytest.mark.parametrize("wgt", bc.WGTS)
@pytest.mark.parametrize("lens", [(60, 98), (56, 66)], ids=["64_60_98", "64_56_66"])
@pytest.mark.parametrize("fields", list(FIELDS))
def test_fields_inside_the_batch(ctxs, fields, lens, wgt):
    ctx = ctxs(wgt)
    rnd, icmp, rule, fold = FIELDS[fields]
    case = bc.make_case(list(FIELDS).index(fields), wgt, True, *lens)
    cfgs = [rnd(case.parts[0][0]), rnd(case.parts[1][0]), icmp(case.parts[2][0])]
    assert [bc.batch_kind(c, e) for c, (_, e) in zip(cfgs, case.parts)] == [1, 2, 3]
    rules = [rule, rule, 0]
    seqs = [_load(ctx, k, cfgs[k], case.parts[k][1], rule=rules[k], fold=fold) for k in range(3)]
    assert _image_named(ctx)
    ctx.set_timing(ctx.TIMING_LAUNCH)
    batches = bc.batches(case)  # all four: every part meets its largest count
    if fields == "rules":
        edge = _fold_edge_batch(case)
        for k, (first, n) in enumerate(edge.sizes):  # the two folds give other bytes in every part
            one, _ = ob.build(seqs[k], k, first, n, pc.SEED_BASE, payload_rule=rules[k], iph_fold=pbgpu.FOLD_SINGLE)
            full, _ = ob.build(seqs[k], k, first, n, pc.SEED_BASE, payload_rule=rules[k], iph_fold=pbgpu.FOLD_FULL)
            assert not np.array_equal(one, full), k
        batches.append(edge)
    bufs = _bufs(ctx, batches)
    try:
        for b in batches:
            _launches(ctx)
            ctx.build_batch([(k, b.sizes[k][0], b.sizes[k][1], bufs[k]) for k in b.order])
            assert _launches(ctx) == 1, "one fused launch"
            for k, (first, n) in enumerate(b.sizes):
                _check(seqs[k], k, first, n, bufs[k], fields, rule=rules[k], fold=fold)
    finally:
        for fb in bufs:
            fb.free()


# ------------------------------------------------------------------ c. guard bands
GUARD_CASES = [bc.make_case(i, wgt, img, tcp, icmp) for i, (wgt, img, tcp, icmp) in enumerate(
    (w, i, t, c) for w in bc.WGTS for i in (True, False) for t in (56, 64) for c in (66, 126))]


@pytest.mark.parametrize("case", GUARD_CASES, ids=[c.id for c in GUARD_CASES])
def test_family_writes_its_streams_and_nothing_else(ctxs, case):
    """No byte before a part's window, none at or past round16(total), pad bytes zero or untouched,
    offsets not written (test_gpu_build_bounds's checks, per part of the fused launch)."""
    ctx = ctxs(case.wgt)
    seqs = _load_parts(ctx, case.parts)
    assert _image_named(ctx) == case.img
    ctx.set_timing(ctx.TIMING_LAUNCH)
    b = bc.batches(case)[case.index % 4]
    gs = []
    try:
        for k, (first, n) in enumerate(b.sizes):
            nf, mb = ctx.build_size(k, n)
            gs.append(Guarded(ctx, nf, mb - 16))
        _launches(ctx)
        ctx.build_batch([(k, b.sizes[k][0], b.sizes[k][1], gs[k].W) for k in b.order])
        assert _launches(ctx) == 1, "one fused launch"
        for k, (first, n) in enumerate(b.sizes):
            o_data, o_off = ob.build(seqs[k], k, first, n, pc.SEED_BASE)
            _check_window(gs[k], o_data, o_off, "%s part %d n %d" % (case.id, k, n))
    finally:
        for g in gs:
            g.free()


# ------------------------------------------------------------------ d. state between calls
def _one_batch(ctx, seqs, sizes, bufs, what, order=(2, 0, 1), launches=1):
    _launches(ctx)
    ctx.build_batch([(k, sizes[k][0], sizes[k][1], bufs[k]) for k in order])
    assert _launches(ctx) == launches, what
    for k, (first, n) in enumerate(sizes):
        _check(seqs[k], k, first, n, bufs[k], what)


@pytest.mark.parametrize("wgt", bc.WGTS)
def test_reloaded_icmp_slot_uses_its_own_image(ctxs, wgt):
    """The ICMP slot reloaded with another length, then without the image: each batch builds the
    sequence loaded last, never an earlier load's image."""
    ctx = ctxs(wgt)
    ctx.set_timing(ctx.TIMING_LAUNCH)
    case = bc.make_case(0, wgt, True, 60, 98)
    seqs = _load_parts(ctx, case.parts)
    sizes = [(11, 2049), (13, 5003), (15, 3 * 49 * 4096 // 98 + 77)]  # the ICMP part: past three image periods
    bufs = [ctx.alloc_frames(*ctx.build_size(k, n)) for k, (_, n) in enumerate(sizes)]
    bufs[2].free()
    bufs[2] = ctx.alloc_frames(sizes[2][1], sizes[2][1] * 126 + 16)
    try:
        for flen, env in ((98, {}), (70, {}), (126, {}), (126, {"PBGPU_XP_IMG": "0"}), (98, {}),
                          (98, {"PBGPU_KERNEL": "vstage"}), (70, {"PBGPU_KERNEL": "auto"})):
            cfg = bc.icmp_cfg(flen)
            seqs[2] = _load(ctx, 2, cfg, env)
            assert bc.batch_kind(cfg, env) == 3
            assert _image_named(ctx) == bc.has_image(cfg, env) == (not env or env == {"PBGPU_KERNEL": "auto"})
            _one_batch(ctx, seqs, sizes, bufs, "icmp %d %s" % (flen, env))
    finally:
        for fb in bufs:
            fb.free()


@pytest.mark.parametrize("img", [True, False], ids=["img", "noimg"])
def test_single_builds_around_a_batch_in_span_mode(ctxs, img):
    """Span timing: a single build runs on its sequence's own stream, the batch on the context's.
    A build of the TCP sequence into its buffer, the batch into the same three buffers, and a
    build again, first with the bytes read after every step, then with nothing waited for in
    between.  (This runs the hop between the streams; it does not prove the ordering: a missing
    wait would only show when the device happens to overlap the launches.)"""
    ctx = ctxs(512)
    case = bc.make_case(1, 512, img, 56, 74)
    seqs = _load_parts(ctx, case.parts)
    ctx.set_timing(ctx.TIMING_SPAN)
    sizes = [b.sizes for b in bc.batches(case)]
    bufs = _bufs(ctx, bc.batches(case))
    try:
        f1, n1 = sizes[3][1]
        ctx.build(1, f1, n1, bufs[1])
        _check(seqs[1], 1, f1, n1, bufs[1], "single build before")
        ctx.build_batch([(k, sizes[1][k][0], sizes[1][k][1], bufs[k]) for k in range(3)])
        for k in range(3):
            _check(seqs[k], k, sizes[1][k][0], sizes[1][k][1], bufs[k], "batch")
        ctx.build(1, f1 + 2, n1, bufs[1])
        _check(seqs[1], 1, f1 + 2, n1, bufs[1], "single build after")
        # the same three steps back to back
        ctx.build(1, f1, n1, bufs[1])
        ctx.build_batch([(k, sizes[0][k][0], sizes[0][k][1], bufs[k]) for k in range(3)])
        ctx.build(1, f1 + 4, n1, bufs[1])
        for k in (0, 2):
            _check(seqs[k], k, sizes[0][k][0], sizes[0][k][1], bufs[k], "batch, not waited for")
        _check(seqs[1], 1, f1 + 4, n1, bufs[1], "single build after, not waited for")
        ctx.sync()
        assert ctx.kernel_time()[1] == 6
    finally:
        ctx.set_timing(ctx.TIMING_LAUNCH)
        for fb in bufs:
            fb.free()


@pytest.mark.parametrize("wgt", bc.WGTS)
@pytest.mark.parametrize("img", [True, False], ids=["img", "noimg"])
def test_64bit_first_frame_inside_the_batch(ctxs, img, wgt):
    """PBGPU_XP_FA64=1 at load: both page bodies find their pages' first frames by the 64-bit path."""
    ctx = ctxs(wgt)
    ctx.set_timing(ctx.TIMING_LAUNCH)
    case = bc.make_case(2, wgt, img, 56, 98)
    seqs = [_load(ctx, k, cfg, dict(env, PBGPU_XP_FA64="1")) for k, (cfg, env) in enumerate(case.parts)]
    assert _image_named(ctx) == img
    batches = bc.batches(case)
    bufs = _bufs(ctx, batches)
    try:
        for b in batches[1:3]:
            _one_batch(ctx, seqs, b.sizes, bufs, "fa64", order=b.order)
    finally:
        for fb in bufs:
            fb.free()


RING = 40


def _ring_folds(words, ring):
    """How often a fresh slot's count ring is folded by a run of launches of `words` records each: a
    launch whose records do not fit behind the pending ones folds the ring first; the ring's
    capacity is `ring` words, or the largest launch so far if that is more."""
    cap = used = folds = 0
    for w in words:
        if used + w > cap:
            folds += used > 0
            used = 0
            cap = max(cap, w, ring)
        used += w
    return folds


@pytest.mark.parametrize("wgt", bc.WGTS)
def test_count_ring_folds_between_batches(wgt):
    """PBGPU_CTR_RING=40 in a context of its own, so each slot's first ring is the 40-word one (a
    slot keeps its ring across reloads, and a context that has built already holds the default
    8 Mi words).  A part writes one record per workgroup: 1, 8, 9 and 25 or 26 per launch in the four
    count classes, none more than 40, so the ring never grows; eight batches write 86 to 88 records
    per part and a launch that finds less room than it needs folds the ring first, at least twice
    per part (_ring_folds, asserted below).  The counters are read once, at the end, and are
    exact."""
    case = bc.make_case(3, wgt, False, 60, 82)
    batches = bc.batches(case) * 2
    for k in range(3):
        words = [bc.part_grid(case.lens[k], b.sizes[k][1], case.ppw[k], False)[3] for b in batches]
        assert max(words) <= RING and 86 <= sum(words) <= 88 and _ring_folds(words, RING) >= 2, (k, words)
    with _env({"PBGPU_BATCH_WGT": str(wgt)}):
        ctx = GpuContext(0)
    bufs = []
    try:
        ctx.set_timing(ctx.TIMING_LAUNCH)
        seqs = [_load(ctx, k, cfg, dict(env, PBGPU_CTR_RING=str(RING))) for k, (cfg, env) in enumerate(case.parts)]
        bufs = _bufs(ctx, batches)
        frames = [0, 0, 0]
        for rep, b in enumerate(batches):
            ctx.build_batch([(k, b.sizes[k][0] + 2 * rep, b.sizes[k][1], bufs[k]) for k in b.order])
            for k in range(3):
                frames[k] += b.sizes[k][1]
        assert _launches(ctx) == 8
        for k, (first, n) in enumerate(batches[-1].sizes):
            _check(seqs[k], k, first + 14, n, bufs[k], "after the folds")
        p1, b1 = ctx.counters(3)
        assert [int(x) for x in p1] == frames
        assert [int(x) for x in b1] == [f * ln for f, ln in zip(frames, case.lens)]
    finally:
        for fb in bufs:
            fb.free()
        ctx.close()


# ------------------------------------------------------------------ e. near misses
N_MISS = (4099, 3001, 2049)
# launches of a three-part call that does not fuse: one per part that has frames
MISS_LAUNCHES = 3


@pytest.mark.parametrize("miss", bc.NEAR_MISSES, ids=[m[0] for m in bc.NEAR_MISSES])
def test_near_miss_sequences_fall_back(ctxs, miss):
    name, slot, cfg, env = miss
    ctx = ctxs(512)
    ctx.set_timing(ctx.TIMING_LAUNCH)
    parts = list(bc.make_case(0, 512, True, 60, 98).parts)
    parts[slot] = (cfg, env)
    seqs = _load_parts(ctx, parts)
    sizes = [(5 + 2 * k, n) for k, n in enumerate(N_MISS)]
    bufs = [ctx.alloc_frames(*ctx.build_size(k, n)) for k, n in enumerate(N_MISS)]
    try:
        _one_batch(ctx, seqs, sizes, bufs, name, launches=MISS_LAUNCHES)
    finally:
        for fb in bufs:
            fb.free()


def test_near_miss_calls_fall_back(ctxs):
    """Valid sequences in calls the rule does not admit: a buffer whose data is not 4-KiB aligned,
    two parts of one kind, a part with no iterations."""
    ctx = ctxs(512)
    ctx.set_timing(ctx.TIMING_LAUNCH)
    case = bc.make_case(0, 512, True, 60, 98)
    seqs = _load_parts(ctx, case.parts)
    seqs.append(_load(ctx, 3, bc.tcp_cfg(56), {}))
    sizes = [(5 + 2 * k, n) for k, n in enumerate(N_MISS)] + [(21, N_MISS[1])]
    bufs = [ctx.alloc_frames(*ctx.build_size(k, n)) for k, (_, n) in enumerate(sizes)]
    g = None
    try:
        # the fused form first, so the fall-backs below are told apart from it
        _one_batch(ctx, seqs, sizes[:3], bufs, "fused")
        # the ICMP part's data at 4 KiB + 2048: an alias of a larger buffer's struct, as Guarded.view makes
        nf, mb = ctx.build_size(2, N_MISS[2])
        g = Guarded(ctx, nf, mb - 16 + 4096)
        half = g.view(data=g.B.f.data + GUARD + 2048, capacity_bytes=mb - 16, capacity_frames=nf)
        assert int(half.f.data) % 4096 == 2048
        _one_batch(ctx, seqs, sizes[:3], bufs[:2] + [half], "half-page aligned data", launches=MISS_LAUNCHES)
        # two TCP parts (slots 1 and 3) next to the ICMP one
        _launches(ctx)
        ctx.build_batch([(k, sizes[k][0], sizes[k][1], bufs[k]) for k in (1, 3, 2)])
        assert _launches(ctx) == MISS_LAUNCHES
        for k in (1, 3, 2):
            _check(seqs[k], k, sizes[k][0], sizes[k][1], bufs[k], "two parts of kind 2")
        # a part with no iterations: the other two are launched, that part reports no frames
        for empty in range(3):
            zs = [(f, 0 if k == empty else n) for k, (f, n) in enumerate(sizes[:3])]
            _launches(ctx)
            ctx.build_batch([(k, zs[k][0], zs[k][1], bufs[k]) for k in (2, 0, 1)])
            assert _launches(ctx) == 2, empty
            assert int(bufs[empty].f.n_frames) == 0 and bufs[empty].total_bytes() == 0
            for k in range(3):
                if k != empty:
                    _check(seqs[k], k, zs[k][0], zs[k][1], bufs[k], "part %d empty" % empty)
    finally:
        if g:
            g.free()
        for fb in bufs:
            fb.free()
