"""tests/batch_cases.py against itself and the oracle (no GPU): the admission rule over the case
table, the near misses and every length; the page arithmetic's pinned values; that the count
classes reach the pages, full groups, tail workgroups and padding they are named for; and that
the oracle builds every case's frames at the stated length."""
import numpy as np

import batch_cases as bc
import oracle_binding as ob
import pb_configs as pc
from pbgpu import Sequence


def test_kinds_of_the_table():
    assert len(bc.CASES) == 64 and len({c.id for c in bc.CASES}) == 64
    for case in bc.CASES:
        assert [bc.batch_kind(cfg, env) for cfg, env in case.parts] == [1, 2, 3], case.id
        assert bc.has_image(*case.parts[2]) == case.img, case.id
        assert [bc.frame_length(cfg) for cfg, _ in case.parts] == list(case.lens), case.id
    # each TCP length meets each block size and both image settings
    assert {(c.tcp_len, c.wgt, c.img) for c in bc.CASES} == {(t, w, i) for t in bc.TCP_LENS for w in bc.WGTS
                                                            for i in (True, False)}
    assert {(c.icmp_len, c.wgt, c.img) for c in bc.CASES} == {(t, w, i) for t in bc.ICMP_LENS for w in bc.WGTS
                                                             for i in (True, False)}


def test_near_misses_have_no_kind():
    assert len(bc.NEAR_MISSES) == 9
    for name, slot, cfg, env in bc.NEAR_MISSES:
        assert bc.batch_kind(cfg, env) == 0, name
    for cfg, env in bc.CASES[0].parts:
        assert bc.batch_kind(cfg, dict(env, PBGPU_BATCH="0")) == 0
        assert bc.batch_kind(cfg, dict(env, PBGPU_KERNEL="linear")) == 0
    udp, tcp, icmp = bc.CASES[0].parts
    nopage = {"PBGPU_KERNEL": "nopage"}
    assert [bc.batch_kind(udp[0], nopage), bc.batch_kind(tcp[0], nopage), bc.batch_kind(icmp[0], nopage)] == [1, 0, 0]
    assert bc.batch_kind(icmp[0], {"PBGPU_XP_STATIC": "0", "PBGPU_XP_FORCE": "1"}) == 3
    assert not bc.has_image(icmp[0], {"PBGPU_XP_FORCE": "1"})
    # a PBGPU_KERNEL value the library knows drops the image and keeps the kind; any other is the default
    for k in ("gpf", "stage", "vstage", "vpage"):
        assert bc.batch_kind(icmp[0], {"PBGPU_KERNEL": k}) == 3 and not bc.has_image(icmp[0], {"PBGPU_KERNEL": k})
    assert bc.has_image(icmp[0], {"PBGPU_KERNEL": "auto"}) and bc.has_image(icmp[0], {})


def _payloads(nbytes):
    yield {"length": {"min": nbytes, "max": nbytes}}
    yield {"exact": " ".join("%02x" % (i & 255) for i in range(nbytes))}
    yield {"exact": "x" * nbytes, "isstring": 1}
    yield {"isstatic": 1, "length": {"min": nbytes, "max": nbytes}}


def test_table_covers_what_the_rule_admits():
    admitted = set()
    envs = ({}, {"PBGPU_XP_FORCE": "1"}, {"PBGPU_XP_IMG": "0"}, {"PBGPU_XP_STATIC": "0"}, {"PBGPU_KERNEL": "nopage"})
    for proto, base in (("udp", "c2_udp_64"), ("tcp", "c4_tcp_syn"), ("icmp", "c5_icmp_echo")):
        for flen in range(42, 129):
            if flen < bc.HL[proto]:
                continue
            for pl in _payloads(flen - bc.HL[proto]):
                cfg = pc.get(base)
                cfg["payloads"] = [pl]
                for env in envs:
                    kind = bc.batch_kind(cfg, env)
                    if kind:
                        admitted.add((kind, flen, bc.has_image(cfg, env)))
    table = set()
    for case in bc.CASES:
        for k, (cfg, env) in enumerate(case.parts):
            table.add((k + 1, case.lens[k], bc.has_image(cfg, env)))
    assert table == admitted
    assert admitted == ({(1, 64, False)} | {(2, n, False) for n in (56, 60, 64)} |
                        {(3, n, i) for n in range(66, 127, 4) for i in (True, False)})


def test_page_params_pinned():
    for flen, slots, ppw in ((56, 75, 6), (60, 70, 7), (64, 65, 7)):
        assert bc.page_params(flen, 512, False)[:2] == (slots, ppw) == bc.page_params(flen, 256, False)[:2]
    for flen, slots, ppw in ((66, 64, 8), (70, 60, 8), (74, 57, 8), (78, 54, 9), (98, 43, 9), (126, 34, 9)):
        assert bc.page_params(flen, 512, False)[:2] == (slots, ppw) == bc.page_params(flen, 256, False)[:2]
        assert bc.page_params(flen, 512, True)[:2] == (slots, 8)
        assert bc.page_params(flen, 256, True)[:2] == (slots, 4)
    assert bc.page_params(64, 512, False, whole=True) == (64, 8, 1)
    assert bc.page_params(64, 256, False, whole=True) == (64, 4, 1)
    assert bc.page_params(98, 512, True)[2] == 49
    periods = [bc.page_params(n, 512, True)[2] for n in bc.ICMP_LENS]
    assert (min(periods), max(periods)) == (33, 63) and all(p % 2 for p in periods)
    # 66 B: the edge of the image body's one pass of slots, and of the slot limit without the image
    assert bc.page_params(66, 512, True)[0] == 64 and 64 * bc.page_params(66, 512, False)[1] == 512
    for flen in bc.ICMP_LENS + bc.TCP_LENS:
        slots, ppw, _ = bc.page_params(flen, 256, False)
        assert slots * ppw <= 512


def test_count_classes_do_what_they_claim():
    seen = set()           # (part, class) over the table
    padded = {0: set(), 1: set()}
    for case in bc.CASES:
        img = (False, False, case.img)
        per_part = [set() for _ in range(3)]
        bs = bc.batches(case)
        assert len(bs) == 4
        firsts = set()
        for r, b in enumerate(bs):
            assert sorted(b.order) == [0, 1, 2]
            classes = set()
            for k, (first, n) in enumerate(b.sizes):
                flen, ppw = case.lens[k], case.ppw[k]
                assert first % 2 == 1 and n * flen < bc.MAX_PART_BYTES
                firsts.add(first)
                cls = bc.counts(flen, ppw, n if n in (1, 5) else 1).index(n)
                classes.add(cls)
                per_part[k].add(cls)
                seen.add((k, cls, n if cls == 0 else 0))
                nch, full, tail, grid = bc.part_grid(flen, n, ppw, img[k])
                last = n * flen - (nch - 1) * bc.PAGE  # bytes in the last page
                if cls == 0:
                    assert (nch, full, tail) == (1, 0, 1) and n in (1, 5)
                elif cls == 1:
                    assert (nch, full, tail) == (8 * ppw, 8, 0) and 0 < last < bc.PAGE
                elif cls == 2:
                    assert (nch, full, tail) == (8 * ppw + 1, 8, 1) and last <= flen
                else:
                    assert (nch, full, tail) == (24 * ppw + 6, 24, -(-6 // ppw)) and 0 < last < bc.PAGE
                assert grid == (-(-nch // (8 * ppw)) * 8 if img[k] else full + tail)
                if k < 2:
                    padded[k].add(grid % 8 != 0)
            assert len(classes) == 3, (case.id, r)
        assert all(p == {0, 1, 2, 3} for p in per_part), case.id
        assert len(firsts) == 12 and sum(f >= 2 ** 40 for f in firsts) == 3 and bc.BIG_FIRST in firsts
    # each part meets both sizes of class a somewhere, and g[0], g[1] both with and without padding
    assert {(k, 0, few) for k in range(3) for few in (1, 5)} <= seen
    assert padded == {0: {True, False}, 1: {True, False}}
    assert {tuple(b.order) for c in bc.CASES for b in bc.batches(c)} == set(bc.ORDERS)


def test_rule_matches_the_planner():
    """The rule restated in batch_cases.py against the library's planner (pbgpu_plan_describe, no
    GPU): the kind, the image, the page kernel and the page parameters of every part of every case
    and of every near miss."""
    import plan_cases as plc

    family = {None: ("pb_small_kernel",), "whole": ("pb_xsmall_kernel",), "cut": ("pb_xpage_kernel", "pb_ximg_kernel")}
    parts = [(c.id, cfg, env) for c in bc.CASES for cfg, env in c.parts]
    parts += [(name, cfg, env) for name, _, cfg, env in bc.NEAR_MISSES]
    assert len(parts) == 3 * 64 + 9
    for what, cfg, env in parts:
        assert "PBGPU_BATCH" not in env
        name, f = plc.parse(plc.describe(cfg, env))
        assert f["batch"] == bc.batch_kind(cfg, env), what
        assert (f["img_np"] > 0) == bc.has_image(cfg, env), what
        pk = bc.page_kernel(cfg, env)
        flen = bc.frame_length(cfg)
        if flen is None:  # two payloads: no small kernel at all
            assert pk is None and not name.startswith(("pb_small", "pb_xsmall", "pb_xpage", "pb_ximg")), what
            continue
        assert name.startswith(family[pk]), (what, name)
        if pk == "whole":
            assert (1 << f["xs_fp_shift"], f["xs_np"]) == bc.page_params(flen, 256, False, whole=True)[:2], what
        elif pk == "cut":
            assert (f["xp_fpp"], f["xs_np"]) == bc.page_params(flen, 512, False)[:2], what
            if f["img_np"]:
                assert f["img_np"] == bc.page_params(flen, 512, True)[2], what


def test_oracle_builds_every_case_config():
    done = set()
    for case in bc.CASES:
        for k, (cfg, env) in enumerate(case.parts):
            key = (k, case.lens[k])
            if key in done:
                continue
            done.add(key)
            data, off = ob.build(Sequence.from_config(cfg), k, 1, 9, pc.SEED_BASE)
            assert np.array_equal(np.diff(off.astype(np.int64)), np.full(9, case.lens[k])), case.id
            assert len(data) == 9 * case.lens[k]
            assert data[23] == {0: 17, 1: 6, 2: 1}[k]  # the IPv4 protocol byte
    for name, slot, cfg, env in bc.NEAR_MISSES:
        data, off = ob.build(Sequence.from_config(cfg), slot, 1, 9, pc.SEED_BASE)
        want = bc.frame_length(cfg)
        if want is not None:
            assert set(np.diff(off.astype(np.int64))) == {want}, name
        else:
            assert len(off) == 19, name  # two payloads: two frames per iteration
