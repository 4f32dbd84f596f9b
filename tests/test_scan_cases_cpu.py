"""tests/scan_cases.py without a GPU: that every case reaches pb_scan_blocks' second pass by the
sources' own constants, that the planner gives each case the kernel and the workgroup size its
arithmetic assumes, that the numpy references agree with the oracle, pyfrag and pyseg, and that the
comparison test_gpu_scan_passes.py uses fails on offsets whose carry into the second pass is lost."""
import os
import re
import shutil

import numpy as np
import pytest

import oracle_binding as ob
import pb_configs as pc
import plan_cases as plc
import pyfrag
import pyseg
import scan_cases as sc
from pbgpu import Sequence

K = sc.constants()
ALL = sc.BUILDS + sc.CUTS
SMALL = 5000


def test_constants_are_the_ones_the_cases_were_sized_for():
    assert K["PASS"] == 1024 * K["IT"] == 8192
    assert K["PB_SCAN_FRAMES_PER_BLOCK"] == 256 * K["PB_SCAN_ITEMS"] == 2048
    assert (K["PB_VL_GRP"], K["PB_FG_WT"], K["PB_FG_CB"], K["PB_VST_SCAN_MIN_WGF"]) == (32, 256, 16, 32)


@pytest.mark.parametrize("case", ALL, ids=[c.id for c in ALL])
def test_every_case_has_its_entries_in_the_second_pass(case):
    n = sc.entries(case)
    assert n > K["PASS"]
    assert n == K["PASS"] + sc.in_pass_2(case) and n <= 2 * K["PASS"]
    # the second pass's first entry is whole and has frames on either side to compare
    nf = case.n if isinstance(case, sc.Cut) else case.frames
    assert sc.boundary(case) + sc.frames_per_entry(case) < nf
    assert [w for w in sc.windows(case) if w[0] < sc.boundary(case) < w[0] + w[1]] == [(sc.boundary(case) - 32, 64)]
    assert sc.windows(case)[0] == (0, 64) and sc.windows(case)[-1] == (nf - 64, 64)


def test_entries_is_the_launch_arithmetic():
    """entries() at and around each stated count, against numbers worked out by hand: 2^23 + 2^20 =
    294,912 workgroups of 32 frames = 9,216 groups of 32; 2^24 + 2^21 = 9,216 blocks of 2,048 frames;
    2^21 + 2^18 = 9,216 rows of 256 frames."""
    for cid in ("vline_wgf32", "vstage_wgf32"):
        b, nf = sc.BUILD[cid], (1 << 23) + (1 << 20) + 5
        assert b.frames == nf
        assert [sc.entries(b, f) for f in (nf, nf - 1, nf - 4, nf - 5, nf - 6, nf + 1019, nf + 1020)] == \
            [9217, 9217, 9217, 9216, 9216, 9217, 9218]
        assert sc.frames_per_entry(b) == 1024 and sc.boundary(b) == 1 << 23
        assert b.wgf >= K["PB_VST_SCAN_MIN_WGF"]  # below it the build takes the 3-pass scan
    b, nf = sc.BUILD["vstage_3pass"], (1 << 24) + (1 << 21) + 5
    assert b.frames == nf
    assert [sc.entries(b, f) for f in (nf, nf - 1, nf - 4, nf - 5, nf + 2043, nf + 2044)] == \
        [9217, 9217, 9217, 9216, 9217, 9218]
    assert sc.frames_per_entry(b) == 2048 and sc.boundary(b) == 1 << 24
    n_src = (1 << 21) + (1 << 18) + 77
    assert sc.SRC.frames == n_src
    for c in sc.CUTS:
        assert (c.first, c.n) in ((0, n_src), (129, n_src - 129)) and c.first + c.n == n_src
        assert [sc.entries(c, f) for f in (n_src, n_src - 1, n_src - 76, n_src - 77, n_src - 129)] == \
            [9217, 9217, 9217, 9216, 9216]
        assert sc.frames_per_entry(c) == 256 and sc.boundary(c) == 1 << 21
        # the whole run's count kernel ends in a workgroup of one row; the second run's workgroups are full
        assert sc.entries(c) % K["PB_FG_CB"] == (0 if c.first else 1)
    # the last row: 77 source frames of the whole run, 204 of the run that leaves out the first 129
    assert [c.n - (1 << 21) - 4 * (1 << 16) for c in sc.CUTS] == [77, 77 - 129, 77, 77 - 129]
    assert (n_src - 129) % 256 == 204
    # the cut source itself is one pass of its own scan
    assert sc.entries(sc.SRC) == 293 and sc.SRC.wgf * K["PB_VL_GRP"] * K["PASS"] > n_src


@pytest.mark.parametrize("name,old,new", [("pbgpu_kernels.hip", "IT = 8,", "IT = 16,"),
                                          ("pbgpu_kernels.hip", "IT = 8,", "IT = 4,"),
                                          ("pb_device.h", "PB_FG_WT 256u", "PB_FG_WT 512u"),
                                          ("pb_device.h", "PB_VL_GRP 32 ", "PB_VL_GRP 64 "),
                                          ("pbgpu.cpp", "PB_SCAN_FRAMES_PER_BLOCK (256 * 8)",
                                           "PB_SCAN_FRAMES_PER_BLOCK (256 * 16)")])
def test_a_changed_constant_changes_entries(tmp_path, monkeypatch, name, old, new):
    """The regexes read what the sources say: on a copy with one constant changed, the case that
    depends on it no longer has PASS + 1025 entries (which the test above then refuses)."""
    for n in ("pbgpu_kernels.hip", "pb_device.h", "pb_plan.h", "pbgpu.cpp"):
        shutil.copy(os.path.join(sc.CSRC, n), tmp_path / n)
    text = (tmp_path / name).read_text()
    assert len(re.findall(re.escape(old), text)) == 1, old
    (tmp_path / name).write_text(text.replace(old, new))
    changed = sc.read_constants(str(tmp_path))
    assert changed != K
    monkeypatch.setattr(sc, "constants", lambda: changed)
    assert any(sc.entries(c) != changed["PASS"] + sc.in_pass_2(c) for c in ALL)


@pytest.mark.parametrize("case", sc.BUILDS + [sc.SRC], ids=[b.id for b in sc.BUILDS + [sc.SRC]])
def test_planner_gives_the_kernel_and_workgroup_the_arithmetic_assumes(case):
    name, f = plc.parse(plc.describe(sc.config(case), case.env))
    assert name.startswith(case.kernel + "<"), name
    assert (f["fixed_len"], f["fpi"], f["min_flen"], f["max_flen"]) == (0, 1, 42 + case.lo, 42 + case.hi)
    assert f["vl_wgf" if case.kernel == "pb_vline_kernel" else "stage_wgf"] == case.wgf
    # len_wgf: the length pass's workgroup (pb_plan_len_wgf), 0 where the build takes the 3-pass scan
    assert f["len_wgf"] == (0 if case.scan == "3pass" else case.wgf)


@pytest.mark.parametrize("case", sc.BUILDS + [sc.SRC], ids=[b.id for b in sc.BUILDS + [sc.SRC]])
def test_vectorised_lengths_are_the_oracles(case):
    seq = Sequence.from_config(sc.config(case))
    for first in (sc.FIRST_ITER, sc.FIRST_ITER + sc.boundary(case) - 32):
        _, off = ob.build(seq, sc.SLOT, first, SMALL, pc.SEED_BASE)
        L = sc.build_lengths(case, SMALL, first)
        assert L.min() >= 42 + case.lo and L.max() == 42 + case.hi
        sc.assert_offsets(sc.offsets_of(L), off, case.id)


@pytest.mark.parametrize("kind,opt", [("frag", 68), ("seg", 32)])
@pytest.mark.parametrize("first", [0, sc.SKIP])
def test_vectorised_cut_references_are_pyfrags_and_pysegs(kind, opt, first):
    seq = Sequence.from_config(sc.config(sc.SRC))
    frames = ob.frames(seq, sc.SLOT, sc.FIRST_ITER + first, SMALL, pc.SEED_BASE)
    L = sc.source_lengths()[first:first + SMALL]
    assert [len(f) for f in frames] == L.tolist()
    out, cnt = pyfrag.fragment_all(frames, opt) if kind == "frag" else pyseg.segment_all(frames, opt)
    ref = sc.cut_reference(kind, opt, L)
    assert ref.counts == cnt
    assert ref.out_len.tolist() == [len(f) for f in out]
    sc.assert_offsets(ref.off, np.concatenate([[0], np.cumsum([len(f) for f in out])]).astype(np.uint64), kind)
    per = [len(pyfrag.fragment(f, opt) if kind == "frag" else pyseg.segment(f, opt)) for f in frames]
    assert ref.K.tolist() == per and set(per) == {1, 2, 3}
    assert ref.first_rec.tolist() == np.concatenate([[0], np.cumsum(per)]).tolist()
    if kind == "seg":  # the inserted bytes, the segmenter's second scan: 42 per extra segment
        assert cnt["out_bytes"] - int(L.sum()) == 42 * (cnt["n_out"] - SMALL) > 0


def test_cut_row_sums_differ_from_row_to_row():
    """Both cuts' row sums around the pass boundary are no constant: a carry of the wrong rows'
    sums is another number."""
    for c in sc.CUTS:
        ref = sc.cut_reference(c.kind, c.opt, sc.source_lengths()[c.first:c.first + 8200 * 256])
        rows = ref.K.reshape(-1, 256).sum(axis=1)
        assert len(set(rows[8180:8200].tolist())) > 5
        assert ref.counts["out_min_len"] < ref.counts["out_max_len"]


@pytest.mark.parametrize("case", sc.BUILDS, ids=[b.id for b in sc.BUILDS])
def test_comparison_detects_a_dropped_carry_in_a_build(case):
    off = sc.offsets_of(sc.build_lengths(case))
    sc.assert_offsets(off.copy(), off, case.id)
    bad = sc.drop_carry(off, sc.boundary(case))
    assert np.array_equal(bad[:sc.boundary(case)], off[:sc.boundary(case)]) and bad[sc.boundary(case)] == 0
    with pytest.raises(AssertionError, match="first at entry %d:" % sc.boundary(case)):
        sc.assert_offsets(bad, off, case.id)
    assert int(bad[-1]) != int(off[-1])  # total_bytes() differs as well


@pytest.mark.parametrize("case", sc.CUTS, ids=[c.id for c in sc.CUTS])
def test_comparison_detects_a_dropped_carry_in_a_cut(case):
    ref = sc.cut_case_reference(case)
    at = int(ref.first_rec[sc.boundary(case)])  # the first record of row PASS
    assert 0 < at < ref.counts["n_out"]
    with pytest.raises(AssertionError, match="first at entry %d:" % at):
        sc.assert_offsets(sc.drop_carry(ref.off, at), ref.off, case.id)
