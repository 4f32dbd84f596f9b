"""The inputs of test_gpu_repack_pages.py reach what the page loops of the five repack writers do only
with several pages per workgroup.  No GPU: every figure comes from the Python references' record
offsets, the window and header-slot sizes read out of csrc/pb_device.h, and repack_cases.geometry(),
which walks a launch the way the kernels do.  These are conditions on the inputs: no change of a
kernel can make them pass.  The references' outputs also pass their own independent checkers."""
import struct

import pytest

import pyfrag
import pypcap
import pyseg
import pyverify
import pyxlat
import repack_cases as rc
from repack_cases import CASES, PAGE, PERS, WRITERS, case_geometry, case_id, source

SIZES = rc.device_sizes()


def geos(writer, per, kinds=None):
    """(case, geometry) of the writer's cases that run at `per` pages per workgroup."""
    return [(c, case_geometry(c, per)) for c in CASES
            if c.writer == writer and per in c.pers and (kinds is None or c.kind in kinds)]


def test_sizes_come_from_the_device_header():
    assert set(SIZES) == {"PB_PC_WIN", "PB_EN_WIN", "PB_EN_HREC", "PB_FG_WIN", "PB_FG_HREC", "PB_XL_WIN", "PB_XL_HREC"}
    assert all(60 < v < 1024 for v in SIZES.values())
    # a window of the shortest records covers fewer bytes than the 3 and the 32 pages of (a)
    for w, rec in (("pcap", 17), ("encap", 18), ("frag", 14), ("seg", 14), ("xlat", 62)):
        assert SIZES[rc.WIN_OF[w]] * rec < 3 * PAGE


def test_geometry_on_hand_made_records():
    """geometry() itself, on records small enough to follow by hand: 290 records of 100 B and a
    window of 50 (it reaches 4,900 B) at 4 pages per workgroup."""
    g = rc.geometry([100] * 290, 0, 4, 50)
    assert (g.total, g.npages, g.grid, g.multi, g.end_page, g.last_pages) == (29000, 8, 2, 2, 3, 4)
    # workgroup 0: the window from record 0 ends at byte 4900, inside page 1, so it moves there, to record
    # 40, and again on pages 2 and 3; workgroup 1 starts at record 163 and moves on pages 5 (to record
    # 204) and 6 (to 245); on page 7 the window's last entry would be record 294, past the output's end
    assert g.moves == [3, 2] and g.move_pages == [1, 2, 3, 5, 6]
    assert g.carried == [100] and g.nostart == [] and g.max_touch == 42  # page 7's first byte is 72 B into record 286
    # records that are whole pages, one of three pages and a byte, and a short one, at 2 pages per workgroup
    g = rc.geometry([PAGE] * 5 + [3 * PAGE + 1, 10], 0, 2, None)
    assert (g.total, g.npages, g.grid) == (8 * PAGE + 11, 9, 5)
    assert (g.start0, g.end4095, g.nostart, g.moves) == (3, 2, [7], [0] * 5)  # starts on pages 1, 3, 5; ends on 1, 3
    assert g.carried == [3 * PAGE + 1] and (g.end_page, g.last_pages) == (0, 1)
    # the pcap file header: record 0 starts at byte 24
    g = rc.geometry([PAGE - 24, PAGE], 24, 2, 258)
    assert (g.total, g.start0, g.end4095) == (2 * PAGE, 1, 1)


@pytest.mark.parametrize("writer", WRITERS)
def test_several_pages_per_workgroup(writer):
    for per in PERS:
        for c, g in geos(writer, per):
            assert g.multi >= 2 and g.npages > per, case_id(c)


@pytest.mark.parametrize("writer", WRITERS)
def test_a_window_moves_inside_a_workgroup(writer):
    """(a).  At 3 pages per workgroup a window can move twice at the most (on the second and the third
    page), so the three moves are asked at 32 and both at 3.  VXLAN's shortest record is 64 B: a window
    of them covers four pages, VLAN's runs stand for the encapsulator at 3."""
    for per, least in ((3, 2), (32, 3)):
        gs = geos(writer, per, ("runs",))
        assert max(max(g.moves) for _, g in gs) >= least
        assert max(g.moves_after_long for _, g in gs) >= 1
        # and where a window moves, it moved because it ran out: on more pages than one per workgroup
        assert max(len(g.move_pages) for _, g in gs) >= 20
    # the runs of short records put as many records into one page as the header slots allow for
    short = 16 + rc.SHORT[writer] if writer == "pcap" else {"encap": 18, "xlat": 62}.get(writer, 14)
    most = max(g.max_touch for _, g in geos(writer, 32, ("runs",)))
    assert most >= PAGE // short
    if rc.HREC_OF[writer]:
        assert most <= SIZES[rc.HREC_OF[writer]]
    assert most < SIZES[rc.WIN_OF[writer]]


@pytest.mark.parametrize("writer", WRITERS)
def test_pages_carried_without_a_move(writer):
    """(b): a record of about 1514 B and one of about 9 KB hold the first byte of a later page of a
    workgroup, and the window stays."""
    for per in PERS:
        carried = set()
        for _, g in geos(writer, per, ("runs",)):
            carried |= set(g.carried)
        assert any(1500 <= x <= 1600 for x in carried) and any(9000 <= x <= 9200 for x in carried)


@pytest.mark.parametrize("writer", WRITERS)
def test_pages_in_which_no_record_starts(writer):
    """(c): the longest frame the writer takes is in every runs source; its pcap record, its
    encapsulation and its translation cover 15 whole pages, and in the fragmenter's and the segmenter's
    output (whose records are no longer than the mtu, or the mss and the headers) a copied 9-KB frame
    covers one."""
    for c in CASES:
        if c.writer == writer and c.kind == "runs":
            assert max(len(f) for f in source(c)[0]) == rc.biggest(writer, c.oname)
    for per in PERS:
        n = max(len(g.nostart) for _, g in geos(writer, per, ("runs",)))
        assert n >= (1 if writer in ("frag", "seg") else 15)
    if writer == "frag":
        assert "1500" in rc.RUNS_OPTS["frag"]
    if writer == "seg":
        assert {"8", "1460f2"} <= set(rc.RUNS_OPTS["seg"])


@pytest.mark.parametrize("writer", WRITERS)
def test_record_edges_on_page_edges(writer):
    """(d), in every runs source and at every `per`."""
    for per in PERS:
        for c, g in geos(writer, per, ("runs",)):
            assert g.start0 >= 1 and g.end4095 >= 1, case_id(c)


@pytest.mark.parametrize("writer", WRITERS)
def test_ragged_ends(writer):
    """(e)"""
    for per in PERS:
        by = {c.arg: g for c, g in geos(writer, per, ("ragged%d" % per,))}
        assert set(by) == set(rc.RAGGED)
        assert by["exact"].total % (per * PAGE) == 0 and by["exact"].total == by["minus16"].total + 16 == \
            by["plus16"].total - 16
        assert by["exact"].end_page == by["minus16"].end_page == per - 1  # a workgroup's last page
        assert by["exact"].last_pages == per
        assert (by["plus16"].end_page, by["plus16"].last_pages) == (0, 1)  # its first, in a short last workgroup
        assert (by["middle"].end_page, by["middle"].last_pages) == (1, 2)  # a middle one from per 3 on
        assert by["middle"].total % 16 and 2 < per + (per == 2)
        ends = {g.end_page for _, g in geos(writer, per)}
        assert {0, per - 1} <= ends and (per == 2 or ends - {0, per - 1})


@pytest.mark.parametrize("writer", WRITERS)
def test_fixed_length_sources(writer):
    """(f)"""
    fixed = [c for c in CASES if c.writer == writer and c.kind == "fixed"]
    lens = {c.arg for c in fixed}
    want = {14, 60, 64, 1500, 1621, 9043, 65535}
    if writer == "xlat":  # takes 42 B to 65,515 B
        want = want - {14, 65535} | {65515}
    if writer == "encap":  # takes what stays a 16-bit length with its header
        want = want - {65535} | {65531, 65485}
    assert lens == want
    assert any(c.first > 0 for c in fixed)
    for c in fixed:
        frames, flen, first, n = source(c)
        assert flen == c.arg and all(len(f) == flen for f in frames) and first == c.first and first + n <= len(frames)
        assert rc.windowed(c) == (writer in ("frag", "seg") and not rc.copy_path(c))
    if writer in ("frag", "seg"):
        copies = [c for c in fixed if rc.copy_path(c)]
        assert {c.arg for c in copies} >= {14, 60, 1500} and any(c.first for c in copies)
        for c in copies:
            assert rc.reference(c) == source(c)[0][c.first:c.first + source(c)[3]]
        assert any(not rc.copy_path(c) for c in fixed)


def test_option_sets():
    """(g)"""
    used = {w: {c.oname for c in CASES if c.writer == w} for w in WRITERS}
    assert used["encap"] == {"vlan", "vxlan"} and used["xlat"] == {"label", "hash"} and used["pcap"] == {"hdr", "nohdr"}
    assert {rc.OPTS["frag"][o] for o in used["frag"]} >= {(576, False), (576, True), (1500, False), (1500, True)}
    seg = {rc.OPTS["seg"][o] for o in used["seg"]}
    assert {m for m, _ in seg} == {8, 536, 1460} and {f for _, f in seg} == {0, 1, 2, 3}
    for c in CASES:
        if c.writer == "seg" and c.kind in ("runs", "zoo"):  # TCP headers of 20, 24 and 60 B in one batch
            hs = {pyseg.l4_header_len(f) for f in source(c)[0] if len(f) > 200 and pyseg.classify(f, 1460) == "tcp"}
            assert {20, 24, 60} <= hs, case_id(c)
        if c.writer == "frag" and c.kind in ("runs", "zoo"):  # DF frames, so that ignore_df decides something
            assert any(pyfrag.classify(f, 1500) == "df" for f in source(c)[0]), case_id(c)


def _split_back(frames, refs, count):
    at = 0
    for f in frames:
        k = count(f)
        yield f, refs[at:at + k]
        at += k
    assert at == len(refs)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind in ("runs", "zoo") or c.arg == "middle"], ids=case_id)
def test_references_pass_their_own_checkers(case):
    frames, _, first, n = source(case)
    frames, refs = frames[first:first + n], rc.reference(case)
    o = rc.OPTS[case.writer][case.oname]
    if case.writer == "seg":
        pyseg.check_all(frames, refs, *o)
    elif case.writer == "xlat":
        assert all(pyxlat.check6(r) for r in refs)
    elif case.writer == "frag":
        for f, parts in _split_back(frames, refs, lambda f: len(pyfrag.fragment(f, *o))):
            if len(parts) > 1 and struct.unpack("!H", f[20:22])[0] & 0x3FFF:
                # the source is a fragment itself, and reassemble() takes whole packets only
                assert b"".join(x[34:] for x in parts) == f[34:] and all(x[:14] == f[:14] for x in parts)
            else:
                assert pyfrag.reassemble(parts) == f
            assert len(parts) == 1 or all(pyverify.ip_csum_ok(x) and len(x) - 14 <= o[0] for x in parts)
    elif case.writer == "encap":
        vlan = case.oname == "vlan"
        for f, r in zip(frames, refs):
            assert (r[:12] + r[16:] if vlan else r[50:]) == f
            assert vlan or (pyverify.ip_csum_ok(r) and struct.unpack("!H", r[16:18])[0] == len(r) - 14)
    else:
        stream = pypcap.pcap_stream(frames, o["t0_ns"], o["step_ps"], 0, True, o.get("nsec", False))
        nsec, recs = pypcap.read_pcap(stream)
        assert nsec == o.get("nsec", False) and [r[2] for r in recs] == frames
        assert [16 + len(f) for f in frames] == [len(r) for r in refs]
