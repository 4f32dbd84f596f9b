"""The verify tests' own tools (verify_ref.py) without a GPU: the clean-frame maker's codes under
the reference and the C checker, the facts about mutants the GPU tests build on, and the case
table: which kernel path each tested shape takes, from pbgpu_verify's launch arithmetic restated
over the constants pb_device.h defines.  A change of those constants breaks the table here; it
does not silently move a GPU case to another path."""
import numpy as np
import pytest

import verify_ref as vr
from verify_ref import clean_code, good_frame, ref_code, ref_one

LENGTHS = list(range(34, 400)) + [1499, 1500, 1514, 2049, 4096, 9043, 65535]


@pytest.mark.parametrize("fill", [None, 0xFF, 0x00], ids=["random", "ff", "00"])
@pytest.mark.parametrize("proto", [17, 6, 1])
def test_good_frame_codes(proto, fill):
    """Code 0 at every length, except a segment shorter than two bytes without a pseudo header."""
    for L in LENGTHS:
        f = good_frame(L, proto, 7, fill)
        assert len(f) == L and (f[12], f[13], f[14], f[23]) == (8, 0, 0x45, proto)
        assert ref_one(f) == clean_code(L, proto), (L, proto, fill)
        assert clean_code(L, proto) == (4 if L < 36 and proto == 1 else 0)


def test_accumulators_at_their_top():
    f = good_frame(65535, 17, 0, 0xFF)
    assert ref_one(f) == 0 and int(np.count_nonzero(f != 0xFF)) <= 12
    raw = np.full(65535, 0xFF, np.uint8)
    assert ref_one(raw) == 6
    assert vr._sum16(raw) == 32767 * 0xFFFF + 0xFF00 < 1 << 32  # what a 32-bit accumulator must hold


def test_short_frames():
    for L in (0, 1, 13, 33):
        assert ref_one(good_frame(64, 17, 3)[:L]) == 8


@pytest.mark.parametrize("proto", [17, 6, 1])
def test_one_byte_mutants(proto):
    """One byte of a clean 1501-B frame changed: bad from byte 14 on, clean before (the Ethernet header)."""
    base = good_frame(1501, proto, 11)
    assert ref_one(base) == 0
    for x in (0x01, 0x80, 0xFF):
        for j in range(1501):
            f = base.copy()
            f[j] ^= x
            code = ref_one(f)
            assert (code != 0) == (j >= 14), (j, x, code)
    for j in range(1501):  # the GPU test's own mutation
        f = base.copy()
        f[j] ^= 1 << (j % 8)
        assert (ref_code(f) != 0) == (j >= 14)


@pytest.mark.parametrize("L,proto", [(40, 17), (98, 1), (1500, 17), (1501, 6), (4097, 17), (9043, 17)])
def test_word_swaps_stay_clean(L, proto):
    base = good_frame(L, proto, 5)
    for seed in range(8):
        g = vr.swap_words(base, seed)
        assert not np.array_equal(g, base) and ref_one(g) == 0


@pytest.mark.parametrize("L,proto", [(98, 1), (1500, 17), (1501, 6), (4097, 17), (9043, 17)])
def test_minus_zero_stays_clean(L, proto):
    for at in (18, 36, 38, L - 2 - (L & 1), 34 + 2 * ((L - 34) // 4)):
        f, g = vr.zero_word_frame(L, proto, 9, at)
        assert ref_one(f) == 0 and ref_one(g) == 0 and int(np.count_nonzero(f != g)) == 2


# ------------------------------------------------------------------ the case table
def test_constants_are_read():
    k = vr.shape_constants()
    assert set(k) == {"PB_VS_STAGE", "PB_VS_BF_MAX", "PB_VST_WT"}
    assert k["PB_VST_WT"] % 64 == 0 and k["PB_VS_STAGE"] % 16 == 0


def test_length_classes():
    """Every length of the per-byte mutant test (L + 1 frames of L bytes) takes the path it is listed under."""
    seen = set()
    for want, lengths in vr.LENGTH_CLASSES:
        for L in lengths:
            assert vr.shape_class(L, L + 1) == want, L
            seen.add(L)
    assert len(seen) == 13 + 13
    # the exact fits: a full window's bytes are the stage's, one byte more is not staged
    k = vr.shape_constants()
    for L in (2048, 4096):
        bf = vr.verify_shape(L, 0, L + 1, L)["bf"]
        assert bf * L == k["PB_VS_STAGE"] and bf * (L + 1) > k["PB_VS_STAGE"]
    # the jumbo samples: about 450 frames, every full window from global memory
    for L in (9043, 65535):
        assert vr.shape_class(L, 449) == (64, "unstaged")


def test_page_kernel_takes_34_to_128():
    for L in (34, 128):
        assert vr.verify_shape(L, 0, 100, L)["kernel"] == "vpg"
    assert vr.verify_shape(129, 0, 100, 129)["kernel"] == "vst"
    assert vr.verify_shape(0, 0, 100, 60)["kernel"] == "vst"  # packed frames, whatever their mean


def test_loop_sizings():
    """The three builds of the loop test: two pages per wave, two windows per workgroup."""
    n = (1 << 21) + (1 << 18)
    sh = vr.verify_shape(60, 0, n, 60)
    assert (sh["kernel"], sh["npages"], sh["per"], sh["grid"]) == ("vpg", 34560, 2, 17280)
    assert vr.verify_shape(60, 0, n - (1 << 18), 60)["per"] == 1  # 2^21 frames alone: one page per wave
    n = 2 * 8 * 16384 + 43
    sh = vr.verify_shape(1500, 0, n, 1500)
    assert (sh["G"], sh["bf"], sh["nw"], sh["wgf"]) == (32, 8, 2, 16) and n % 16 == 11  # ragged: 8 + 3
    assert vr.verify_shape(1500, 0, 2 * 8 * 16384 - 1, 1500)["nw"] == 1
    n = (1 << 18) + 29
    for mean in (800, 824, 850):  # configs[2]: 106..1542 B
        sh = vr.verify_shape(0, 0, n, mean)
        assert (sh["G"], sh["bf"], sh["nw"]) == (32, 8, 2)


def test_sub_range_shapes():
    """A sub-range of a short fixed-length buffer starts in the page its first byte is in."""
    sh = vr.verify_shape(64, 64, 64, 64)
    assert (sh["page0"], sh["npages"], sh["grid"]) == (1, 1, 1)
    sh = vr.verify_shape(60, 68, 2, 60)  # frame 68 straddles byte 4096
    assert (sh["page0"], sh["npages"]) == (0, 2)


def test_packed_mix_classes():
    """The packed mixtures: the mean picks G = 8 / 16, and windows that do not fit the stage sit among
    those that do."""
    for G, n_small in ((8, 2400), (16, 300)):
        frames, jumbo, near = vr.packed_mix(n_small)
        data, off = vr.pack(frames)
        n, mean = len(frames), len(data) // len(frames)
        assert (mean <= 192) if G == 8 else (193 <= mean <= 768)
        assert vr.shape_class(0, n, mean, off) == (G, "both")
        assert len(jumbo) == 10 and len(near) == 4 * 2 + 3 * 3 and len(frames[-1]) == 0
