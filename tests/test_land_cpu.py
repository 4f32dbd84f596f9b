"""The landing model (tests/pyland.py) on hand-written cases, and the input sets of
tests/test_gpu_landing.py: what they cover and how much of a tight slot they leave unspecified."""
import numpy as np
import pytest

import pyland as pl


def u8(*v):
    return np.array(v, dtype=np.uint8)


def test_frames_land_in_their_slots_and_nothing_else_changes():
    frames = [u8(1, 2, 3), u8(), u8(4, 5, 6, 7, 8), u8(9)]
    before = np.full(32, 0xEE, dtype=np.uint8)
    after, lens = pl.land(before, frames, 5, 2, 1, 3, base=1)
    want = np.full(32, 0xEE, dtype=np.uint8)
    want[16:21] = (4, 5, 6, 7, 8)  # frame 2 in slot 3 at 1 + 3 * 5
    want[21] = 9                   # frame 3 in slot 4
    assert np.array_equal(after, want)  # frame 1 is empty: slot 2 keeps its bytes
    assert lens.dtype == np.uint16 and lens.tolist() == [0, 5, 1]
    assert (before == 0xEE).all()  # the input is not written


def test_n_zero_and_a_frame_longer_than_its_slot():
    before = np.arange(16, dtype=np.uint8)
    after, lens = pl.land(before, [u8(1, 2, 3)], 2, 0, 0, 0)
    assert np.array_equal(after, before) and len(lens) == 0
    with pytest.raises(AssertionError):
        pl.land(before, [u8(1, 2, 3)], 2, 0, 0, 1)
    with pytest.raises(AssertionError):  # the last slot would pass the end of the UMEM
        pl.land(before, [u8(1, 2, 3), u8(4)], 4, 3, 0, 2)


def test_tight_slots_carry_the_stream_and_mask_what_lies_past_it():
    frames = [u8(10, 11, 12), u8(20, 21, 22), u8(30, 31, 32)]
    stream = np.concatenate(frames)
    before = np.full(20, 0xEE, dtype=np.uint8)
    after, lens, mask = pl.land(before, frames, 5, 1, 1, 2, base=2, whole=True, stream=stream)
    want = np.full(20, 0xEE, dtype=np.uint8)
    want[7:12] = (20, 21, 22, 30, 31)  # frame 1, then the stream's next two bytes
    want[12:15] = (30, 31, 32)         # frame 2; the stream ends with it
    assert lens.tolist() == [3, 3]
    assert np.array_equal(after[~mask], want[~mask])
    assert np.flatnonzero(mask).tolist() == [15, 16]  # the last slot's two filler bytes
    # a stream that goes on (the landing stops short of the buffer's last frame) leaves no mask
    after, lens, mask = pl.land(before, frames, 5, 0, 0, 2, whole=True, stream=stream)
    assert not mask.any()
    assert after[:10].tolist() == [10, 11, 12, 20, 21, 20, 21, 22, 30, 31]


def test_frame_bytes_have_no_short_period():
    a = pl.frame_bytes(7, 4096)
    for shift in range(1, 300):
        assert (a[shift:] != a[:-shift]).mean() > 0.9, shift
    b = pl.frame_bytes(8, 4096)
    assert (a != b).mean() > 0.9
    assert len(np.unique(a)) == 256
    assert np.array_equal(a[:100], pl.frame_bytes(7, 100))


def test_variable_set_crosses_every_length_with_every_source_offset():
    lengths, blocks = pl.var_blocks()
    off = np.concatenate([[0], np.cumsum(lengths)])
    seen = set()
    for k, (first, n) in enumerate(blocks):
        assert first > 0 and int(off[first]) % 16 == k
        assert lengths[first:first + n] == pl.VAR_SHORT + pl.VAR_LONG
        seen |= {(lengths[f], int(off[f]) % 16) for f in range(first, first + n)}
    assert blocks[-1][0] + blocks[-1][1] == len(lengths)  # the last landing runs to the buffer's last frame
    for length in pl.VAR_SHORT + pl.VAR_LONG:
        assert {o for (ln, o) in seen if ln == length} == set(range(16)), length
    assert max(lengths) == pl.VAR_LMAX
    assert pl.VAR_STRIDES == [4096, 4097, 4098, 4099]
    assert int(off[-1]) < 1 << 20 and len(lengths) * max(pl.VAR_STRIDES) < 8 << 20


def test_fixed_set_covers_every_stride_class():
    for flen in pl.FIXED_LENS:
        s = pl.fixed_strides(flen)
        assert {flen, flen + 1, flen + 3, pl.round64(flen), pl.round64(flen) + 1, 4096} == set(s)
        assert pl.is_tight(flen, flen) and pl.is_tight(flen, pl.round64(flen))
        assert not pl.is_tight(flen, pl.round64(flen) + 1) and min(s) >= flen
    assert {f % 4 for f in pl.FIXED_LENS} == {0, 1, 2, 3}
    assert any(s % 4 for f in pl.FIXED_LENS for s in pl.fixed_strides(f))


@pytest.mark.parametrize("flen", pl.FIXED_LENS)
def test_unspecified_bytes_stay_within_the_cap(flen):
    """Only filler whose stream position is at or past the buffer's total may be left out of a
    comparison.  That is at most stride - flen <= 63 bytes of a slot and the same stretch of at most
    63 stream positions behind the total in every slot; the slot of the buffer's d-th frame from the
    end has stride - flen - d * flen of them, so a landing has more than 63 in all only where
    several frames fit in one slot's filler (flen < 32)."""
    n = pl.FIXED_N
    frames = [pl.frame_bytes(j, flen) for j in range(n)]
    stream = np.concatenate(frames)
    for stride in pl.fixed_strides(flen):
        if not pl.is_tight(flen, stride):
            continue
        for base in pl.FIXED_BASES:
            for first, cnt in pl.fixed_ranges(n):
                before = np.zeros(base + (cnt + 2) * stride, dtype=np.uint8)
                after, lens, mask = pl.land(before, frames, stride, 1, first, cnt, base=base, whole=True,
                                            stream=stream)
                assert (lens == flen).all()
                pl.check_cap(mask, flen, stride, 1, first, cnt, base, len(stream))
                # every range of the set ends with the buffer's last frame
                per_slot = [max(0, stride - flen - d * flen) for d in range(cnt)]
                assert mask.sum() == sum(per_slot) and per_slot[0] == stride - flen <= 63
                if 2 * flen >= stride:
                    assert mask.sum() <= 63  # one frame's filler at the most
                slots = after[base + stride:base + (cnt + 1) * stride].reshape(cnt, stride)
                want = np.concatenate([stream[first * flen:], np.zeros(stride, dtype=np.uint8)])
                for j in (0, cnt // 2, cnt - 1):  # a slot is the stream from its frame on, while it lasts
                    assert np.array_equal(slots[j], want[j * flen:j * flen + stride])
