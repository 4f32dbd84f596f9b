"""The per-frame header fields on every build kernel (tables: tests/field_cases.py; checked without
a GPU by tests/test_field_cases_cpu.py).  Every kernel draws TTL, IPv4 ID, the source range's index,
the source's host bits and the port from one rand_r per iteration with pb_mod on make_div's
constants, loads the range its own way (the hoisted single range, pb_range's table, no table) and
folds the fields into the IPv4 and L4 checksums from its own header placement.

Each case builds one host's sequence under one field variant in slot 5 and asserts the kernel it
ran on, the oracle's offsets and bytes, and that pbgpu_verify finds no bad frame in the built
buffer (under the single-fold rule: as many as the oracle library's checker finds in the oracle's
frames, all by the IPv4 checksum).  The targeted cases build 513 iterations around an iteration where a divisor's residue is
0 or d - 1, or where r0 is the largest of 2^22 iterations, and assert first, on the oracle's frame,
that the window holds that field value.  Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest

import field_cases as fc
import oracle_binding as ob
import pb_configs as pc
from pbgpu import GpuContext, Sequence

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def _oracle(host, cfg, fold, first, n):
    return ob.build(Sequence.from_config(cfg), fc.SLOT, first, n, pc.SEED_BASE, payload_rule=host.rule, iph_fold=fold)


def _check(ctx, monkeypatch, host, cfg, fold, first, n, oracle=None):
    for k, v in host.env.items():
        monkeypatch.setenv(k, v)
    seq = Sequence.from_config(cfg)
    ctx.load_sequence(fc.SLOT, seq, pc.SEED_BASE, payload_rule=host.rule, iph_fold=fold)
    kern = ctx.kernel_name(fc.SLOT)
    assert kern.startswith(host.kernel), kern
    fb = ctx.alloc_frames(*ctx.build_size(fc.SLOT, n))
    try:
        ctx.build(fc.SLOT, first, n, fb)
        ctx.sync()
        g_data, g_off = fb.packed(), fb.offsets()
        checks = fc.verify_checks(cfg)
        res = fb.verify(checks=checks) if checks != 2 else None  # (not for no_csums)
    finally:
        fb.free()
    o_data, o_off = oracle or _oracle(host, cfg, fold, first, n)
    assert np.array_equal(g_off, o_off)
    if not np.array_equal(g_data, o_data):
        bad = int(np.nonzero(g_data != o_data)[0][0])
        f = int(np.searchsorted(o_off, bad, side="right") - 1)
        pytest.fail("first mismatch at frame %d (iteration %d), offset %d" %
                    (f, first + f // seq.frames_per_iter, bad - int(o_off[f])))
    if res is not None:
        # under the single-fold rule a header sum that carries twice leaves a checksum that does not
        # verify, in the oracle's frame too: exactly those frames are bad, by the IPv4 checksum alone
        want_bad = ob.verify_frames(o_data, o_off, 0, len(o_off) - 1) if fold else 0
        assert res.n_checked == len(o_off) - 1 and res.n_bad == want_bad, (res.n_bad, want_bad, res.first_bad)
        assert res.bad_ip_csum == want_bad and res.bad_l4_csum == 0 and res.bad_tot_len == 0


COMBO_CASES = fc.combo_cases()
SINGLE_CASES = fc.single_cases()
TARGET_CASES = fc.target_cases()


@pytest.mark.parametrize("hid,name", COMBO_CASES, ids=["%s-%s" % c for c in COMBO_CASES])
def test_field_combinations(ctx, monkeypatch, hid, name):
    host = fc.HOST[hid]
    cfg, fold = fc.case_cfg(hid, name)
    _check(ctx, monkeypatch, host, cfg, fold, fc.FIRST_ITER, host.n_iter)


@pytest.mark.parametrize("hid,name", SINGLE_CASES, ids=["%s-%s" % c for c in SINGLE_CASES])
def test_one_field_at_a_time(ctx, monkeypatch, hid, name):
    host = fc.HOST[hid]
    cfg, fold = fc.case_cfg(hid, name)
    _check(ctx, monkeypatch, host, cfg, fold, fc.FIRST_ITER, host.n_iter)


@pytest.mark.parametrize("hid,name,tid,k,expect", TARGET_CASES, ids=["%s-%s-%s" % c[:3] for c in TARGET_CASES])
def test_targeted_windows(ctx, monkeypatch, hid, name, tid, k, expect):
    assert k is not None, "no iteration with this residue among 1..2^22"
    host = fc.HOST[hid]
    cfg, fold = fc.case_cfg(hid, name)
    first = fc.window_first(k)
    assert first % 2 == 1 and first <= k < first + fc.WINDOW
    o_data, o_off = _oracle(host, cfg, fold, first, fc.WINDOW)
    f = (k - first) * Sequence.from_config(cfg).frames_per_iter
    frame = o_data[int(o_off[f]):int(o_off[f + 1])]
    assert fc.frame_field(cfg, frame, expect[0], expect[1], fc.draw(pc.SEED_BASE, fc.SLOT, k)), (tid, k, expect)
    _check(ctx, monkeypatch, host, cfg, fold, first, fc.WINDOW, oracle=(o_data, o_off))
