"""The planner's hook against the real load path: for one case per build kernel (pb_kern),
ctx.kernel_name() after a real pbgpu_load_sequence equals the name in pbgpu_plan_describe's line for
the same input, so what tests/test_plan_cpu.py pins without a GPU is what the GPU path loads.
And one build into an output that is not 4-KiB aligned: the page kernel's launch resolves to
pb_small_kernel (pb_plan_launch), bit-exact against the oracle.  Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest

import batch_cases as bc
import oracle_binding as ob
import pb_configs as pc
import plan_cases as plc
from pbgpu import GpuContext, Sequence
from test_gpu_build_bounds import GUARD, PAINT, Guarded

pytestmark = pytest.mark.gpu

# (kernel, config, environment): one per pb_kern value, and the small family's forced forms
CASES = [
    ("pb_small_kernel", pc.get("udp_fixed_odd_65"), {}),
    ("pb_small_kernel", pc.get("c2_udp_64"), {"PBGPU_KERNEL": "linear"}),
    ("pb_xsmall_kernel", pc.get("c2_udp_64"), {}),
    ("pb_xpage_kernel", pc.get("c4_tcp_syn"), {}),
    ("pb_xpage_kernel", pc.get("c5_icmp_echo"), {}),
    ("pb_ximg_kernel", pc.get("c5_icmp_echo"), {"PBGPU_XP_IMG": "2"}),
    ("pb_gpf_kernel", pc.get("c2_udp_1500"), {"PBGPU_KERNEL": "gpf"}),
    ("pb_stage_kernel", pc.get("tcp_static_string_1400"), {}),
    ("pb_vstage_kernel", plc.icmp00_var(), {}),
    ("pb_fstage_kernel", pc.get("c2_udp_1500"), {}),
    ("pb_vline_kernel", pc.get("c3_udp_var"), {}),
    ("pb_vpage_kernel", pc.get("c3_udp_var"), {"PBGPU_KERNEL": "vpage"}),
]
N_UNALIGNED = 4096


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


@pytest.mark.parametrize("kernel,cfg,env", CASES, ids=["%s-%s" % (c[0], plc.env_id(c[2])) for c in CASES])
def test_loaded_kernel_is_the_planned_one(ctx, kernel, cfg, env):
    with plc.environment(env):
        ctx.load_sequence(plc.SLOT, Sequence.from_config(cfg), pc.SEED_BASE)
    name, fields = plc.parse(plc.describe(cfg, env))
    assert name.startswith(kernel + "<"), name
    assert ctx.kernel_name(plc.SLOT) == name
    assert ctx.build_size(plc.SLOT, 1)[0] == fields["fpi"]


def test_every_kernel_has_a_case():
    assert {c[0] for c in CASES} == {"pb_small_kernel", "pb_xsmall_kernel", "pb_xpage_kernel", "pb_ximg_kernel",
                                     "pb_gpf_kernel", "pb_stage_kernel", "pb_vstage_kernel", "pb_fstage_kernel",
                                     "pb_vline_kernel", "pb_vpage_kernel"}
    assert bc.has_image(pc.get("c5_icmp_echo"), {})


def test_unaligned_output_falls_back_to_the_linear_kernel(ctx):
    """4096 64-B frames into a window 64 B past a page boundary: pb_xsmall_kernel's pages cannot
    be used, the build runs pb_small_kernel, and the bytes around the window stay untouched."""
    cfg = pc.get("c2_udp_64")
    seq = Sequence.from_config(cfg)
    with plc.environment({}):
        ctx.load_sequence(plc.SLOT, seq, pc.SEED_BASE)
    assert ctx.kernel_name(plc.SLOT).startswith("pb_xsmall_kernel<")
    nf, mb = ctx.build_size(plc.SLOT, N_UNALIGNED)
    g = Guarded(ctx, nf, mb - 16 + 4096)
    try:
        win = g.view(data=g.B.f.data + GUARD + 64, capacity_bytes=mb - 16, capacity_frames=nf)
        assert int(win.f.data) % 4096 == 64
        ctx.build(plc.SLOT, 77, N_UNALIGNED, win)
        ctx.sync()
        o_data, o_off = ob.build(seq, plc.SLOT, 77, N_UNALIGNED, pc.SEED_BASE)
        assert win.total_bytes() == len(o_data) == 64 * N_UNALIGNED
        whole = g.whole()
        at = GUARD + 64
        assert np.array_equal(whole[at:at + len(o_data)], o_data)
        assert (whole[:at] == PAINT).all() and (whole[at + len(o_data):] == PAINT).all()
    finally:
        g.free()
