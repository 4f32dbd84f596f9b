"""The planner on the CPU: pbgpu_plan_describe (pb_compile + pb_make_plan, no context, no device)
against tests/golden/plan_lines.json, the lines a real pbgpu_load_sequence gave for every case of
tests/plan_cases.py on the commit before the planner existed (the field printer pasted at the end
of that commit's pbgpu_load_sequence, run once on the MI355X; the golden's "recorded_on").  A line
is the kernel's name and every shape field the kernel reads, so a planner that picks another
kernel or another launch shape for any case fails here, without a GPU."""
import copy

import pytest

import pb_configs as pc
import pbgpu
import plan_cases as plc

EINVAL = -22
CASES = plc.cases()


@pytest.fixture(scope="module")
def golden():
    return plc.golden()


def test_table_and_golden_have_the_same_cases(golden):
    assert {c[0] for c in CASES} == set(golden)
    assert len(CASES) > 1500


def test_every_kernel_is_in_the_table(golden):
    kernels = {plc.parse(line)[0].split("<")[0] for line in golden.values()}
    assert kernels == {"pb_small_kernel", "pb_xsmall_kernel", "pb_xpage_kernel", "pb_ximg_kernel", "pb_gpf_kernel",
                       "pb_stage_kernel", "pb_vstage_kernel", "pb_fstage_kernel", "pb_vline_kernel", "pb_vpage_kernel"}


def test_planner_reproduces_every_golden_line(golden):
    bad = []
    for cid, cfg, env, rule, fold in CASES:
        line = plc.describe(cfg, env, rule, fold)
        if line != golden[cid]:
            bad.append((cid, line, golden[cid]))
    assert not bad, "%d of %d differ; first: %r" % (len(bad), len(CASES), bad[0])


def _refused(cfg):
    with pytest.raises(pbgpu.PbError) as e:
        plc.describe(cfg, {})
    return e.value.code


def test_refusals():
    """-EINVAL exactly where pbgpu_load_sequence refuses: a TTL or ID range upside down, no
    destination address, a payload range upside down, a payload past PB_MAX_PCKT_LEN."""
    base = pc.get("c2_udp_64")
    plc.describe(base, {})
    for key, rng in (("ttl", {"min": 65, "max": 64}), ("id", {"min": 2, "max": 1})):
        cfg = copy.deepcopy(base)
        cfg["ip"][key] = rng
        assert _refused(cfg) == EINVAL, key
    cfg = copy.deepcopy(base)
    del cfg["ip"]["dip"]
    assert _refused(cfg) == EINVAL
    for pl in ({"length": {"min": 9, "max": 8}}, {"isstatic": 1, "length": {"min": 9, "max": 8}},
               {"length": {"min": 0, "max": 65535 - 42 + 1}}, {"exact": "41 " * (65535 - 42 + 1)},
               {"exact": "A" * (65535 - 42 + 1), "isstring": 1}):
        cfg = copy.deepcopy(base)
        cfg["payloads"] = [pl]
        assert _refused(cfg) == EINVAL, str(pl)[:40]
    cfg = copy.deepcopy(base)
    cfg["payloads"] = [{"exact": "41 " * (65535 - 42)}]  # the longest payload loads
    assert plc.parse(plc.describe(cfg, {}))[0].startswith("pb_gpf_kernel<")


def test_null_arguments_rejected():
    lib = pbgpu.load_library()
    seq = pbgpu.Sequence.from_config(pc.get("c2_udp_64"))
    assert lib.pbgpu_plan_describe(0, None, None, 0, None, 0) == EINVAL
    assert lib.pbgpu_plan_describe(pbgpu.MAX_SEQUENCES, seq.c, None, 0, b"x" * 8, 8) == EINVAL
