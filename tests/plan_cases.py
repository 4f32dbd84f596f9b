"""The planner's case table (pb_plan.cpp: pb_compile + pb_make_plan), no GPU here.  Each case is
(id, config, environment, payload rule, IPv4 fold) and maps to one line of
tests/golden/plan_lines.json: the kernel's name and the shape fields pbgpu_plan_describe prints.
tests/test_plan_cpu.py holds the library against the golden lines, tests/test_gpu_plan.py the hook
against a real load."""
import contextlib
import json
import os

import batch_cases as bc
import pb_configs as pc
import pbgpu
import static_cases as sc
import test_gpu_kernels as tk

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_lines.json")
SLOT = 5

# one override each, on every config
ENVS = [{"PBGPU_XP_FORCE": "1"}, {"PBGPU_XP_STATIC": "0"}, {"PBGPU_XP_WGT": "256"}, {"PBGPU_XP_NP": "3"},
        {"PBGPU_XP_IMG": "0"}, {"PBGPU_XP_IMG": "2"}, {"PBGPU_SMALL_WGT": "128"}, {"PBGPU_VL_WGF": "64"},
        {"PBGPU_FPW": "32"}, {"PBGPU_WGT": "64"}]
FIXED_LENS = (129, 132, 1500, 1501, 9000)
LONG_PAYLOADS = (57000, 60000, 65000)


def env_id(env):
    return ",".join("%s=%s" % (k[6:], v) for k, v in sorted(env.items())) or "default"


def one_payload(proto, flen, static=False):
    """`proto` frames of flen bytes with one random or one static-random payload."""
    cfg = pc.get(sc.BASE[proto])
    cfg["payloads"] = [{"isstatic": int(static), "length": {"min": flen - sc.HL[proto], "max": flen - sc.HL[proto]}}]
    return cfg


def icmp00_var():
    """ICMP type 0 / code 0, variable length: pb_vline_kernel's orbit sums cannot serve it."""
    cfg = pc.get("c5_icmp_echo")
    cfg["icmp"] = {"type": 0, "code": 0}
    cfg["payloads"] = [{"length": {"min": 64, "max": 1500}}]
    return cfg


def cases():
    """[(id, cfg, env, rule, fold)], ids unique."""
    out = []

    def add(cid, cfg, env=None, rule=0, fold=0):
        out.append((cid, cfg, dict(env or {}), rule, fold))

    for name in pc.ALL:
        add("cfg/%s" % name, pc.get(name))
        for shape, env, _ in tk.SHAPES:
            add("shape/%s/%s" % (shape, name), pc.get(name), env)
        for env in ENVS:
            add("env/%s/%s" % (env_id(env), name), pc.get(name), env)
    for shape, env in tk.FST_SHAPES:
        for proto in ("udp", "tcp", "icmp"):
            for flen in tk.FST_LENS:
                add("fst/%s/%s_%d" % (shape, proto, flen), one_payload(proto, flen), env)
    for name, rule, fold in pc.RULE_CASES:
        add("rule/%s/r%d_f%d" % (name, rule, fold), pc.get(name), {}, rule, fold)
        if (rule, fold) != (1, 0):
            add("rule/%s/r1_f0" % name, pc.get(name), {}, 1, 0)
    for flen in range(43, 131):
        for static in (False, True):
            add("udp1/%d_%s" % (flen, "static" if static else "random"), one_payload("udp", flen, static))
    for flen in range(55, 67):
        add("tcp1/%d" % flen, one_payload("tcp", flen))
    for flen in FIXED_LENS:
        for static in (False, True):
            add("fixed/%d_%s" % (flen, "static" if static else "random"), one_payload("udp", flen, static))
    for plen in LONG_PAYLOADS:
        for static in (False, True):
            add("long/%d_%s" % (plen, "static" if static else "random"), one_payload("udp", plen + 42, static))
    add("icmp00_var", icmp00_var())
    # tests/static_cases.py: every case, with its first pattern
    for cid, proto, flen, form, pats, want in sc.small_cases():
        add("static/small/%s" % cid, sc.static_cfg(proto, sc.pattern(pats[0], flen - sc.HL[proto])), sc.SMALL_FORMS[form])
    for cid, proto, csum, flen, env, pats, want in sc.stage_cases():
        add("static/stage/%s" % cid, sc.static_cfg(proto, sc.pattern(pats[0], flen - sc.HL[proto]), csum), env)
    for cid, proto, plen, env, pats, counts, want in sc.gpf_cases():
        add("static/gpf/%s" % cid, sc.static_cfg(proto, sc.pattern(pats[0], plen)), env)
    for cid, proto, which, env, rule, counts, want in sc.mixed_cases():
        add("static/mixed/%s" % cid, sc.mixed_cfg(proto, which), env, rule)
    # tests/batch_cases.py: every part of every case, and the near misses
    for case in bc.CASES:
        for k, (cfg, env) in enumerate(case.parts):
            add("batch/%s/%d" % (case.id, k), cfg, env)
    for name, slot, cfg, env in bc.NEAR_MISSES:
        add("batch/miss/%s" % name, cfg, env)
    assert len({c[0] for c in out}) == len(out)
    return out


def static_expectations():
    """{case id: (expected kernel name, exact?)} of the static_cases entries above."""
    out = {}
    for c in sc.small_cases():
        out["static/small/%s" % c[0]] = (c[-1], False)
    for table, kind in ((sc.stage_cases(), "stage"), (sc.gpf_cases(), "gpf"), (sc.mixed_cases(), "mixed")):
        for c in table:
            out["static/%s/%s" % (kind, c[0])] = (c[-1], True)
    return out


def golden():
    """{case id: line} of the committed table.  The file keeps each distinct kernel name, sequence
    part (flags ... img_solo) and shape part (the rest) once; a case is the three indices."""
    with open(GOLDEN) as f:
        g = json.load(f)
    return {cid: "%s | %s %s" % (g["names"][n], g["sequence"][s], g["shape"][h]) for cid, (n, s, h) in g["cases"].items()}


def parse(line):
    """(kernel name, {key: int}) of a describe line."""
    name, _, rest = line.partition(" | ")
    return name, {k: int(v, 0) for k, v in (kv.split("=") for kv in rest.split())}


@contextlib.contextmanager
def environment(env):
    """The process environment with exactly env's PBGPU_* variables, for the block."""
    saved = {k: v for k, v in os.environ.items() if k.startswith("PBGPU_")}
    for k in saved:
        del os.environ[k]
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            del os.environ[k]
        os.environ.update(saved)


def describe(cfg, env, rule=0, fold=0):
    """pbgpu_plan_describe's line for a config loaded under env (PbError where the load is refused)."""
    with environment(env):
        return pbgpu.plan_describe(SLOT, pbgpu.Sequence.from_config(cfg), pc.SEED_BASE, rule, fold)
