"""Static payloads (hex, string, file, static-random; sequence.c:264-361) through every build
kernel, bit-exact against the CPU oracle, which tests/test_static_payload_cpu.py holds against
pyspec and host libc.  The small kernels take a static payload from K.stail[], pb_stage_kernel and
pb_gpf_kernel gather it from the device blob at every byte alignment, and its part of the L4 sum
is folded on the host: code of its own next to the random payloads' that the other files run.

Every case asserts the kernel it ran on (tables and expected names: tests/static_cases.py), so
none can pass on another kernel than the one it names.  Run on the MI355X box: pytest -m gpu."""
import copy

import numpy as np
import pytest

import oracle_binding as ob
import pb_configs as pc
import static_cases as sc
from pbgpu import GpuContext, PbError, Sequence

pytestmark = pytest.mark.gpu

SLOT = 5
EINVAL = -22


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def _build(ctx, seq, first, n, rule=0):
    ctx.load_sequence(SLOT, seq, pc.SEED_BASE, payload_rule=rule)
    fb = ctx.alloc_frames(*ctx.build_size(SLOT, n))
    ctx.build(SLOT, first, n, fb)
    ctx.sync()
    data, off = fb.packed(), fb.offsets()
    fb.free()
    return data, off, ctx.kernel_name(SLOT)


def _check(ctx, cfg, first, n, rule=0):
    """As test_gpu_kernels._check: `n` iterations from an odd `first`, offsets and every byte
    against the oracle; returns the kernel's name and the bytes."""
    seq = Sequence.from_config(cfg)
    g_data, g_off, kern = _build(ctx, seq, first, n, rule)
    o_data, o_off = ob.build(seq, SLOT, first, n, pc.SEED_BASE, payload_rule=rule)
    assert np.array_equal(g_off, o_off), kern
    if not np.array_equal(g_data, o_data):
        bad = int(np.nonzero(g_data != o_data)[0][0])
        f = int(np.searchsorted(o_off, bad, side="right") - 1)
        pytest.fail(f"{kern}: first mismatch at byte {bad} (frame {f}, offset {bad - int(o_off[f])}): "
                    f"{int(g_data[bad]):#04x}, oracle {int(o_data[bad]):#04x}")
    return kern, g_data


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------ a. small frames
SMALL = sc.small_cases()


@pytest.mark.parametrize("cid,proto,flen,form,pats,want", SMALL, ids=[c[0] for c in SMALL])
def test_small_static_frames(ctx, monkeypatch, cid, proto, flen, form, pats, want):
    """UDP and TCP frames of hl + 1 .. 128 B with a static payload on pb_xsmall_kernel,
    pb_xpage_kernel (256 and 512 threads) and pb_small_kernel (64 and 128 frames per workgroup)."""
    _setenv(monkeypatch, sc.SMALL_FORMS[form])
    for pat in pats:
        cfg = sc.static_cfg(proto, sc.pattern(pat, flen - sc.HL[proto]))
        for n in sc.XS_COUNTS:
            n = max(1, n * 64 // flen)
            kern, _ = _check(ctx, cfg, 1000003 + 2 * n, n)
            assert kern.startswith(want), (pat, n, kern)


# ------------------------------------------------------------------ b. pb_stage_kernel<G, 0>
STAGE = sc.stage_cases()


@pytest.mark.parametrize("cid,proto,csum,flen,env,pats,want", STAGE, ids=[c[0] for c in STAGE])
def test_stage_static_frames(ctx, monkeypatch, cid, proto, csum, flen, env, pats, want):
    """One static payload, fixed length: frames that start and end at every byte of a 16-B chunk,
    across the group sizes and window sizes, up to the longest frame the LDS stage holds."""
    _setenv(monkeypatch, env)
    for pat in pats:
        cfg = sc.static_cfg(proto, sc.pattern(pat, flen - sc.HL[proto]), csum)
        for n in sc.counts_for(flen):
            kern, _ = _check(ctx, cfg, 3 + 2 * n, n)
            assert kern == want, (pat, n, kern)


# ------------------------------------------------------------------ c. pb_gpf_kernel<G, 0>
GPF = sc.gpf_cases()


@pytest.mark.parametrize("cid,proto,plen,env,pats,counts,want", GPF, ids=[c[0] for c in GPF])
def test_gpf_static_frames(ctx, monkeypatch, cid, proto, plen, env, pats, counts, want):
    """Frames too long for an LDS stage, up to PB_MAX_PCKT_LEN, and the group-per-frame kernel
    forced at 242 and 1501 B with 8 and 64 lanes per frame."""
    _setenv(monkeypatch, env)
    for pat in pats:
        cfg = sc.static_cfg(proto, sc.pattern(pat, plen))
        for n in counts:
            kern, _ = _check(ctx, cfg, 9 + 2 * n, n)
            assert kern == want, (pat, n, kern)


@pytest.mark.parametrize("proto", ["udp", "tcp", "icmp"])
@pytest.mark.parametrize("form", ["hex", "string"])
def test_one_byte_past_the_longest_payload_is_refused(ctx, proto, form):
    """pbgpu_load_sequence: -EINVAL for a static payload that would pass PB_MAX_PCKT_LEN; the
    longest one loads."""
    n = 65535 - sc.HL[proto]

    def cfg(k):
        c = sc.static_cfg(proto, b"")
        c["payloads"] = [{"exact": "41 " * k} if form == "hex" else {"exact": "A" * k, "isstring": 1}]
        return c

    with pytest.raises(PbError) as e:
        ctx.load_sequence(SLOT, Sequence.from_config(cfg(n + 1)), pc.SEED_BASE)
    assert e.value.code == EINVAL
    ctx.load_sequence(SLOT, Sequence.from_config(cfg(n)), pc.SEED_BASE)
    assert ctx.kernel_name(SLOT).startswith("pb_gpf_kernel<")


# ------------------------------------------------------------------ d. RMODE 2, long
MIXED = sc.mixed_cases()


@pytest.mark.parametrize("cid,proto,which,env,rule,counts,want", MIXED, ids=[c[0] for c in MIXED])
def test_mixed_long_payloads(ctx, monkeypatch, cid, proto, which, env, rule, counts, want):
    """Several payloads per iteration, static ones of up to 60 KB among random ones, under both
    payload rules (the static-random draw depends on the rule, quirk B8)."""
    _setenv(monkeypatch, env)
    cfg = sc.mixed_cfg(proto, which)
    for n in counts:
        kern, _ = _check(ctx, cfg, 31 + 2 * n, n, rule)
        assert kern == want, (n, kern)


# ------------------------------------------------------------------ e. sources
@pytest.mark.parametrize("proto", ["udp", "tcp"])
def test_file_sources_build_the_inline_frames(ctx, tmp_path, proto):
    """isfile through Sequence.from_config: a hex file with line breaks and a string file of the
    same 1400 bytes build the frames of the inline hex text; a missing file header-only frames."""
    data = bytes(b or 0x55 for b in sc.pattern("ramp", 1400))  # a string holds no NUL
    toks = ["%02X" % b for b in data]
    hexf, strf = tmp_path / "payload.hex", tmp_path / "payload.bin"
    # a space after each break: the break ends a token, where sscanf ignores it
    hexf.write_text("".join(" ".join(toks[i:i + 16]) + ("\n " if i % 32 else "\r\n ") for i in range(0, 1400, 16)))
    strf.write_bytes(data)
    want = sc.static_cfg(proto, data)
    first, n = 77, 300
    ref_kern, ref = _check(ctx, want, first, n)
    assert ref_kern == "pb_stage_kernel<16, 0>"
    assert ref[sc.HL[proto]:sc.HL[proto] + 1400].tobytes() == data
    for pl in ({"exact": str(hexf), "isfile": 1}, {"exact": str(strf), "isfile": 1, "isstring": 1}):
        cfg = copy.deepcopy(want)
        cfg["payloads"] = [pl]
        kern, got = _check(ctx, cfg, first, n)
        assert kern == ref_kern
        assert np.array_equal(got, ref)
    cfg = copy.deepcopy(want)
    cfg["payloads"] = [{"exact": str(tmp_path / "no_such_file"), "isfile": 1}]
    kern, got = _check(ctx, cfg, first, n)
    assert len(got) == n * sc.HL[proto]
    assert kern.startswith("pb_xpage_kernel" if proto == "tcp" else "pb_small_kernel<"), kern


# ------------------------------------------------------------------ f. sharding
@pytest.mark.parametrize("proto", ["udp", "tcp"])
def test_shards_build_the_whole(ctx, proto):
    """[k, k + 100) in one build and as [k, k + 37) + [k + 37, k + 100): the same bytes.  The
    static payload takes no part in the seed stream; the random header fields still vary."""
    cfg = sc.static_cfg(proto, sc.pattern("ramp", 1501 - sc.HL[proto]))
    k = 123457
    kern, whole = _check(ctx, cfg, k, 100)
    assert kern == "pb_stage_kernel<16, 0>"
    kern_a, a = _check(ctx, cfg, k, 37)
    kern_b, b = _check(ctx, cfg, k + 37, 63)
    assert kern_a == kern_b == kern
    assert np.array_equal(np.concatenate([a, b]), whole)
    frames = whole.reshape(100, 1501)
    assert (frames[:, sc.HL[proto]:] == frames[0, sc.HL[proto]:]).all()
    assert len({f[26:30].tobytes() for f in frames}) > 90  # source addresses drawn per iteration
