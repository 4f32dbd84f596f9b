"""The header-field tables of tests/field_cases.py, CPU only.

1. Every host's kernel name, for every variant it runs, from the planner (pbgpu_plan_describe);
   the hosts cover every pb_kern.
2. The numpy seed() / rand_r() against pyspec's scalar ones; every targeted iteration is found.
3. The C oracle (lean and faithful) against tests/pyspec.py, frame for frame, for every variant on
   the hosts pyspec can afford, under both IPv4 fold rules, at the GPU file's first iteration and
   at the targeted ones.
4. A source range's text: pyspec.parse_range against host libc's strtok_r / inet_aton / atoi, the
   calls the oracle and the library make, and the oracle against pyspec on each token.
5. make_div's constants for every divisor a header field can have: n - ((n * m) >> sh) * d == n % d
   at the edges of n < 2^31, the range of rand_r."""
import ctypes
import ctypes.util
import socket
import struct

import numpy as np
import pytest

import field_cases as fc
import oracle_binding as ob
import pb_configs as pc
import pbgpu
import plan_cases as plc
import pyspec
from pbgpu import Sequence

N_ITER = 200


# ------------------------------------------------------------------ 1. hosts
def test_hosts_cover_every_kernel():
    names = set()
    for h in fc.HOSTS:
        name = plc.parse(plc.describe(h.cfg, h.env, h.rule, 0))[0]
        assert name.startswith(h.kernel), (h.id, name)
        names.add(name.split("<")[0])
    assert names == set(fc.ALL_KERNELS)
    assert set(fc.SINGLE_HOSTS) | set(fc.ICMP_HOSTS) | set(fc.PYSPEC_HOSTS) <= set(fc.HOST)


def test_every_case_keeps_its_hosts_kernel():
    cases = fc.combo_cases() + fc.single_cases()
    assert len(cases) == len(set(cases)) == len(fc.HOSTS) * len(fc.COMBOS) + sum(
        len(fc.single_hosts(v)) for v in fc.SINGLES)
    for hid, name in cases:
        h = fc.HOST[hid]
        cfg, fold = fc.case_cfg(hid, name)
        got = plc.parse(plc.describe(cfg, h.env, h.rule, fold))[0]
        assert got.startswith(h.kernel), (hid, name, got)


def test_range_tables():
    """The 64-entry table holds every prefix length on both addresses' halves and the five fail-path
    entries; the other tables' ranges differ pairwise in their network bits."""
    t = fc.RANGES64
    assert len(t) == pbgpu.MAX_RANGES == 64
    assert {"255.255.255.255/%d" % c for c in range(0, 33, 2)} | {"0.0.0.0/%d" % c for c in range(1, 33, 2)} <= set(t)
    assert all(r in t for r in fc.FAIL_RANGES) and all(pyspec.parse_range(r) is None for r in fc.FAIL_RANGES)
    assert pyspec.parse_range(t[0]) is not None and pyspec.parse_range(t[-1]) is not None
    nets = [pyspec.parse_range(fc._net(i)) for i in range(26)]
    for i, (na, ha) in enumerate(nets):
        assert na & ha == 0 and na != 0
        for nb, hb in nets[:i]:
            both = ~(ha | hb) & 0xFFFFFFFF  # bits that are network bits of both
            assert (na ^ nb) & both
    assert [len(fc.range_table(n)) for n in fc.RANGE_COUNTS] == list(fc.RANGE_COUNTS)
    assert fc.range_table(63) == t[:63]


# ------------------------------------------------------------------ 2. the draws
def test_numpy_draws_equal_pyspec():
    ks = np.concatenate([np.arange(0, 3000), np.arange(fc.FIRST_ITER, fc.FIRST_ITER + 1000),
                         np.array([2 ** 32 - 1, 2 ** 32, 2 ** 40 + 7, 2 ** 48 - 1])]).astype(np.uint64)
    for seq_idx in (0, fc.SLOT, 255):
        s = fc.np_seed(pc.SEED_BASE, seq_idx, ks)
        r, s2 = fc.np_rand_r(s)
        for i, k in enumerate(ks.tolist()):
            want = pyspec.seed(pc.SEED_BASE, seq_idx, k)
            assert int(s[i]) == want, (seq_idx, k)
            assert (int(r[i]), int(s2[i])) == pyspec.rand_r(want), (seq_idx, k)
    r0 = fc.first_draws(pc.SEED_BASE, fc.SLOT)
    for k in (0, 1, 4099, fc.SEARCH):
        assert int(r0[k]) == pyspec.rand_r(pyspec.seed(pc.SEED_BASE, fc.SLOT, k))[0]


def test_every_target_is_found():
    r0 = fc.first_draws(pc.SEED_BASE, fc.SLOT)
    ds = fc.all_divisors()
    assert {2, 3, 7, 8, 63, 64, 191, 256, 8901, 64001, 65535, 65536} <= set(ds)
    for d in ds:
        t = fc.targets(pc.SEED_BASE, fc.SLOT, d)
        assert t.zero is not None and t.last is not None, d
        assert 1 <= t.zero <= fc.SEARCH and 1 <= t.last <= fc.SEARCH
        assert int(r0[t.zero]) % d == 0 and int(r0[t.last]) % d == d - 1, d
        assert not np.any(r0[1:t.zero] % np.uint32(d) == 0) and not np.any(r0[1:t.last] % np.uint32(d) == d - 1)
        assert int(r0[t.largest]) == int(r0[1:].max())
    t = fc.targets(pc.SEED_BASE, fc.SLOT, 65535)
    assert int(r0[t.largest]) > 2 ** 31 - 1024  # close to rand_r's largest value
    cases = fc.target_cases()
    assert all(c[3] is not None for c in cases)
    assert len(cases) == sum(7 if h.proto != "icmp" else 5 for h in fc.HOSTS) * len(fc.TARGETED)


# ------------------------------------------------------------------ 3. oracle == pyspec
def _same(cfg, rule, first, n):
    seq = Sequence.from_config(cfg)
    for fold in (0, 1):
        want = pyspec.build(cfg, fc.SLOT, first, n, pc.SEED_BASE, literal=bool(rule), single_fold=bool(fold))
        for faithful in (False, True):
            got = ob.frames(seq, fc.SLOT, first, n, pc.SEED_BASE, payload_rule=rule, iph_fold=fold, faithful=faithful)
            assert len(got) == len(want)
            for i, (g, w) in enumerate(zip(got, want)):
                assert g == w, "iteration %d + frame %d (fold %d, faithful %s)" % (first, i, fold, faithful)
    return want


PYSPEC_CASES = [c for c in fc.combo_cases() + fc.single_cases() if c[0] in fc.PYSPEC_HOSTS + fc.SINGLE_HOSTS]


@pytest.mark.parametrize("hid,name", PYSPEC_CASES, ids=["%s-%s" % c for c in PYSPEC_CASES])
def test_oracle_equals_pyspec(hid, name):
    h = fc.HOST[hid]
    cfg, _ = fc.case_cfg(hid, name)
    _same(cfg, h.rule, fc.FIRST_ITER, N_ITER)
    ks = set()
    for d in fc.field_divisors(cfg) + (fc.PORT_D,):
        ks.update(fc.targets(pc.SEED_BASE, fc.SLOT, d))
    for k in sorted(ks):
        _same(cfg, h.rule, k, 1)


def test_target_frames_carry_their_fields():
    """What tests/test_gpu_fields.py asserts of each targeted window's frame, on pyspec's frames."""
    seen = set()
    for hid, name, tid, k, (field, value) in fc.target_cases():
        if hid not in ("xsmall_udp64", "xpage_icmp98_static") or (hid, name, k, field) in seen:
            continue
        seen.add((hid, name, k, field))
        cfg, _ = fc.case_cfg(hid, name)
        frame = pyspec.build(cfg, fc.SLOT, k, 1, pc.SEED_BASE)[0]
        assert fc.frame_field(cfg, frame, field, value, fc.draw(pc.SEED_BASE, fc.SLOT, k)), (hid, name, tid)


# ------------------------------------------------------------------ 4. range text
@pytest.fixture(scope="module")
def libc():
    lib = ctypes.CDLL(ctypes.util.find_library("c"))
    lib.strtok_r.restype = ctypes.c_void_p
    lib.strtok_r.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
    lib.inet_aton.restype = ctypes.c_int
    lib.inet_aton.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    lib.atoi.restype = ctypes.c_int
    lib.atoi.argtypes = [ctypes.c_void_p]
    return lib


def _libc_range(libc, text):
    """(net, host mask) or None, by the calls of the oracle's parse_range on host libc."""
    buf = ctypes.create_string_buffer(text.encode())
    save = ctypes.c_void_p()
    ip = libc.strtok_r(ctypes.addressof(buf), b"/", ctypes.byref(save))
    cs = libc.strtok_r(None, b"/", ctypes.byref(save))
    addr = ctypes.c_uint32(0)
    if not ip or not cs or not libc.inet_aton(ip, ctypes.byref(addr)):
        return None
    cidr = libc.atoi(cs)
    if cidr < 0 or cidr > 32:
        return None
    hm = 0xFFFFFFFF if cidr == 0 else (1 << (32 - cidr)) - 1
    return socket.ntohl(addr.value) & ~hm & 0xFFFFFFFF, hm


# what the issue's tokens must give, stated by hand: (network, host mask)
BY_HAND = {
    "/8/24": (0x00000000, 0xFF),            # strtok_r skips the slash in front: ip "8" = 0.0.0.8, /24
    "10.1/16": (0x0A000000, 0xFFFF),        # inet_aton: "10.1" = 10.0.0.1
    "0x0a.1.2.3/8": (0x0A000000, 0xFFFFFF),
    "10.0.0.0/8/3": (0x0A000000, 0xFFFFFF),
    "10.0.0.0/ 8": (0x0A000000, 0xFFFFFF),  # atoi skips white space
    "10.0.0.0/abc": (0, 0xFFFFFFFF),        # atoi 0: the whole address random
    "10.0.0.0/+8": (0x0A000000, 0xFFFFFF),
    "10.0.0.0/-1": None,
    "bogus": None,
    "10.0.0.0": None,
    "192.168.7.0/33": None,
}


@pytest.mark.parametrize("tok", fc.RANGE_TOKENS, ids=[repr(t) for t in fc.RANGE_TOKENS])
def test_range_text_equals_libc(libc, tok):
    want = _libc_range(libc, tok)
    if tok in BY_HAND:
        assert want == BY_HAND[tok]
    assert pyspec.parse_range(tok) == want
    cfg = fc.variant(fc.HOST["xsmall_udp64"], ranges=[tok])
    frames = _same(cfg, 0, fc.FIRST_ITER, 32)
    r0 = [pyspec.rand_r(pyspec.seed(pc.SEED_BASE, fc.SLOT, fc.FIRST_ITER + i))[0] for i in range(32)]
    got = [struct.unpack("!I", f[26:30])[0] for f in frames]
    assert got == [0x7F000001 if want is None else want[0] | (r & want[1]) for r in r0]


def test_range_text_table_holds_the_issues_tokens():
    assert set(BY_HAND) - {"10.0.0.0/-1"} <= set(fc.RANGE_TOKENS)
    assert pyspec.parse_range(None) is None
    assert pyspec.atoi("4294967304") == 8 and pyspec.atoi("-") == 0 and pyspec.atoi(" \t-12x") == -12


# ------------------------------------------------------------------ 5. make_div
class PbDiv(ctypes.Structure):
    _fields_ = [("d", ctypes.c_uint32), ("m", ctypes.c_uint32), ("sh", ctypes.c_uint32)]


def test_make_div_constants():
    """pb_div make_div(uint32_t) (csrc/pb_plan.h), by the library's exported C++ symbol."""
    fn = getattr(pbgpu.load_library(), "_Z8make_divj")  # a missing symbol fails here
    fn.restype = PbDiv
    fn.argtypes = [ctypes.c_uint32]
    ds = np.arange(1, 65556 + 1, dtype=np.uint64)
    m = np.empty(len(ds), dtype=np.uint64)
    sh = np.empty(len(ds), dtype=np.uint64)
    for i, d in enumerate(ds.tolist()):
        v = fn(d)
        assert v.d == d
        m[i], sh[i] = v.m, v.sh
    top = np.uint64(2 ** 31 - 1)
    kd = top // ds * ds  # the largest multiple of d below 2^31
    assert np.all(kd < np.uint64(2 ** 31)) and np.all(kd + ds > top)
    assert np.all(m < np.uint64(2 ** 32)) and np.all(sh < np.uint64(64))
    for what, n in (("0", np.zeros_like(ds)), ("d-1", ds - 1), ("d", ds), ("kd-1", kd - 1), ("kd", kd),
                    ("2^31-1", np.full_like(ds, top))):
        assert np.all(n * m < np.uint64(2 ** 63))  # the product fits 64 bits
        got = n - ((n * m) >> sh) * ds
        bad = np.nonzero(got != n % ds)[0]
        assert not len(bad), "n = %s: d = %d gives %d" % (what, int(ds[bad[0]]), int(got[bad[0]]))
