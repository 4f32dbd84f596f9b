"""Case tables of tests/test_gpu_fields.py: the per-frame header fields (TTL, IPv4 ID, source
range index, source host bits, port; sequence.c:443-527) on every build kernel.  Every kernel's
prologue draws them from one r0 = rand_r(seed) with pb_mod (csrc/pb_device.h) on constants of
make_div (csrc/pb_plan.cpp), loads the range its own way and places the header itself.

No GPU code here: hosts (the smallest sequence shapes that reach each pb_kern, with the kernel
name they must run on), field variants, range tables, and the iterations at which a divisor's
residue is 0 or d - 1 or r0 is the largest, found with a numpy restatement of seed() and rand_r().
tests/test_field_cases_cpu.py holds the tables against the planner, pyspec and the oracle."""
import collections
import copy
import functools

import numpy as np

import pb_configs as pc
import pyspec
import static_cases as sc

SLOT = 5
FIRST_ITER = 987654321
N_ITER = 4099       # several workgroups of every kernel and a partial last one (pb_vline_kernel: 17 of 252 frames)
N_ITER_LONG = 1031  # the 1500-B and 9043-B hosts: no case stores more than about 10 MB
WINDOW = 513        # iterations of a targeted window
SEARCH = 1 << 22    # targets() looks at iterations 1..SEARCH

Host = collections.namedtuple("Host", "id proto cfg env rule kernel n_iter small")


# ------------------------------------------------------------------ hosts
def _payload(proto, lo, hi=None, static=False):
    """`proto` frames with one payload: random of lo..hi bytes, or the static ramp of lo bytes."""
    cfg = pc.get(sc.BASE[proto])
    if static:
        cfg["payloads"] = [{"exact": sc.hex_text(sc.pattern("ramp", lo))}]
    else:
        cfg["payloads"] = [{"length": {"min": lo, "max": lo if hi is None else hi}}]
    return cfg


def _frame(proto, flen, static=False):
    return _payload(proto, flen - sc.HL[proto], static=static)


def _hosts():
    out = []

    def add(hid, proto, cfg, kernel, env=None, rule=0, n_iter=N_ITER, small=False):
        out.append(Host(hid, proto, cfg, dict(env or {}), rule, kernel, n_iter, small))

    # one lane per frame and its page forms (frames of at most 128 B: `small`, also run through pyspec)
    add("xsmall_udp64", "udp", _frame("udp", 64), "pb_xsmall_kernel<16, 17, true,", small=True)
    add("xsmall_udp128", "udp", _frame("udp", 128), "pb_xsmall_kernel<32, 17, true,", small=True)
    add("xpage256_tcp60", "tcp", _frame("tcp", 60), "pb_xpage_kernel<16, 6, true, 256,", {"PBGPU_XP_WGT": "256"}, small=True)
    add("xpage512_tcp60", "tcp", _frame("tcp", 60), "pb_xpage_kernel<16, 6, true, 512,", {"PBGPU_XP_WGT": "512"}, small=True)
    add("xpage_icmp98_static", "icmp", _frame("icmp", 98, True), "pb_xpage_kernel<32, 1, false, 512, false>", small=True)
    add("ximg_icmp66_static", "icmp", _frame("icmp", 66, True), "pb_ximg_kernel<", {"PBGPU_XP_IMG": "2"}, small=True)
    add("ximg_icmp98_static", "icmp", _frame("icmp", 98, True), "pb_ximg_kernel<", {"PBGPU_XP_IMG": "2"}, small=True)
    add("small_udp65", "udp", _frame("udp", 65), "pb_small_kernel<32, 17, true,", small=True)
    # (an even static length of 52-128 B takes pb_xpage_kernel: the static pb_small_kernel host is odd)
    add("small_udp107_static", "udp", _frame("udp", 107, True), "pb_small_kernel<32, 17, false,", small=True)
    # fixed lengths over 128 B, multiples of 4, random payload
    add("fstage_udp132", "udp", _frame("udp", 132), "pb_fstage_kernel<")
    add("fstage_udp1500", "udp", _frame("udp", 1500), "pb_fstage_kernel<", n_iter=N_ITER_LONG)
    add("fstage_tcp1500", "tcp", _frame("tcp", 1500), "pb_fstage_kernel<", n_iter=N_ITER_LONG)
    # packed variable lengths, payloads of at least 32 B
    add("vline_udp", "udp", _payload("udp", 32, 96), "pb_vline_kernel<42,")
    add("vline_tcp", "tcp", _payload("tcp", 32, 96), "pb_vline_kernel<54,")
    add("vline_icmp", "icmp", _payload("icmp", 32, 96), "pb_vline_kernel<42,")
    add("vpage_udp", "udp", _payload("udp", 32, 96), "pb_vpage_kernel<42,", {"PBGPU_KERNEL": "vpage"})
    # the LDS stage with every payload random: short packed frames, and a fixed odd jumbo length
    add("vstage_udp_0_33", "udp", _payload("udp", 0, 33), "pb_vstage_kernel<", small=True)
    add("vstage_udp9043", "udp", _frame("udp", 9043), "pb_vstage_kernel<", n_iter=N_ITER_LONG)
    # the LDS stage with static payloads: one static payload, and udp_multi_payload's mixed list
    add("stage_udp142_static", "udp", _frame("udp", 142, True), "pb_stage_kernel<8, 0>")
    add("stage_udp_mixed", "udp", pc.get("udp_multi_payload"), "pb_stage_kernel<8, 2>")
    add("stage_udp_mixed_literal", "udp", pc.get("udp_multi_payload"), "pb_stage_kernel<8, 2>", rule=1)
    # a group of lanes per frame
    add("gpf_udp242_static", "udp", _frame("udp", 242, True), "pb_gpf_kernel<8, 0>", {"PBGPU_KERNEL": "gpf"})
    add("gpf_udp242", "udp", _frame("udp", 242), "pb_gpf_kernel<8, 1>", {"PBGPU_KERNEL": "gpf"})
    assert len({h.id for h in out}) == len(out)
    return out


HOSTS = _hosts()
HOST = {h.id: h for h in HOSTS}
ALL_KERNELS = ("pb_small_kernel", "pb_xsmall_kernel", "pb_xpage_kernel", "pb_ximg_kernel", "pb_gpf_kernel",
               "pb_stage_kernel", "pb_vstage_kernel", "pb_fstage_kernel", "pb_vline_kernel", "pb_vpage_kernel")
# the one-at-a-time variants' hosts; ICMP type / code 255 has no field there and takes two ICMP hosts
SINGLE_HOSTS = ("xsmall_udp64", "xpage512_tcp60", "vline_udp", "stage_udp_mixed")
ICMP_HOSTS = ("xpage_icmp98_static", "vline_icmp")
# hosts whose every variant also runs through tests/pyspec.py on the CPU
PYSPEC_HOSTS = tuple(h.id for h in HOSTS if h.small) + ("vline_udp",)


# ------------------------------------------------------------------ range tables
FAIL_RANGES = ["bogus", "10.0.0.0", "192.168.7.0/33", "10.1.2.0/-1", None]  # the fail path: 127.0.0.1


def _net(i):
    """Range i of a family with pairwise different first octets and prefixes of 8..32 bits, so no
    two ranges share their network bits; the address carries host bits the mask must clear."""
    return "%d.%d.%d.%d/%d" % (11 + i, (37 * i + 5) % 256, (91 * i + 17) % 256, (53 * i + 201) % 256, 8 + (5 * i) % 25)


def _table64():
    """PB_MAX_RANGES entries: every prefix length /0../32, even ones on 255.255.255.255 and odd ones
    on 0.0.0.0 (what the frame carries of the address is the mask's doing alone), the five fail-path
    entries and 26 ranges of _net(), a range of _net() first and last."""
    mid = ["%s/%d" % ("255.255.255.255" if c % 2 == 0 else "0.0.0.0", c) for c in range(33)]
    mid += FAIL_RANGES + [_net(i) for i in range(1, 25)]
    assert len(mid) == 62
    return [_net(0)] + [mid[(37 * i) % 62] for i in range(62)] + [_net(25)]


RANGES64 = _table64()
RANGE_COUNTS = (1, 2, 3, 7, 8, 63, 64)


def range_table(n):
    """n source ranges: the 64-entry table (or its first 63), else the first n of _net()."""
    if n >= 63:
        return list(RANGES64[:n])
    return [_net(i) for i in range(n)]


# strtok_r / inet_aton / atoi on a range's text (PB-Common rand_ip as the oracle restates it)
RANGE_TOKENS = ["/8/24", "10.1/16", "0x0a.1.2.3/8", "10.0.0.0/8/3", "10.0.0.0/ 8", "10.0.0.0/abc", "10.0.0.0/+8",
                "0.0.0.0/0", "10.9.8.7/32", "bogus", "10.0.0.0", "192.168.7.0/33", "172.16.5.4/20", "10.1.2.0/-1",
                "/", "", "//", "10.0.0.0/", "10.0.0.0//8", "///10.0.0.0///8", "10.0.0.0/8 ", "10.0.0.0/08",
                "10.0.0.0/0x10", " 10.0.0.0/8", "10.0.0.0 /8", "10.0.0.0/32x", "10.0.0.0/-", "10.0.0.0/-0",
                "10.0.0.0/\t\n 12", "010.0.0.1/9", "1.2.3/24", "16909060/31", "1.2.3.4.5/8", "256.0.0.1/8",
                "10.0.0.0/4294967304", "10.0.0.0/2147483648"]


# ------------------------------------------------------------------ variants
def variant(host, ttl=None, ident=None, ranges=None, sip=None, no_source=False, sport=None, dport=None, tos=None,
            flags=False, icmp=None, ipcsum=None, l4csum=None):
    """The host's config with the given header fields; what is None stays as the host has it.
    ttl, ident: (min, max); ranges: a count (range_table) or a list; ports: 0 = random."""
    cfg = copy.deepcopy(host.cfg)
    ip = cfg["ip"]
    if ttl is not None:
        ip["ttl"] = {"min": ttl[0], "max": ttl[1]}
    if ident is not None:
        ip["id"] = {"min": ident[0], "max": ident[1]}
    if ranges is not None:
        ip["ranges"] = range_table(ranges) if isinstance(ranges, int) else list(ranges)
    if sip is not None or no_source:
        ip.pop("ranges", None)
    if sip is not None:
        ip["sip"] = sip
    if tos is not None:
        ip["tos"] = tos
    if ipcsum is not None:
        ip["csum"] = ipcsum
    if l4csum is not None:
        cfg["l4csum"] = l4csum
    if host.proto in ("udp", "tcp"):  # (ICMP has no ports)
        ports = cfg.setdefault(host.proto, {})
        if sport is not None:
            ports["sport"] = sport
        if dport is not None:
            ports["dport"] = dport
    if flags and host.proto == "tcp":
        cfg["tcp"].update({f: 1 for f in ("syn", "ack", "psh", "fin", "rst", "urg", "ece", "cwr")})
    if icmp is not None and host.proto == "icmp":
        cfg["icmp"] = {"type": icmp[0], "code": icmp[1]}
    return cfg


# name -> (variant()'s arguments, IPv4 fold rule); every host runs these
WIDE = dict(ttl=(0, 255), ident=(0, 65535), ranges=64, sport=0, dport=0)
COMBOS = {
    "wide": (WIDE, 0),
    "narrow": (dict(ttl=(0, 1), ident=(65534, 65535), ranges=2, sport=0, dport=53), 0),
    "odd": (dict(ttl=(1, 3), ident=(1, 65535), ranges=7), 0),         # divisors 3 and 65,535
    "defaults": (dict(ident=(0, 64000), ranges=1), 0),                # one range: the hoisted rg1
    "none": (dict(sip="10.0.0.1", ttl=(200, 200), ident=(0x1234, 0x1234), sport=1234, dport=65535), 0),  # K.ranges null
    "localhost": (dict(no_source=True), 0),
    "no_csums": (dict(ipcsum=0, l4csum=0), 0),
    "single_fold": (WIDE, 1),
}
TARGETED = ("wide", "odd", "defaults")

TTL_PAIRS = [(0, 255), (0, 1), (254, 255), (1, 3), (10, 200)]
ID_PAIRS = [(0, 65535), (0, 1), (65534, 65535), (1, 65535), (0, 64000), (100, 9000)]


def _singles():
    s = {}
    for lo, hi in TTL_PAIRS:
        s["ttl_%d_%d" % (lo, hi)] = dict(ttl=(lo, hi))
    for lo, hi in ID_PAIRS:
        s["id_%d_%d" % (lo, hi)] = dict(ident=(lo, hi))
    for n in RANGE_COUNTS:
        s["ranges_%d" % n] = dict(ranges=n)
    for sp in (65535, 0):
        for dp in (65535, 0):
            s["sport_%s_dport_%s" % ("rnd" if not sp else "fixed", "rnd" if not dp else "fixed")] = dict(sport=sp, dport=dp)
    s["tos_ff"] = dict(tos=0xFF)
    s["tcp_all_flags"] = dict(flags=True)
    s["icmp_255_255"] = dict(icmp=(255, 255))
    s["sip_refused"] = dict(sip="300.1.2.3")  # inet_aton refuses it: 0.0.0.0
    for ipc in (1, 0):
        for l4c in (1, 0):
            s["ipcsum%d_l4csum%d" % (ipc, l4c)] = dict(ipcsum=ipc, l4csum=l4c)
    s["range_text"] = dict(ranges=RANGE_TOKENS)
    return s


SINGLES = _singles()


def single_hosts(name):
    if name == "tcp_all_flags":
        return tuple(h for h in SINGLE_HOSTS if HOST[h].proto == "tcp")
    if name == "icmp_255_255":
        return ICMP_HOSTS
    return SINGLE_HOSTS


def combo_cases():
    """[(host id, variant name)] of the combination variants."""
    return [(h.id, v) for h in HOSTS for v in COMBOS]


def single_cases():
    return [(h, v) for v in SINGLES for h in single_hosts(v)]


def case_cfg(hid, name):
    """(config, fold rule) of a case of either table."""
    args, fold = COMBOS[name] if name in COMBOS else (SINGLES[name], 0)
    return variant(HOST[hid], **args), fold


def verify_checks(cfg):
    """The pbgpu_verify checks a config's frames can pass: tot_len, and each checksum it computes."""
    return 2 | (1 if cfg["ip"].get("csum", 1) else 0) | (4 if cfg.get("l4csum", 1) else 0)


# ------------------------------------------------------------------ targeted iterations
def np_seed(seed_base, seq_idx, k):
    """pyspec.seed on a uint64 array of iterations."""
    k = np.asarray(k, dtype=np.uint64)
    x = np.uint64(seed_base) ^ (np.uint64((seq_idx << 48) & (2 ** 64 - 1)) + k)
    z = x + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return ((z ^ (z >> np.uint64(31))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def np_rand_r(s):
    """pyspec.rand_r on a uint32 array of seeds: (values, seeds after)."""
    a, c = np.uint32(pyspec.A), np.uint32(pyspec.Cc)
    s = np.asarray(s, dtype=np.uint32) * a + c
    r = (s >> np.uint32(16)) & np.uint32(0x7FF)
    s = s * a + c
    r = (r << np.uint32(10)) ^ ((s >> np.uint32(16)) & np.uint32(0x3FF))
    s = s * a + c
    r = (r << np.uint32(10)) ^ ((s >> np.uint32(16)) & np.uint32(0x3FF))
    return r, s


@functools.lru_cache(maxsize=4)
def first_draws(seed_base, seq_idx):
    """r0 of iterations 0..SEARCH (index = iteration)."""
    with np.errstate(over="ignore"):
        r0 = np_rand_r(np_seed(seed_base, seq_idx, np.arange(SEARCH + 1, dtype=np.uint64)))[0]
    r0.setflags(write=False)
    return r0


Targets = collections.namedtuple("Targets", "zero last largest")


@functools.lru_cache(maxsize=None)
def targets(seed_base, seq_idx, d):
    """Among iterations 1..SEARCH: the first k with r0 % d == 0, the first with r0 % d == d - 1, and
    the k with the largest r0 (None where there is none)."""
    r0 = first_draws(seed_base, seq_idx)[1:]
    res = r0 % np.uint32(d)

    def first(v):
        hit = np.nonzero(res == np.uint32(v))[0]
        return int(hit[0]) + 1 if len(hit) else None

    return Targets(first(0), first(d - 1), int(np.argmax(r0)) + 1)


def draw(seed_base, seq_idx, k):
    return int(first_draws(seed_base, seq_idx)[k])


def window_first(k):
    """A targeted window's first iteration: 100 before the target, odd, at least 1."""
    return max(1, k - 100) | 1


PORT_D = 65535


def field_divisors(cfg):
    """(TTL, ID, range count) divisors of a config (1: the field is fixed)."""
    ip = cfg["ip"]
    ttl, idd = ip.get("ttl", {}), ip.get("id", {})
    nr = 0 if ip.get("sip") is not None else len(ip.get("ranges", []))
    return (ttl.get("max", 64) - ttl.get("min", 64) + 1, idd.get("max", 64000) - idd.get("min", 0) + 1, max(1, nr))


def all_divisors():
    """Every divisor the case tables draw a header field with."""
    ds = {PORT_D}
    for hid, name in combo_cases() + single_cases():
        ds.update(field_divisors(case_cfg(hid, name)[0]))
    return sorted(ds)


def target_cases(seed_base=pc.SEED_BASE):
    """[(host id, variant, target id, iteration, expectation)] of the targeted windows: both residues
    of the port, ID and range-count divisors and the largest r0.  The expectation is (field, value)
    with field among "port", "id", "range" (value: the range's index) and "draw" (value: r0)."""
    out = []
    for h in HOSTS:
        for name in TARGETED:
            cfg, _ = case_cfg(h.id, name)
            _, id_d, rng_d = field_divisors(cfg)
            id_min = cfg["ip"]["id"]["min"]
            tp, ti, tr = (targets(seed_base, SLOT, d) for d in (PORT_D, id_d, rng_d))
            if h.proto != "icmp":
                out.append((h.id, name, "port_1", tp.zero, ("port", 1)))
                out.append((h.id, name, "port_65535", tp.last, ("port", 65535)))
            out.append((h.id, name, "id_min", ti.zero, ("id", id_min)))
            out.append((h.id, name, "id_max", ti.last, ("id", id_min + id_d - 1)))
            out.append((h.id, name, "range_first", tr.zero, ("range", 0)))
            out.append((h.id, name, "range_last", tr.last, ("range", rng_d - 1)))
            out.append((h.id, name, "largest_r0", tp.largest, ("draw", draw(seed_base, SLOT, tp.largest))))
    return out


def expected_saddr(cfg, idx, r0):
    """The source address range idx of cfg gives at draw r0 (pyspec's rule)."""
    rg = pyspec.parse_range(cfg["ip"]["ranges"][idx])
    return 0x7F000001 if rg is None else rg[0] | (r0 & rg[1])


def frame_field(cfg, frame, field, value, r0):
    """Whether a target's frame (its bytes, built at draw r0) carries the target's field."""
    frame = bytes(frame)
    ident = int.from_bytes(frame[18:20], "big")
    if field == "id":
        return ident == value
    if field == "range":
        return int.from_bytes(frame[26:30], "big") == expected_saddr(cfg, value, r0)
    if field == "draw":
        _, id_d, _ = field_divisors(cfg)
        return r0 == value and ident == cfg["ip"]["id"]["min"] + r0 % id_d
    ports = cfg["tcp" if cfg["ip"]["protocol"] == "tcp" else "udp"]
    got = [int.from_bytes(frame[at:at + 2], "big") for at, key in ((34, "sport"), (36, "dport")) if not ports.get(key, 0)]
    return bool(got) and all(p == value for p in got)
