"""Case tables of tests/test_gpu_static_payloads.py: static payloads (hex, string, file and
static-random, sequence.c:264-361) through every build kernel, each case with the kernel name it
must run on.  Kept apart from the GPU file so that tests/test_static_payload_cpu.py can check,
without a GPU, that the expected names cover every static form of every kernel."""
import copy

import pb_configs as pc

HL = {"udp": 42, "tcp": 54, "icmp": 42}
PROTO_NUM = {"udp": 17, "tcp": 6, "icmp": 1}
BASE = {"udp": "c2_udp_64", "tcp": "c4_tcp_syn", "icmp": "c5_icmp_echo"}  # random sources, ports, IDs
BUDGET = 6 << 20  # bytes per build, as test_gpu_kernels._iters


# ------------------------------------------------------------------ payload contents
def pattern(name, n):
    """Contents under which a wrong shift, byte order or carry shows: the ramp; all 0xFF (the
    folded sum is 0xFFFF); zeros; one 0x80 at an even / odd index near the middle of zeros."""
    if name == "ramp":
        return bytes((7 * i + 3) & 255 for i in range(n))
    if name == "ff":
        return b"\xff" * n
    if name == "zero":
        return bytes(n)
    b = bytearray(n)
    at = (n // 2 & ~1) + (name == "x80_odd")
    b[at if at < n else 0] = 0x80  # (a 1-B payload has no odd index)
    return bytes(b)


OTHER_PATTERNS = ("ff", "zero", "x80_even", "x80_odd")


def hex_text(data):
    return " ".join("%02x" % b for b in data)


def static_cfg(proto, data, l4csum=1):
    """`proto` frames with one static hex payload; the headers keep their random fields."""
    cfg = copy.deepcopy(pc.get(BASE[proto]))
    cfg["payloads"] = [{"exact": hex_text(data)}]
    cfg["l4csum"] = l4csum
    return cfg


# ------------------------------------------------------------------ a. small frames
XS_LENS = [42, 43, 44, 48, 52, 56, 60, 64, 72, 96, 98, 100, 106, 108, 116, 120, 124, 127, 128]  # test_gpu_kernels.XS_LENS
XS_COUNTS = [1, 5, 200, 2048, 2049, 2 * 2048 * 5 + 77]  # test_gpu_kernels.XS_COUNTS, scaled by 64 / length there
SMALL_FORMS = {
    "default": {},
    "xpage_forced_256": {"PBGPU_XP_FORCE": "1", "PBGPU_XP_WGT": "256"},
    "xpage_forced_512": {"PBGPU_XP_FORCE": "1", "PBGPU_XP_WGT": "512"},
    "linear_wg64": {"PBGPU_KERNEL": "linear", "PBGPU_SMALL_WGT": "64"},
    "linear_wg128": {"PBGPU_KERNEL": "linear", "PBGPU_SMALL_WGT": "128"},
}
SMALL_OTHER_LENS = (64, 98, 127, 128)


def small_kernel(proto, flen, form):
    """The rule test_small_frames_pages states for static payloads: even 52-128 B take
    pb_xpage_kernel (every even length when forced), 64 / 128 B pb_xsmall_kernel, the rest and
    everything under PBGPU_KERNEL=linear pb_small_kernel."""
    if form.startswith("linear"):
        kern = "pb_small_kernel"
    elif flen % 2 == 0 and (form.startswith("xpage_forced") or (4096 % flen and 52 <= flen <= 128)):
        kern = "pb_xpage_kernel"
    else:
        kern = "pb_xsmall_kernel" if 4096 % flen == 0 else "pb_small_kernel"
    return "%s<%d, %d, false," % (kern, 16 if flen <= 64 else 32, PROTO_NUM[proto])


def small_cases():
    """(id, proto, frame length, form, patterns, expected kernel prefix)"""
    out = []
    for proto in ("udp", "tcp"):
        for flen in XS_LENS:
            if flen <= HL[proto]:  # no room for a payload byte
                continue
            for form in SMALL_FORMS:
                pats = ("ramp",) + (OTHER_PATTERNS if flen in SMALL_OTHER_LENS else ())
                out.append(("%s_%d_%s" % (proto, flen, form), proto, flen, form, pats, small_kernel(proto, flen, form)))
    return out


# ------------------------------------------------------------------ b. pb_stage_kernel<G, 0>
# The longest frame whose stage still fits the LDS, and one byte more (pb_gpf_kernel).  They follow
# stage_bytes in pbgpu_load_sequence: one frame per window, round16(flen + 30) + PB_STAGE_LDS(64)
# (6724 B) <= 64 KiB, so flen <= 58770 whatever the protocol.
STAGE_MAX_FLEN = 58770
STAGE_LENS = [129, 130, 131, 132, 143, 144, 145, 242, 1500, 1501, 1502, 1503, 4096, 4097, 9043, STAGE_MAX_FLEN]
STAGE_COUNTS = [1, 7, 33, 129, 1031]
STAGE_OTHER_LENS = (131, 1501, 9043)
STAGE_OTHER_PATTERNS = ("ff", "x80_even", "x80_odd")
# forced shapes of test_gpu_kernels.SHAPES and the group size each one gives at these lengths
STAGE_SHAPES = {
    "stage_g8_wgf5": ({"PBGPU_KERNEL": "stage", "PBGPU_G": "8", "PBGPU_WGF": "5"}, 8),
    "stage_g64_kb4": ({"PBGPU_KERNEL": "stage", "PBGPU_G": "64", "PBGPU_STAGE_KB": "4"}, 64),
    "stage_wave": ({"PBGPU_KERNEL": "stage", "PBGPU_WGT": "64", "PBGPU_WGF": "24"}, None),
    "stage_g32_kb36": ({"PBGPU_KERNEL": "stage", "PBGPU_G": "32", "PBGPU_STAGE_KB": "36"}, 32),
}
STAGE_SHAPE_LENS = (242, 1501, 9043)


def stage_g(flen):
    """Lanes per frame pbgpu_load_sequence picks for a fixed length: the smallest group that wastes
    the fewest lanes and whose 256 / G frames span at most 26 KiB; at these lengths 8 up to 242 B,
    16 around 1500 B, 64 from 4096 B."""
    return 8 if flen <= 242 else (16 if flen < 4096 else 64)


def counts_for(flen, counts=STAGE_COUNTS):
    return [n for n in counts if n * flen <= BUDGET]


def stage_cases():
    """(id, proto, l4csum, frame length, env, patterns, expected kernel name)"""
    out = []
    for proto in ("udp", "tcp", "icmp"):
        for csum in (1, 0):
            for flen in STAGE_LENS:
                pats = ("ramp",) + (STAGE_OTHER_PATTERNS if flen in STAGE_OTHER_LENS else ())
                out.append(("%s_csum%d_%d" % (proto, csum, flen), proto, csum, flen, {}, pats,
                            "pb_stage_kernel<%d, 0>" % stage_g(flen)))
        for shape, (env, g) in STAGE_SHAPES.items():
            for flen in STAGE_SHAPE_LENS:
                out.append(("%s_%s_%d" % (proto, shape, flen), proto, 1, flen, env, ("ramp",),
                            "pb_stage_kernel<%d, 0>" % (g or stage_g(flen))))
    return out


# ------------------------------------------------------------------ c. pb_gpf_kernel<G, 0>
LONGEST = {"udp": 65493, "tcp": 65481}  # PB_MAX_PCKT_LEN - headers
GPF_FRAMES = 8


def gpf_cases():
    """(id, proto, payload length, env, patterns, frame counts, expected kernel name)"""
    out = []
    for proto in ("udp", "tcp"):
        for plen in (STAGE_MAX_FLEN + 1 - HL[proto], 60000, LONGEST[proto]):
            out.append(("%s_%d" % (proto, plen), proto, plen, {}, ("ramp", "ff"), [GPF_FRAMES], "pb_gpf_kernel<32, 0>"))
        for flen in (242, 1501):
            for g in (8, 64):
                out.append(("%s_forced_g%d_%d" % (proto, g, flen), proto, flen - HL[proto],
                            {"PBGPU_KERNEL": "gpf", "PBGPU_G": str(g)}, ("ramp",), counts_for(flen),
                            "pb_gpf_kernel<%d, 0>" % g))
    return out


# ------------------------------------------------------------------ d. RMODE 2, long
def mixed_payloads(which):
    ramp = pattern("ramp", 4097)
    text = "".join(chr(33 + (5 * i) % 94) for i in range(300))  # 300 printable characters
    return {
        "hex_rnd_srnd_str": [{"exact": hex_text(ramp[:1400])}, {"length": {"min": 100, "max": 1400}},
                             {"isstatic": 1, "length": {"min": 900, "max": 1000}}, {"exact": text, "isstring": 1}],
        "rnd_hex1_hex4097": [{"length": {"min": 2000, "max": 3000}}, {"exact": "a7"}, {"exact": hex_text(ramp)}],
        "srnd58k_rnd": [{"isstatic": 1, "length": {"min": 58000, "max": 60000}}, {"length": {"min": 0, "max": 40}}],
    }[which]


MIXED_SETS = {"hex_rnd_srnd_str": (3, 300), "rnd_hex1_hex4097": (3, 300), "srnd58k_rnd": (3, 16)}


def mixed_cases():
    """(id, proto, payload set, env, payload rule, iteration counts, expected kernel name)"""
    out = []
    for proto in ("udp", "tcp"):
        for which, counts in MIXED_SETS.items():
            for kernel, env in (("default", {}), ("gpf", {"PBGPU_KERNEL": "gpf"})):
                for rule in (0, 1):
                    # a window of two of the third set's frames does not fit the LDS: group per frame
                    stage = kernel == "default" and which != "srnd58k_rnd"
                    out.append(("%s_%s_%s_%s" % (proto, which, kernel, "literal" if rule else "stream"), proto, which, env,
                                rule, counts, "pb_stage_kernel<8, 2>" if stage else "pb_gpf_kernel<8, 2>"))
    return out


def mixed_cfg(proto, which):
    cfg = copy.deepcopy(pc.get(BASE[proto]))
    cfg["payloads"] = mixed_payloads(which)
    return cfg


def expected_kernel_names():
    names = {c[-1] for c in small_cases()}
    for table in (stage_cases(), gpf_cases(), mixed_cases()):
        names |= {c[-1] for c in table}
    return names
