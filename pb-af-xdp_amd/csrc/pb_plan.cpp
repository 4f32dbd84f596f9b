// pb_plan.cpp — the host-only planner of pbgpu_load_sequence (pb_plan.h): host arithmetic only,
// no HIP runtime call.
#include <arpa/inet.h>
#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "pb_plan.h"

namespace
{

uint32_t host_rand_r(uint32_t *seed)
{
    uint32_t x = *seed, r;
    x = x * PB_LCG_A + PB_LCG_C;
    r = (x >> 16) & 0x7FFu;
    x = x * PB_LCG_A + PB_LCG_C;
    r = (r << 10) ^ ((x >> 16) & 0x3FFu);
    x = x * PB_LCG_A + PB_LCG_C;
    r = (r << 10) ^ ((x >> 16) & 0x3FFu);
    *seed = x;
    return r;
}

uint32_t host_seed(uint64_t seed_base, uint32_t seq, uint64_t k)
{
    uint64_t z = (seed_base ^ (((uint64_t)seq << 48) + k)) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)(z ^ (z >> 31));
}

int str_ieq(const char *a, const char *b)
{
    for (; *a && *b; a++, b++)
        if (tolower((unsigned char)*a) != tolower((unsigned char)*b))
            return 0;
    return *a == *b;
}

void parse_mac(const char *s, uint8_t mac[6])
{
    memset(mac, 0, 6);
    if (s)
        sscanf(s, "%hhx:%hhx:%hhx:%hhx:%hhx:%hhx", &mac[0], &mac[1], &mac[2], &mac[3], &mac[4], &mac[5]);
}

// "<ip>/<cidr>" (strtok semantics, as PB-Common rand_ip splits it); invalid
// ranges take the reference's fail path, 127.0.0.1 (sequence.c:473-482).
uint2 compile_range(const char *r)
{
    uint2 out = make_uint2(0x7F000001u, 0u);
    if (r == NULL)
        return out;
    char *cpy = strdup(r);
    if (cpy == NULL)
        return out;
    char *save = NULL;
    char *ip = strtok_r(cpy, "/", &save);
    char *cs = strtok_r(NULL, "/", &save);
    struct in_addr a;
    if (ip && cs && inet_aton(ip, &a))
    {
        int cidr = atoi(cs);
        if (cidr >= 0 && cidr <= 32)
        {
            uint32_t hm = cidr == 0 ? 0xFFFFFFFFu : (cidr == 32 ? 0u : ((1u << (32 - cidr)) - 1u));
            out = make_uint2(ntohl(a.s_addr) & ~hm, hm);
        }
    }
    free(cpy);
    return out;
}

// exact payload text -> bytes (sequence.c:269-337)
int compile_exact(const pb_payload_opt_t *po, std::vector<uint8_t> &bytes)
{
    std::vector<char> text;
    if (po->is_file)
    {
        FILE *fp = fopen(po->exact, "rb");
        if (fp)
        {
            fseek(fp, 0, SEEK_END);
            long n = ftell(fp);
            fseek(fp, 0, SEEK_SET);
            text.assign(n > 0 ? (size_t)n + 1 : 1, 0);
            if (n > 0 && fread(text.data(), 1, (size_t)n, fp) != (size_t)n)
                text.assign(1, 0);
            fclose(fp);
        }
        else
        {
            text.assign(1, 0);
        }
    }
    else
    {
        size_t n = strlen(po->exact);
        text.assign(po->exact, po->exact + n + 1);
    }
    bytes.clear();
    if (po->is_string)
    {
        size_t n = strlen(text.data());
        bytes.assign(text.data(), text.data() + n);
    }
    else
    {
        char *rest = text.data(), *tok;
        while ((tok = strtok_r(rest, " ", &rest)) != NULL)
        {
            unsigned char b = 0;
            sscanf(tok, "%2hhx", &b);
            bytes.push_back(b);
        }
    }
    return bytes.size() > PB_MAX_PCKT_LEN ? PBGPU_EINVAL : PBGPU_OK;
}

uint32_t le_word_sum(const uint8_t *p, size_t n)
{
    uint64_t s = 0;
    for (size_t j = 0; j < n; ++j)
        s += (uint64_t)p[j] << ((j & 1) * 8);
    while (s >> 16)
        s = (s & 0xFFFF) + (s >> 16);
    return (uint32_t)s;
}

// Dynamic LDS that caps a launch at per_cu workgroups per CU: total LDS per workgroup just over
// 160 KiB / (per_cu + 1).  (The measured shape: 64-B pages with 41,384 B per workgroup ran 0.29-0.30
// ms per 2^25 frames, with 46,592 B 0.35 ms like 2 per CU, profiles/r05/ab/xs9.jsonl, so the
// point just past the next count's boundary is the one to take.)
#define PB_LDS_PER_CU (160u * 1024u)
#define PB_XS_WG_PER_CU 3 // pb_xsmall_kernel
uint32_t lds_cap_pad(uint32_t static_bytes, uint32_t per_cu)
{
    const uint32_t target = PB_LDS_PER_CU / (per_cu + 1u) + 512u;
    return target > static_bytes ? target - static_bytes : 0u;
}

// small fixed frames: one lane per frame (pb_small_kernel) and its page forms
pb_kern plan_small(pb_compiled &C, const pb_opts &O)
{
    pb_kargs &K = C.K;
    const std::vector<pb_pl> &pls = C.pls;
    const uint32_t minf = C.min_flen;
    pb_kern kern = PB_KERN_SMALL;
    K.small_ndw = minf <= 64 ? 16 : 32;
    {
        // the linear small kernel's frames per workgroup: 64 for even lengths (their 64-frame
        // regions end on 128-B lines), measured 2.5% faster than 256 on the 98-B ICMP frame
        // (0.649 vs 0.666 ms per 2^25 frames; 128: 0.666; profiles/r02/ab/small_wgt_icmp98.txt);
        // odd lengths keep 256 (line-aligned regions).  PBGPU_SMALL_WGT = 64 / 128 / 256 overrides
        const uint32_t w = O.small_wgt ? O.small_wgt : (minf % 2 == 0 ? 64u : 256u);
        K.small_wgt = (w == 64 || w == 128) ? w : 0u;
    }
    const bool xp_force = O.xp_force; // pb_xpage_kernel for any even length
    if (4096 % minf == 0 && minf == 4 * K.small_ndw && !xp_force) // pages of whole frames: pb_xsmall_kernel (64 / 128 B)
    {
        kern = PB_KERN_XSMALL;
        while ((minf << K.xs_fp_shift) < 4096)
            ++K.xs_fp_shift;
        K.xs_np = 256 >> K.xs_fp_shift;
        // one wave per page is fastest with few waves per CU (profiles/r05/ab/xs9.jsonl):
        // 64-B frames 0.297-0.303 ms per 2^25 at 3 workgroups per CU, 0.323-0.329 uncapped
        // (measured for 64-B frames only; 128-B pages keep the uncapped launch)
        if (K.xs_fp_shift == 6)
            K.lds_pad = lds_cap_pad(K.xs_np * PB_XPG, PB_XS_WG_PER_CU);
    }
    else if ((xp_force && minf % 2 == 0) ||
             (O.kernel != PBO_K_NOPAGE && minf % 2 == 0 && minf >= 52 && minf <= 128 &&
              (minf % 4 == 0 && minf <= 64 ? true : !pls[0].random && O.xp_static)))
    {
        // XCD-owned 4 KiB pages for frames cut at the page edges (pb_xpage_kernel): one slot
        // per frame touching a page, 512-thread workgroups (one pass of slots): lengths of
        // 52-64 B that are multiples of 4, and static payloads at every even length of 52-128 B
        // that does not divide 4096.  Round 4 (profiles/r04/ab/len_*.jsonl, xp_*.jsonl): static
        // payloads 5-16% faster than the linear small kernel at 54-126 B, 13% at the 98-B ICMP
        // frame (0.474-0.481 vs 0.549-0.552 ms, 4 buffers), and the rate does not depend on the
        // buffer's placement; random payloads over 64 B or of 2 mod 4 lose
        // 20-30% (each straddling frame's payload generated twice); 60-B TCP 512 vs 256
        // threads 0.296-0.298 vs 0.300-0.302 ms.  Pages per workgroup: 9 for lengths of 2 mod 4 (98 B:
        // 0.474-0.481 ms vs 0.496-0.501 at 7, 0.489-0.491 at 11, 0.574-0.577 at 5), 7 otherwise
        // (68 / 100 / 120 B: 7 faster than 9), at most the slots of one pass.
        kern = PB_KERN_XPAGE;
        K.xp = 1;
        K.xp_fpp = (4096 + minf - 1) / minf + 1;
        K.xp_div = make_div(K.xp_fpp);
        K.xp_inv = 1.0 / (double)minf;
        K.xp_wgt = O.xp_wgt == 256 ? 256 : 512;
        const uint32_t want = minf % 4 == 2 ? 9u : 7u;
        K.xs_np = std::max<uint32_t>(1, std::min<uint32_t>(want, 2 * PB_WG / K.xp_fpp));
        if (O.xp_np && O.xp_np * K.xp_fpp <= 2 * PB_WG) // at most two frame slots per 256 lanes
            K.xs_np = O.xp_np;
    }
    if (!pls[0].random)
    {
        const uint32_t p0 = (K.hl - 2) / 4;
        for (uint32_t j = 0; j < pls[0].slen; ++j)
        {
            const uint32_t pos = K.hl + j;
            K.stail[pos / 4 - p0] |= (uint32_t)C.blob[pls[0].blob_off + j] << (8 * (pos % 4));
        }
    }
    // PBGPU_KERNEL=linear: neither page kernel (the page shape above stays in K, as it always has:
    // pbk_batch_kind still reads it, and batch_fusable refuses the sequence by the option)
    return O.kernel == PBO_K_LINEAR ? PB_KERN_SMALL : kern;
}

// frames > 128 B and every variable length: the group, staged, line and page kernels
pb_kern plan_large(pb_compiled &C, const pb_opts &O, pb_plan &P)
{
    pb_kargs &K = C.K;
    const std::vector<pb_pl> &pls = C.pls;
    const uint32_t minf = C.min_flen, maxf = C.max_flen, flags = K.flags;
    const int n_random = C.n_random;
    pb_kern kern = PB_KERN_GPF;
    // lanes per frame (measured, profiles/r01/gsweep): equal-length frames take
    // the group size that wastes the fewest lanes on the frame's chunk count,
    // preferring 32 (1500-B frames: 4.2 TB/s at G=32, 3.5 at 8, 2.9 at 64);
    // packed variable-length frames take 8 (configs[2]: 3.35 TB/s at 8, 2.7
    // at 32).  PBGPU_G overrides (8, 16, 32, 64) for experiments.
    if (K.fixed_len)
    {
        const uint32_t nch = (minf + 15) / 16 + 1;
        double best = -1;
        for (uint32_t gg : {32u, 16u, 8u})
        {
            const double util = (double)nch / (gg * ((nch + gg - 1) / gg));
            if (util > best + 0.05)
                best = util, K.gpf_g = gg;
        }
    }
    else
    {
        K.gpf_g = 8;
    }
    if (O.g)
        K.gpf_g = O.g;
    K.gpf_rmode = n_random == (int)pls.size() ? 1 : (n_random == 0 ? 0 : 2);
    const uint32_t ngw = PB_WG / K.gpf_g; // frames in flight per workgroup
    uint32_t fpw = O.fpw ? O.fpw : PB_WG;
    fpw = fpw < ngw ? ngw : (fpw > PB_WG ? PB_WG : fpw);
    K.gpf_fpw = fpw / ngw * ngw;

    // staged kernel (frames assembled in LDS, each window of the output written
    // as one contiguous run).  Lanes per frame G: the smallest of the group
    // sizes that waste the fewest lanes on a frame's payload chunks whose
    // 256 / G frames in flight span at most 26 KiB.  Fixed-length windows hold
    // k * 256 / G frames (~20 KiB); variable-length windows PBGPU_STAGE_KB
    // (default 24) KiB.  Measured (profiles/r01/stage): 1500-B frames 5.1 TB/s
    // at G = 16, 16 frames per window (group-per-frame: 4.1); 1024-B 5.2 at 16
    // frames; 9000-B 5.2 at G = 64.
    // variable-length frames: staged with G = 8 (configs[2], 2^23 frames: 1.81-1.86 ms
    // vs 2.01 on the group-per-frame kernel, since B writes payload chunks
    // unmasked); PBGPU_KERNEL=gpf forces the group-per-frame kernel.  A flat B
    // (one list of the window's payload chunks, checksums from LCG-cycle prefix
    // sums) measured slower: 2.1-2.5 ms
    const bool gpf_only = O.kernel == PBO_K_GPF;
    const uint32_t avg = (minf + maxf) / 2;
    const uint32_t npc = (avg - K.hl) / 16 + 2;
    double umax = 0;
    for (uint32_t gg : {8u, 16u, 32u, 64u})
        umax = std::max(umax, (double)npc / (gg * ((npc + gg - 1) / gg)));
    uint32_t sg = 64;
    for (uint32_t gg : {8u, 16u, 32u, 64u})
        if ((double)npc / (gg * ((npc + gg - 1) / gg)) >= umax - 0.02 && (PB_WG / gg) * avg <= 26 * 1024)
        {
            sg = gg;
            break;
        }
    if (!K.fixed_len)
        sg = 8;
    if (O.g)
        sg = O.g;
    const uint32_t wgt = O.wgt == 64 ? 64u : (uint32_t)PB_WG;
    uint32_t wgf = K.fixed_len ? 64 : 128;
    if (O.wgf && O.wgf <= PB_WG)
        wgf = O.wgf;
    wgf = std::min(wgf, wgt);
    uint32_t win, sbytes;
    if (K.fixed_len)
    {
        const uint32_t ngw2 = std::max(1u, wgt / sg);
        uint32_t fw = ngw2 * std::max(1u, (20u * 1024 * wgt / PB_WG) / (ngw2 * maxf));
        if (O.stage_kb)
            fw = std::max(1u, O.stage_kb * 1024 / maxf);
        if (O.fpw)
            fw = O.fpw;
        const uint32_t fit = (uint32_t)((64 * 1024 - 48 - PB_STAGE_LDS(std::max(wgf, fw))) / maxf);
        fw = std::max(1u, std::min(fw, fit)); // the stage must fit 64 KiB of LDS
        win = fw * maxf;
        sbytes = (win + 30 + 15) / 16 * 16;
    }
    else
    {
        // 24 KiB windows.  pb_vstage_kernel (configs[2], 2^25 frames, profiles/r02/ab/hv2_*):
        // 6.37 ms at 24 KiB, 6.68 at 16, 7.34 at 28 (3 workgroups per CU) since it keeps
        // only 9 header dwords per frame in LDS; with 16-dword images 16 KiB was best
        const uint32_t skb = O.stage_kb ? O.stage_kb : 24;
        sbytes = (skb * 1024 + 15) / 16 * 16;
        if (sbytes < 2 * maxf + 48)
            sbytes = (2 * maxf + 48 + 15) / 16 * 16;
        win = sbytes - maxf - 32;
    }
    if (K.fixed_len)
    {
        const uint32_t fw = win / maxf; // whole windows per workgroup
        wgf = fw > wgt ? wgt : std::min<uint32_t>(wgt / fw * fw, fw * ((wgf + fw - 1) / fw));
    }
    else if (!O.wgf)
        wgf = std::min<uint32_t>(wgt, std::max(wgf, win / minf + 1));
    if (!gpf_only && sbytes + PB_STAGE_LDS(wgf) <= 64 * 1024)
    {
        kern = PB_KERN_STAGE;
        K.gpf_g = sg;
        K.stage_win = win;
        K.stage_wgf = wgf;
        K.stage_wgt = wgt;
        K.stage_bytes = sbytes;
        // every payload random, stream rule: pb_vstage_kernel (no header pass, no
        // serial byte loops in phase A; configs[2] 1.74 vs 1.87 ms per 2^23 frames at
        // the best window of each); PBGPU_KERNEL=stage keeps pb_stage_kernel
        if (K.gpf_rmode == 1 && !(flags & PBK_LITERAL) && wgt == PB_WG && O.kernel != PBO_K_STAGE &&
            sbytes + PB_VST_LDS(wgf) <= 64 * 1024)
        {
            kern = PB_KERN_VSTAGE;
            K.vst = 1;
            K.vst_shape = O.vst_shape;
            // phase A has one lane per slot (ghosts + own frames): as many own frames as
            // lanes allow, which also spreads the per-workgroup work over the most windows
            // (configs[2], 2^25 frames: 6.37 ms at 240-252 vs 6.44 at 218 and 6.50 at 200;
            // profiles/r02/ab/wf24*)
            // (as many as still leave 4 workgroups per CU when the window's frames fit)
            K.stage_wgf = std::min<uint32_t>(K.stage_wgf, PB_WG - PB_VST_GHOSTS);
            if (!O.wgf && !K.fixed_len)
            {
                uint32_t best = PB_WG - PB_VST_GHOSTS;
                while (best > K.stage_wgf && K.stage_bytes + PB_VST_LDS(best) > 160 * 1024 / 4)
                    --best;
                K.stage_wgf = best;
            }
        }
    }
    // fixed-length staged kernel (pb_fstage_kernel): lengths > 128 B that are a
    // multiple of 4, every payload random, stream rule.  One stage buffer, then two;
    // G = the smallest of 16, 32, 64 whose stage of 256 / G frames fits 64 KiB with
    // the per-frame records; 64 frames per workgroup.  Measured on 1500-B frames
    // (profiles/r01/fstage): 1 buffer G = 16 2.12 ms per 2^23 frames, 2 buffers 2.20,
    // G = 32 2.21, G = 64 2.35, 32 / 128 frames per workgroup 2.15 / 2.20;
    // pb_stage_kernel 2.29.  PBGPU_KERNEL=stage / gpf keep the older kernels,
    // PBGPU_FST_G, PBGPU_FST_WGF, PBGPU_FST_NBUF override the shape.
    const bool fst_ok = K.fixed_len && minf > 128 && minf % 4 == 0 && K.gpf_rmode == 1 &&
                        !(flags & PBK_LITERAL) && !gpf_only && O.kernel != PBO_K_STAGE;
    // packed variable lengths, every payload random, stream rule, payloads of >= 32 B:
    // pb_vline_kernel (no LDS stage).  ICMP type 0 / code 0 is left to
    // pb_vstage_kernel: its header word sum can be 0, where the orbit sums cannot tell a
    // zero payload sum from 0xFFFF.  PBGPU_KERNEL=vstage keeps pb_vstage_kernel.
    const bool icmp00 = C.icmp00;
    if (!K.fixed_len && K.gpf_rmode == 1 && !(flags & PBK_LITERAL) && !gpf_only && minf >= K.hl + 32 &&
        maxf <= 4096 && !icmp00 && O.kernel != PBO_K_VSTAGE && O.kernel != PBO_K_STAGE)
    {
        const uint32_t nsp = K.hl == 54 ? 5u : 4u;
        uint32_t wf = O.vl_wgf ? O.vl_wgf : PB_WG - PB_VST_GHOSTS;
        wf = std::max(32u, std::min<uint32_t>(wf, PB_WG - PB_VST_GHOSTS));
        uint32_t nl48 = 0, nlines = 0;
        for (;; wf -= 4)
        {
            const uint64_t rmax = (uint64_t)wf * maxf + 256; // own frames + the line before the first
            nl48 = (maxf + 31) / 16 + 1;
            nlines = (uint32_t)(rmax / 128 + 2);
            if (PB_VL_LDS(wf, nsp, nl48, nlines) <= 40 * 1024 || wf <= 32) // >= 4 workgroups per CU
                break;
        }
        // the orbit prefix-sum table (pb_orbit_sum, pb_vline_kernel): the 2^24-step
        // walk runs once per process; each context uploads the result
        P.orbit = true;
        kern = PB_KERN_VLINE;
        K.vl = 1;
        K.vl_wgf = wf;
        K.vl_nl48 = nl48;
        K.vl_nlines = nlines;
        // PBGPU_KERNEL=vpage, one payload: the page-shaped writer (pb_vrec_kernel +
        // pb_vpage_kernel).  Bit-exact and immune to the buffer placement
        // that slows pb_vline_kernel, but 7.1 vs 4.2 ms per 2^25 configs[2] frames: each
        // page's frame setup runs one lane per frame (~6 of 64 lanes), 3.4 G VALU
        // instructions per launch against 2.0 G (profiles/r06/vpage/)
        const uint32_t nfp = (4096 + minf - 1) / minf + 1;
        if (pls.size() == 1 && nfp <= 64 && O.kernel == PBO_K_VPAGE)
        {
            kern = PB_KERN_VPAGE;
            K.vl = 0;
            K.vp = 1;
            K.vp_nfp = nfp;
        }
    }
    if (fst_ok)
    {
        const uint32_t eg = O.fst_g, ew = O.fst_wgf, en = O.fst_nbuf;
        for (uint32_t nb : {1u, 2u})
        {
            if (en && nb != en)
                continue;
            for (uint32_t gg : {16u, 32u, 64u})
            {
                if ((eg && gg != eg) || K.hl / 4 >= gg)
                    continue;
                const uint32_t ngw = PB_WG / gg;
                uint32_t fw = ew ? ew : 64;
                fw = std::max(ngw, std::min<uint32_t>(PB_WG, fw / ngw * ngw));
                const uint32_t sb = (ngw * minf + 15) / 16 * 16;
                if ((size_t)nb * sb + PB_FST_LDS(fw) <= 64 * 1024)
                {
                    K.fst_g = gg;
                    K.fst_wgf = fw;
                    K.fst_sb = sb;
                    K.fst_nbuf = nb;
                    break;
                }
            }
            if (K.fst_g)
                break;
        }
        if (K.fst_g)
            kern = PB_KERN_FSTAGE;
    }
    return kern;
}

bool kern_is_small(pb_kern k)
{
    return k == PB_KERN_SMALL || k == PB_KERN_XSMALL || k == PB_KERN_XPAGE || k == PB_KERN_XIMG;
}

} // namespace

pb_div make_div(uint32_t d)
{
    pb_div v;
    v.d = d;
    uint32_t l = 0;
    while ((1ull << l) < d)
        ++l;
    v.sh = 31 + l;
    v.m = (uint32_t)(((1ull << v.sh) + d - 1) / d);
    return v;
}

int pb_compile(uint16_t seq_idx, const pb_sequence_t *seq, const uint8_t *src_mac, const uint8_t *dst_mac,
               const pb_rules_t *rules, uint64_t seed_base, pb_compiled *out)
{
    pb_rules_t R = {PB_PAYLOAD_STREAM, PB_FOLD_FULL};
    if (rules)
        R = *rules;
    if (seq->ip.dst_ip == NULL) // seq_send refuses it, sequence.c:723-728
        return PBGPU_EINVAL;
    if (seq->pl_cnt > PB_MAX_PAYLOADS || seq->ip.range_count > PB_MAX_RANGES)
        return PBGPU_EINVAL;
    if (seq->ip.min_ttl > seq->ip.max_ttl || seq->ip.min_id > seq->ip.max_id)
        return PBGPU_EINVAL; // rand_num modulus <= 0: undefined in the reference

    pb_kargs &K = out->K;
    memset(&K, 0, sizeof K);
    uint8_t t[64];
    memset(t, 0, sizeof t);

    uint8_t sm[6], dm[6];
    if (src_mac)
        memcpy(sm, src_mac, 6);
    else
        parse_mac(seq->eth.src_mac, sm);
    if (dst_mac)
        memcpy(dm, dst_mac, 6);
    else
        parse_mac(seq->eth.dst_mac, dm);

    uint32_t proto = 17;
    if (seq->ip.protocol && str_ieq(seq->ip.protocol, "tcp"))
        proto = 6;
    else if (seq->ip.protocol && str_ieq(seq->ip.protocol, "icmp"))
        proto = 1;
    K.proto = proto;
    K.l4len = proto == 6 ? 20 : 8;
    K.hl = 14 + 20 + K.l4len;
    if (proto == 17)
        K.csum_dw = 10, K.csum_hi = 0; // byte 40
    else if (proto == 6)
        K.csum_dw = 12, K.csum_hi = 1; // byte 50
    else
        K.csum_dw = 9, K.csum_hi = 0;  // byte 36

    // template, sequence.c:161-258
    memcpy(t + 0, dm, 6);
    memcpy(t + 6, sm, 6);
    t[12] = 0x08;
    t[13] = 0x00;
    t[14] = 0x45;
    t[15] = seq->ip.tos;
    t[23] = (uint8_t)proto;
    uint32_t flags = 0;
    if (seq->ip.min_ttl != seq->ip.max_ttl)
    {
        flags |= PBK_RND_TTL;
        K.ttl_min = seq->ip.min_ttl;
        K.ttl = make_div((uint32_t)seq->ip.max_ttl - seq->ip.min_ttl + 1);
    }
    else
    {
        t[22] = seq->ip.max_ttl;
    }
    if (seq->ip.min_id != seq->ip.max_id)
    {
        flags |= PBK_RND_ID;
        K.id_min = seq->ip.min_id;
        K.id = make_div((uint32_t)seq->ip.max_id - seq->ip.min_id + 1);
    }
    else
    {
        t[18] = (uint8_t)(seq->ip.max_id >> 8);
        t[19] = (uint8_t)seq->ip.max_id;
    }
    std::vector<uint2> &ranges = out->ranges;
    ranges.clear();
    if (seq->ip.src_ip != NULL)
    {
        struct in_addr a;
        memset(&a, 0, sizeof a);
        inet_aton(seq->ip.src_ip, &a);
        memcpy(t + 26, &a.s_addr, 4);
    }
    else if (seq->ip.range_count > 0)
    {
        flags |= PBK_RND_SADDR;
        for (int r = 0; r < seq->ip.range_count; ++r)
            ranges.push_back(compile_range(seq->ip.ranges[r]));
        K.rng = make_div(seq->ip.range_count);
    }
    else
    {
        const uint32_t lo = htonl(0x7F000001u); // sequence.c:484-490
        memcpy(t + 26, &lo, 4);
    }
    {
        struct in_addr a;
        memset(&a, 0, sizeof a);
        inet_aton(seq->ip.dst_ip, &a);
        memcpy(t + 30, &a.s_addr, 4);
    }
    if (proto == 17 || proto == 6)
    {
        const uint16_t sp = proto == 17 ? seq->udp.src_port : seq->tcp.src_port;
        const uint16_t dp = proto == 17 ? seq->udp.dst_port : seq->tcp.dst_port;
        if (sp)
            t[34] = (uint8_t)(sp >> 8), t[35] = (uint8_t)sp;
        else
            flags |= PBK_RND_SPORT;
        if (dp)
            t[36] = (uint8_t)(dp >> 8), t[37] = (uint8_t)dp;
        else
            flags |= PBK_RND_DPORT;
        K.port = make_div(65535);
        flags |= PBK_PSEUDO;
    }
    if (proto == 6)
    {
        t[46] = 5 << 4;
        t[47] = (uint8_t)((seq->tcp.fin & 1) | (seq->tcp.syn & 1) << 1 | (seq->tcp.rst & 1) << 2 |
                          (seq->tcp.psh & 1) << 3 | (seq->tcp.ack & 1) << 4 | (seq->tcp.urg & 1) << 5 |
                          (seq->tcp.ece & 1) << 6 | (seq->tcp.cwr & 1) << 7);
    }
    else if (proto == 1)
    {
        t[34] = seq->icmp.type;
        t[35] = seq->icmp.code;
    }
    if (seq->ip.csum)
        flags |= PBK_IP_CSUM;
    if (seq->l4_csum)
        flags |= PBK_L4_CSUM;
    if (R.iph_fold == PB_FOLD_SINGLE)
        flags |= PBK_IPH_SINGLE;
    if (R.payload_rule == PB_PAYLOAD_LITERAL)
        flags |= PBK_LITERAL;
    memcpy(K.tmpl, t, 64);
    out->icmp00 = proto == 1 && t[34] == 0 && t[35] == 0;

    // payloads, sequence.c:264-374
    std::vector<pb_pl> &pls = out->pls;
    pls.clear();
    std::vector<uint8_t> &blob = out->blob;
    blob.assign(96, 0); // >= 80 B of zeros before every static payload
    uint16_t dl_setup[PB_MAX_PAYLOADS];
    memset(dl_setup, 0, sizeof dl_setup);
    uint32_t sseed = host_seed(seed_base, seq_idx, PB_STATIC_SEED_K); // quirk B2
    int n_random = 0;
    uint32_t max_random = 0;
    for (int i = 0; i < seq->pl_cnt; ++i)
    {
        const pb_payload_opt_t *po = &seq->pls[i];
        pb_pl P;
        memset(&P, 0, sizeof P);
        std::vector<uint8_t> bytes;
        bool is_static = po->is_static;
        if (po->exact != NULL)
        {
            is_static = true;
            int rc = compile_exact(po, bytes);
            if (rc)
                return rc;
        }
        else if (po->is_static && po->max_len > 0)
        {
            if (po->min_len > po->max_len)
                return PBGPU_EINVAL;
            uint32_t s2 = sseed;
            const uint32_t len = po->min_len + host_rand_r(&s2) % ((uint32_t)po->max_len - po->min_len + 1);
            dl_setup[i] = (uint16_t)len;
            bytes.assign(len, 0);
            if (R.payload_rule == PB_PAYLOAD_LITERAL)
            {
                // the shadowed index runs while j < data_len[j], which may pass the payload's
                // own length: those draws still advance the seed, their bytes are not sent
                for (uint32_t j = 0; j < PB_MAX_PAYLOADS && j < dl_setup[j]; ++j)
                {
                    const uint8_t v = (uint8_t)host_rand_r(&sseed);
                    if (j < len)
                        bytes[j] = v;
                }
            }
            else
            {
                for (uint32_t j = 0; j < len; ++j)
                    bytes[j] = (uint8_t)host_rand_r(&sseed);
            }
        }
        if (is_static)
        {
            dl_setup[i] = (uint16_t)bytes.size();
            P.random = 0;
            P.slen = (uint32_t)bytes.size();
            P.blob_off = (uint32_t)blob.size();
            P.ssum = le_word_sum(bytes.data(), bytes.size());
            blob.insert(blob.end(), bytes.begin(), bytes.end());
            blob.insert(blob.end(), 96 + 16 - (bytes.size() & 15), 0); // >= 96 B zero pad, 16-B aligned
        }
        else if (po->max_len > 0)
        {
            if (po->min_len > po->max_len)
                return PBGPU_EINVAL;
            P.random = 1;
            P.min_len = po->min_len;
            P.len = make_div((uint32_t)po->max_len - po->min_len + 1);
            ++n_random;
            if (po->max_len > max_random)
                max_random = po->max_len;
        }
        else
        {
            P.random = 0; // non-static, max_len 0: empty payload (sequence.c:557-560)
            P.slen = 0;
            P.blob_off = 16 + 64;
        }
        if (K.hl + (P.random ? po->max_len : P.slen) > PB_MAX_PCKT_LEN)
            return PBGPU_EINVAL;
        pls.push_back(P);
    }
    if (pls.empty()) // sequence.c:364-374
    {
        pb_pl P;
        memset(&P, 0, sizeof P);
        P.blob_off = 16 + 64;
        pls.push_back(P);
    }
    // literal rule with several payloads (quirk B8, sequence.c:349 / 552): a random payload's
    // loop `for (u16 i = 0; i < data_len[i]; i++)` reads the other payloads' data_len[]
    // entries, so it draws until the first j with data_len[j] <= j.  Entries j > i hold
    // their setup values (declared rule, as the oracle); their part of the stop index is
    // fixed per payload here, the part of j <= i is found per iteration in pb_payload.
    std::vector<uint32_t> &lit_stop = out->lit_stop;
    lit_stop.assign(pls.size(), 0);
    for (size_t i = 0; i < pls.size(); ++i)
    {
        uint32_t j = (uint32_t)i + 1;
        while (j < PB_MAX_PAYLOADS && j < dl_setup[j])
            ++j;
        lit_stop[i] = j;
    }
    if ((flags & PBK_LITERAL) || max_random <= 64)
        flags |= PBK_SUM_IN_A;

    K.pl_cnt = (uint32_t)pls.size();
    K.pl0 = pls[0];
    K.flags = flags;
    K.seed_base = seed_base;
    K.seq = seq_idx;

    // frame lengths
    uint32_t minf = 0xFFFFFFFFu, maxf = 0;
    for (const pb_pl &P : pls)
    {
        const uint32_t lo = K.hl + (P.random ? P.min_len : P.slen);
        const uint32_t hi = K.hl + (P.random ? P.min_len + P.len.d - 1 : P.slen);
        minf = lo < minf ? lo : minf;
        maxf = hi > maxf ? hi : maxf;
    }
    out->min_flen = minf;
    out->max_flen = maxf;
    out->fpi = (uint32_t)pls.size();
    out->n_random = n_random;
    const bool fixed = pls.size() == 1 && (!pls[0].random || pls[0].len.d == 1);
    K.fixed_len = fixed ? minf : 0;
    if (fixed)
        K.flen = make_div(minf);
    blob.insert(blob.end(), 64, 0);
    return PBGPU_OK;
}

pb_plan pb_make_plan(pb_compiled &C, const pb_opts &O)
{
    pb_plan P;
    pb_kargs &K = C.K;
    P.kern = K.fixed_len && C.min_flen <= 128 ? plan_small(C, O) : plan_large(C, O, P);
    // pb_ximg_kernel (static-payload ICMP frames): only IPv4 ID, TTL, checksum and
    // source address vary per frame, so the stream's bytes repeat every img_np = flen / gcd(flen,
    // 4096) pages outside those fields.  The caller builds its first img_np pages once, at load, with
    // pb_xpage_kernel (counted into a scratch counter array, not the sequence's)
    if (K.xp && K.proto == 1 && !C.pls[0].random && K.fixed_len % 2 == 0 && O.xp_img && !O.xp_force &&
        O.kernel == PBO_K_AUTO &&
        !(K.flags & (PBK_RND_SPORT | PBK_RND_DPORT)))
    {
        uint32_t g = K.fixed_len, a = PB_XPG;
        while (a)
        {
            const uint32_t t = g % a;
            g = a;
            a = t;
        }
        P.img_np = K.fixed_len / g;
        P.img_solo = O.xp_img == 2;
        if (P.img_solo)
            P.kern = PB_KERN_XIMG;
    }
    return P;
}

pb_kern pb_plan_launch(const pb_plan &P, const pb_opts &O, uint32_t batch_wgt, pb_kargs &K)
{
    pb_kern kern = P.kern;
    K.xs_grid = 0;
    if (kern != PB_KERN_XSMALL && kern != PB_KERN_XPAGE && kern != PB_KERN_XIMG)
    {
        K.lds_pad = 0; // (PBGPU_KERNEL=linear: the page shape's cap stays in the loaded K)
        return kern;
    }
    if (batch_wgt && kern == PB_KERN_XSMALL) // pb_batch_kernel's 64-B part at the batch's block size
        K.xs_np = batch_wgt >> K.xs_fp_shift;
    if (K.img && (batch_wgt || P.img_solo)) // pb_ximg_kernel / the batch's ICMP part: one page per wave
    {
        kern = PB_KERN_XIMG;
        K.xs_np = (batch_wgt ? batch_wgt : PB_WG) / 64;
    }
    else
        K.img = nullptr;
    // XCD-owned 4 KiB pages, xs_np per workgroup: pb_xsmall_kernel (one wave per page) takes
    // groups of 8 workgroups (pages past the stream are skipped);
    // pb_xpage_kernel and the batch's 64-B part take full groups of 8, then the tail pages in order
    const uint64_t nch = (K.total_bytes + 4095) / 4096;
    if (((uintptr_t)K.out & 4095u) != 0 || nch >= 0x7FFFFFFFull)
    {
        // the load-time occupancy cap (lds_pad) belongs to pb_xsmall_kernel's page launch alone: the
        // linear fallback (an output not 4-KiB aligned) keeps its own occupancy
        K.lds_pad = 0;
        return PB_KERN_SMALL;
    }
    K.xs_nch = (uint32_t)nch;
    const uint32_t np = K.xs_np;
    K.xs_full = (uint32_t)(nch / (8 * np) * 8);
    if (kern == PB_KERN_XPAGE || (batch_wgt && kern == PB_KERN_XSMALL))
        K.xs_grid = K.xs_full + (uint32_t)((nch - (uint64_t)K.xs_full * np + np - 1) / np);
    else
        K.xs_grid = (uint32_t)((nch + 8ull * np - 1) / (8ull * np) * 8);
    // (PBGPU_XP_FA64=1: the 64-bit path at any size, so the tests reach it)
    K.xp_fa_hi = kern != PB_KERN_XSMALL && ((uint64_t)nch * (4096 % K.fixed_len) >= (1ull << 31) || O.xp_fa64);
    return kern;
}

uint32_t pb_plan_len_wgf(const pb_plan &P, const pb_opts &O, const pb_kargs &K)
{
    switch (P.kern)
    {
    case PB_KERN_VPAGE: return PB_WG;
    case PB_KERN_VLINE: return K.vl_wgf;
    case PB_KERN_VSTAGE: return K.stage_wgf >= PB_VST_SCAN_MIN_WGF && !O.vst_scan3 ? K.stage_wgf : 0u;
    default: return 0;
    }
}

void pb_plan_name(const pb_plan &P, const pb_kargs &K, char *buf, size_t n)
{
    const uint32_t l4 = (K.flags & PBK_L4_CSUM) ? 1u : 0u;
    const char *rnd = K.pl0.random ? "true" : "false";
    switch (P.kern)
    {
    case PB_KERN_VPAGE:
        snprintf(buf, n, "pb_vpage_kernel<%u, %u> (after pb_vrec_kernel<%u, %u>)", K.hl, l4, K.hl, l4);
        break;
    case PB_KERN_VLINE: snprintf(buf, n, "pb_vline_kernel<%u, %u>", K.hl, l4); break;
    case PB_KERN_FSTAGE: snprintf(buf, n, "pb_fstage_kernel<%u, %u>", K.fst_g, l4); break;
    case PB_KERN_VSTAGE: snprintf(buf, n, "pb_vstage_kernel<%u, %u>", K.gpf_g, l4); break;
    case PB_KERN_STAGE: snprintf(buf, n, "pb_stage_kernel<%u, %u>", K.gpf_g, K.gpf_rmode); break;
    case PB_KERN_GPF: snprintf(buf, n, "pb_gpf_kernel<%u, %u>", K.gpf_g, K.gpf_rmode); break;
    case PB_KERN_XIMG: snprintf(buf, n, "pb_ximg_kernel<%u>", (uint32_t)PB_WG); break;
    case PB_KERN_XPAGE:
        snprintf(buf, n, "pb_xpage_kernel<%u, %u, %s, %u, %s>%s", K.small_ndw, K.proto, rnd, K.xp_wgt,
                 K.fixed_len % 4 == 0 ? "true" : "false", P.img_np ? " (in pbgpu_build_batch: pb_ximg_body)" : "");
        break;
    case PB_KERN_XSMALL:
        snprintf(buf, n, "pb_xsmall_kernel<%u, %u, %s, %u>", K.small_ndw, K.proto, rnd, (uint32_t)PB_WG);
        break;
    default:
        snprintf(buf, n, "pb_small_kernel<%u, %u, %s, %u, %u>", K.small_ndw, K.proto, rnd,
                 K.small_wgt ? K.small_wgt : (uint32_t)PB_WG, K.fixed_len % 4 == 2 ? 2u : 0u);
        break;
    }
}

void pb_plan_describe(const pb_compiled &C, const pb_plan &P, const pb_opts &O, int batch_kind, char *buf, size_t n)
{
    const pb_kargs &K = C.K;
    char name[160];
    pb_plan_name(P, K, name, sizeof name);
    size_t at = 0;
    auto put = [&](const char *key, unsigned long long v) {
        if (at < n)
            at += (size_t)snprintf(buf + at, n - at, " %s=%llu", key, v);
    };
    at = (size_t)snprintf(buf, n, "%s | flags=0x%x", name, K.flags);
    put("fixed_len", K.fixed_len);
    put("min_flen", C.min_flen);
    put("max_flen", C.max_flen);
    put("fpi", C.fpi);
    put("batch", (unsigned)batch_kind);
    put("orbit", P.orbit);
    put("img_np", P.img_np);
    put("img_solo", P.img_solo);
    if (!K.fixed_len)
        put("len_wgf", pb_plan_len_wgf(P, O, K));
    if (kern_is_small(P.kern))
    {
        uint32_t h = 2166136261u; // FNV-1a over stail's words
        for (uint32_t w : K.stail)
            h = (h ^ w) * 16777619u;
        put("small_ndw", K.small_ndw);
        put("small_wgt", K.small_wgt);
        put("stail", h);
    }
    switch (P.kern)
    {
    case PB_KERN_XSMALL:
        put("xs_fp_shift", K.xs_fp_shift);
        put("xs_np", K.xs_np);
        put("lds_pad", K.lds_pad);
        break;
    case PB_KERN_XPAGE:
    case PB_KERN_XIMG:
        put("xs_np", K.xs_np);
        put("xp_fpp", K.xp_fpp);
        put("xp_wgt", K.xp_wgt);
        break;
    case PB_KERN_GPF:
        put("gpf_g", K.gpf_g);
        put("gpf_rmode", K.gpf_rmode);
        put("gpf_fpw", K.gpf_fpw);
        break;
    case PB_KERN_STAGE:
    case PB_KERN_VSTAGE:
        put("gpf_g", K.gpf_g);
        put("gpf_rmode", K.gpf_rmode);
        put("stage_win", K.stage_win);
        put("stage_wgf", K.stage_wgf);
        put("stage_wgt", K.stage_wgt);
        put("stage_bytes", K.stage_bytes);
        if (P.kern == PB_KERN_VSTAGE)
            put("vst_shape", K.vst_shape);
        break;
    case PB_KERN_FSTAGE:
        put("fst_g", K.fst_g);
        put("fst_wgf", K.fst_wgf);
        put("fst_sb", K.fst_sb);
        put("fst_nbuf", K.fst_nbuf);
        break;
    case PB_KERN_VPAGE:
        put("vp_nfp", K.vp_nfp);
        [[fallthrough]];
    case PB_KERN_VLINE:
        put("vl_wgf", K.vl_wgf);
        put("vl_nl48", K.vl_nl48);
        put("vl_nlines", K.vl_nlines);
        break;
    default: break;
    }
}
