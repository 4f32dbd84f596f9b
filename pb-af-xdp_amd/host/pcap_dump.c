/*
 * pcap_dump.c — pcktbatch-gpu --pcapdump (pcap_dump.h).
 *
 * Per sequence: two frame buffers and two stream buffers on the GPU, two registered host buffers.
 * Batch k is (with --stamp stamped in place, verified, with --segment cut into segments in a buffer of
 * their own and verified again, with --fragment fragmented into a fragment buffer
 * and verified again, with --xlat6 translated to IPv6 into a buffer of its own, with --encap encapsulated
 * into a third frame buffer,) packed into stream buffer k & 1; batch k + 1's build is queued into the
 * other frame buffer; then stream k is copied to its host buffer in one piece and written with
 * one write() per buffer (looped only on a short write).
 */
#include "pcap_dump.h"

#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#define PB_DUMP_BATCH_BYTES_MAX (256ull << 20) /* device bytes per frame buffer, as the TX workers' */

int pb_pcap_dump_check(const pb_config_t *cfg, int seq_cnt, const struct cmd_line_af_xdp *cmd)
{
    if (cmd->pcap)
    {
        fprintf(stderr, "--pcapdump does not combine with --pcap: one capture per run.\n");
        return PBGPU_EINVAL;
    }
    if (cmd->tx && strcmp(cmd->tx, "xsk") == 0)
    {
        fprintf(stderr, "--pcapdump does not combine with --tx xsk: it has no TX path.\n");
        return PBGPU_EINVAL;
    }
    if (cmd->gpus > 1)
    {
        fprintf(stderr, "--pcapdump runs on one GPU (--gpu I); --gpus %d given.\n", cmd->gpus);
        return PBGPU_EINVAL;
    }
    for (int i = 0; i < seq_cnt; ++i)
    {
        const pb_sequence_t *s = &cfg->seq[i];
        if (s->max_bytes || s->time)
        {
            fprintf(stderr, "[%d] --pcapdump stops on a packet count only: %s is set.\n", i + 1,
                    s->max_bytes ? "max bytes" : "time");
            return PBGPU_EINVAL;
        }
        if (s->max_pckts == 0)
        {
            fprintf(stderr, "[%d] --pcapdump needs a packet count (--maxpckts / \"maxpckts\") above 0.\n", i + 1);
            return PBGPU_EINVAL;
        }
        if (pb_xlat_refuses(s, i + 1) != 0)
            return PBGPU_EINVAL;
    }
    return PBGPU_OK;
}

static int write_all(int fd, const uint8_t *p, uint64_t n)
{
    while (n)
    {
        const ssize_t w = write(fd, p, n);
        if (w < 0)
        {
            if (errno == EINTR)
                continue;
            return -1;
        }
        p += w;
        n -= (uint64_t)w;
    }
    return 0;
}

typedef struct dump_state
{
    pbgpu_ctx *ctx;
    int fd;
    int header_due; /* the run's first pack carries the file header */
    const struct cmd_line_af_xdp *cmd;
    const char *device;
} dump_state_t;

/* One sequence: frames [0, max_pckts) stamped from t0_ns; *n_done = the frames written. */
static int dump_sequence(dump_state_t *D, const pb_sequence_t *seq, uint16_t idx, uint64_t t0_ns, uint64_t step_ps,
                         uint64_t *n_done, uint64_t *n_verified, uint64_t *n_bad, uint64_t *n_packed, uint64_t *b_packed,
                         pb_wire_tally_t *wire)
{
    const int seq_num = idx + 1;
    pbgpu_ctx *ctx = D->ctx;
    pbgpu_frames *src[2] = {NULL, NULL}, *dst[2] = {NULL, NULL};
    pbgpu_frames *enc = NULL; /* --encap: the batch as it is packed (the pack returns before the next encap) */
    pbgpu_frames *frg = NULL; /* --fragment: the batch's fragments (what is encapsulated, or packed) */
    pbgpu_frames *x6 = NULL;  /* --xlat6: the batch as IPv6 (what is encapsulated, or packed) */
    pbgpu_frames *sgm = NULL; /* --segment: the batch's segments (what is fragmented, translated, encapsulated or packed) */
    uint8_t *hb[2] = {NULL, NULL};
    int reg[2] = {0, 0};
    int rc;
    uint64_t done = 0, iter = 0; /* built frames written; the current batch's first iteration */
    uint64_t packed = 0, packed_b = 0; /* frames packed (--fragment: fragments) and their bytes */
    pb_rules_t rules;
    uint8_t smac[6], dmac[6];
    pb_seq_prepare(seq, D->device, D->cmd, seq_num, &rules, smac, dmac);
    if ((rc = pbgpu_load_sequence(ctx, idx, seq, smac, dmac, &rules, D->cmd->seed_base)) != 0)
    {
        fprintf(stderr, "[%d] Error loading sequence on GPU %d :: %s.\n", seq_num, D->cmd->gpu_first, pbgpu_strerror(rc));
        return rc;
    }
    /* --encap: the outer MACs are the sequence's */
    const int encap = pb_get_encap() != NULL;
    pbgpu_encap_opts eopts;
    memset(&eopts, 0, sizeof eopts);
    if (encap)
        eopts = *pb_get_encap();
    memcpy(eopts.dst_mac, dmac, 6);
    memcpy(eopts.src_mac, smac, 6);
    /* --xlat6: 20 more bytes a frame, ahead of the encapsulation's (never beside --fragment) */
    const pbgpu_xlat_opts *xo = pb_get_xlat();
    const uint32_t xextra = xo ? 20u : 0u;
    const uint32_t extra = (encap ? (eopts.mode == PBGPU_ENCAP_VLAN ? 4u : 50u) : 0u) + xextra;
    const uint32_t fpi = seq->pl_cnt < 1 ? 1u : seq->pl_cnt;
    const uint64_t quota = seq->max_pckts;
    uint64_t batch = D->cmd->gpu_batch ? D->cmd->gpu_batch : (1u << 20);
    if (batch > (quota + fpi - 1) / fpi)
        batch = (quota + fpi - 1) / fpi;
    uint64_t mf = 0, mb = 0;
    for (;;)
    {
        if ((rc = pbgpu_build_size(ctx, idx, batch, &mf, &mb)) != 0)
            goto out;
        if (batch == 1 || mb <= PB_DUMP_BATCH_BYTES_MAX)
            break;
        batch >>= 1;
    }
    /* --fragment: pbgpu_fragment_bound's arithmetic for the sequence's longest frame (16 iterations:
     * the size bound is then the frames times that frame, plus 16) */
    const pbgpu_frag_opts *fo = pb_get_fragment();
    uint64_t of = mf, obytes = mb; /* the frames and bytes a batch can become before it is encapsulated */
    /* --segment: first, so the fragmenter's bound below starts from the segments (94 bytes of headers
     * at the most for each but a frame's first) */
    const int segm = pb_get_segment() != NULL;
    pbgpu_seg_opts sgo;
    memset(&sgo, 0, sizeof sgo);
    uint64_t longest = 0;
    if (segm || fo)
    {
        uint64_t f16 = 0, b16 = 0;
        if ((rc = pbgpu_build_size(ctx, idx, 16, &f16, &b16)) != 0)
            goto out;
        longest = f16 ? (b16 - 16) / f16 : 0;
    }
    if (segm)
    {
        sgo = *pb_get_segment();
        uint32_t ks = 1, piece = 0;
        pb_seg_plan_for(seq, &sgo, (uint32_t)longest, &ks, &piece);
        of = mf * ks;
        obytes = mb + 94 * mf * (ks - 1) + 16;
        longest = piece;
        if ((rc = pbgpu_frames_alloc(ctx, of, obytes, &sgm)) != 0)
            goto out;
    }
    if (fo)
    {
        const uint64_t c = (fo->mtu - 20u) & ~7u;
        const uint64_t kmax = longest > fo->mtu + 14ull ? (longest - 34 + c - 1) / c : 1;
        obytes += 34 * of * (kmax - 1) + 16;
        of *= kmax;
        if ((rc = pbgpu_frames_alloc(ctx, of, obytes, &frg)) != 0)
            goto out;
    }
    const uint64_t cap = 24 + (16 + extra) * of + obytes + 16;
    if (encap && (rc = pbgpu_frames_alloc(ctx, of, obytes + extra * of + 16, &enc)) != 0)
        goto out;
    if (xo && (rc = pbgpu_frames_alloc(ctx, of, obytes + xextra * of + 16, &x6)) != 0)
        goto out;
    const size_t page = (size_t)sysconf(_SC_PAGESIZE);
    for (int i = 0; i < 2; ++i)
    {
        if ((rc = pbgpu_frames_alloc(ctx, mf, mb, &src[i])) != 0 || (rc = pbgpu_frames_alloc(ctx, 1, cap, &dst[i])) != 0)
            goto out;
        if (posix_memalign((void **)&hb[i], page, (cap + page - 1) / page * page) != 0)
        {
            hb[i] = NULL;
            rc = PBGPU_ENOMEM;
            goto out;
        }
        memset(hb[i], 0, cap);
        reg[i] = pbgpu_host_register(ctx, hb[i], cap) == 0; /* unregistered memory still works, slower */
    }
    const uint32_t vchecks = (seq->ip.csum ? PBGPU_VERIFY_IP_CSUM | PBGPU_VERIFY_TOT_LEN : 0u) |
                             (seq->l4_csum ? PBGPU_VERIFY_L4_CSUM : 0u);
    uint64_t n_cur = batch;
    int cur = 0;
    if ((rc = pbgpu_build(ctx, idx, 0, n_cur, src[0])) != 0)
    {
        fprintf(stderr, "[%d] Error building frames on GPU %d :: %s.\n", seq_num, D->cmd->gpu_first, pbgpu_strerror(rc));
        goto out;
    }
    /* --stamp: the frames that will be packed, with the pack's own t0, step and first index */
    const pbgpu_stamp_opts *so = pb_get_stamp();
    while (n_cur)
    {
        if (so)
        {
            const uint64_t have0 = src[cur]->n_frames;
            pbgpu_stamp_opts s = *so;
            s.t0_ns = t0_ns;
            s.step_ps = step_ps;
            s.first_index = packed;
            if (!seq->l4_csum)
                s.flags |= PBGPU_STAMP_NO_CSUM;
            if ((rc = pbgpu_stamp(ctx, src[cur], 0, have0 < quota - done ? have0 : quota - done, &s, NULL)) != 0)
            {
                fprintf(stderr, "[%d] Error stamping frames on GPU %d :: %s.\n", seq_num, D->cmd->gpu_first,
                        pbgpu_strerror(rc));
                goto out;
            }
        }
        if (D->cmd->verify)
        {
            pbgpu_verify_result r;
            if ((rc = pbgpu_verify(ctx, src[cur], 0, src[cur]->n_frames, vchecks, &r, NULL)) != 0)
            {
                fprintf(stderr, "[%d] Error verifying frames on GPU %d :: %s.\n", seq_num, D->cmd->gpu_first,
                        pbgpu_strerror(rc));
                goto out;
            }
            *n_verified += src[cur]->n_frames;
            if (r.n_bad)
            {
                *n_bad += r.n_bad;
                pb_verify_failed_msg(seq_num, r.n_bad, r.first_bad, iter);
                rc = PBGPU_EIO;
                goto out;
            }
        }
        const uint64_t have = src[cur]->n_frames;
        const uint64_t take = have < quota - done ? have : quota - done; /* the last batch: up to the quota */
        pbgpu_frames *bf = src[cur]; /* the batch as it is encapsulated or packed, and its frames */
        uint64_t btake = take;
        if (segm)
        {
            if ((rc = pbgpu_segment(ctx, src[cur], 0, take, &sgo, sgm, NULL)) != 0)
            {
                fprintf(stderr, "[%d] Error segmenting frames on GPU %d :: %s.\n", seq_num, D->cmd->gpu_first,
                        pbgpu_strerror(rc));
                goto out;
            }
            bf = sgm;
            btake = sgm->n_frames;
            if (D->cmd->verify) /* segments are plain frames the verifier parses: the sequence's own checks again */
            {
                pbgpu_verify_result r;
                if ((rc = pbgpu_verify(ctx, sgm, 0, btake, vchecks, &r, NULL)) != 0)
                {
                    fprintf(stderr, "[%d] Error verifying frames on GPU %d :: %s.\n", seq_num, D->cmd->gpu_first,
                            pbgpu_strerror(rc));
                    goto out;
                }
                if (r.n_bad)
                {
                    *n_bad += r.n_bad;
                    pb_verify_failed_msg(seq_num, r.n_bad, r.first_bad, iter);
                    rc = PBGPU_EIO;
                    goto out;
                }
            }
        }
        if (fo)
        {
            if ((rc = pbgpu_fragment(ctx, bf, 0, btake, fo, frg, NULL)) != 0)
            {
                fprintf(stderr, "[%d] Error fragmenting frames on GPU %d :: %s.\n", seq_num, D->cmd->gpu_first,
                        pbgpu_strerror(rc));
                goto out;
            }
            bf = frg;
            btake = frg->n_frames;
            if (D->cmd->verify) /* a fragment has no L4 checksum of its own */
            {
                pbgpu_verify_result r;
                if ((rc = pbgpu_verify(ctx, frg, 0, btake, PBGPU_VERIFY_IP_CSUM | PBGPU_VERIFY_TOT_LEN, &r, NULL)) != 0)
                {
                    fprintf(stderr, "[%d] Error verifying frames on GPU %d :: %s.\n", seq_num, D->cmd->gpu_first,
                            pbgpu_strerror(rc));
                    goto out;
                }
                if (r.n_bad)
                {
                    *n_bad += r.n_bad;
                    pb_verify_failed_msg(seq_num, r.n_bad, r.first_bad, iter);
                    rc = PBGPU_EIO;
                    goto out;
                }
            }
        }
        if (xo)
        {
            if ((rc = pbgpu_xlat46(ctx, bf, 0, btake, xo, x6, NULL)) != 0)
            {
                fprintf(stderr, "[%d] Error translating frames to IPv6 on GPU %d :: %s%s.\n", seq_num, D->cmd->gpu_first,
                        pbgpu_strerror(rc), rc == PBGPU_EINVAL ? " (a frame that is not UDP, TCP or an ICMP echo?)" : "");
                goto out;
            }
            bf = x6;
        }
        if (encap && (rc = pbgpu_encap(ctx, bf, 0, btake, &eopts, enc, NULL)) != 0)
        {
            fprintf(stderr, "[%d] Error encapsulating frames on GPU %d :: %s%s.\n", seq_num, D->cmd->gpu_first,
                    pbgpu_strerror(rc), rc == PBGPU_EINVAL ? " (a frame too long for the outer header?)" : "");
            goto out;
        }
        if (pb_get_verify_wire()) /* --verifywire: the batch as it is packed, after the last repack */
        {
            pbgpu_wire_opts wo;
            pbgpu_wire_result wr;
            pb_wire_opts_for(seq, &wo);
            if ((rc = pbgpu_verify_wire(ctx, encap ? enc : bf, 0, btake, &wo, &wr, NULL)) != 0)
            {
                fprintf(stderr, "[%d] Error verifying frames as sent on GPU %d :: %s.\n", seq_num, D->cmd->gpu_first,
                        pbgpu_strerror(rc));
                goto out;
            }
            pb_wire_tally_add(wire, &wr);
            if (wr.n_bad)
            {
                pb_verify_wire_failed_msg(seq_num, wr.n_bad, wr.first_bad, iter);
                rc = PBGPU_EIO;
                goto out;
            }
        }
        pbgpu_pcap_opts o;
        memset(&o, 0, sizeof o);
        o.t0_ns = t0_ns;
        o.step_ps = step_ps;
        o.first_index = packed; /* timestamps index the frames packed */
        o.flags = D->header_due ? PBGPU_PCAP_FILE_HEADER : 0u;
        uint64_t nbytes = 0;
        if ((rc = pbgpu_pcap_pack(ctx, encap ? enc : bf, 0, btake, &o, dst[cur], &nbytes, NULL)) != 0)
        {
            fprintf(stderr, "[%d] Error packing the pcap stream on GPU %d :: %s.\n", seq_num, D->cmd->gpu_first,
                    pbgpu_strerror(rc));
            goto out;
        }
        packed += btake;
        packed_b += nbytes - (D->header_due ? 24u : 0u) - 16u * btake;
        D->header_due = 0;
        /* the next batch builds while this one's stream crosses the host link and is written */
        const uint64_t left = quota - done - take;
        uint64_t n_next = (left + fpi - 1) / fpi;
        if (n_next > batch)
            n_next = batch;
        if (pb_stop_requested())
            n_next = 0;
        if (n_next && (rc = pbgpu_build(ctx, idx, iter + n_cur, n_next, src[cur ^ 1])) != 0)
        {
            fprintf(stderr, "[%d] Error building frames on GPU %d :: %s.\n", seq_num, D->cmd->gpu_first,
                    pbgpu_strerror(rc));
            goto out;
        }
        if (nbytes && (rc = pbgpu_copy_packed(ctx, dst[cur], hb[cur], 0, nbytes)) != 0)
        {
            fprintf(stderr, "[%d] Error copying the pcap stream from GPU %d :: %s.\n", seq_num, D->cmd->gpu_first,
                    pbgpu_strerror(rc));
            goto out;
        }
        if (write_all(D->fd, hb[cur], nbytes) != 0)
        {
            fprintf(stderr, "[%d] Error writing the pcap file :: %s.\n", seq_num, strerror(errno));
            rc = PBGPU_EIO;
            goto out;
        }
        done += take;
        iter += n_cur;
        n_cur = n_next;
        cur ^= 1;
    }
    rc = PBGPU_OK;
out:
    (void)pbgpu_sync(ctx);
    for (int i = 0; i < 2; ++i)
    {
        if (reg[i])
            (void)pbgpu_host_unregister(ctx, hb[i]);
        free(hb[i]);
        pbgpu_frames_free(ctx, dst[i]);
        pbgpu_frames_free(ctx, src[i]);
    }
    pbgpu_frames_free(ctx, enc);
    pbgpu_frames_free(ctx, frg);
    pbgpu_frames_free(ctx, x6);
    pbgpu_frames_free(ctx, sgm);
    *n_done = done;
    *n_packed = packed;
    *b_packed = packed_b;
    return rc;
}

int pb_pcap_dump(const pb_config_t *cfg, int seq_cnt, const struct cmd_line_af_xdp *cmd, const char *path, int t0_set,
                 uint64_t t0_ns)
{
    int rc = pb_pcap_dump_check(cfg, seq_cnt, cmd);
    if (rc != 0)
        return rc;
    if (seq_cnt > PB_MAX_SEQUENCES)
        seq_cnt = PB_MAX_SEQUENCES;
    if (!t0_set)
    {
        struct timespec ts;
        clock_gettime(CLOCK_REALTIME, &ts);
        t0_ns = (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
    }
    dump_state_t D;
    memset(&D, 0, sizeof D);
    D.cmd = cmd;
    D.device = cfg->interface;
    D.header_due = 1;
    if ((rc = pbgpu_open(cmd->gpu_first, &D.ctx)) != 0)
    {
        fprintf(stderr, "Error opening GPU %d :: %s.\n", cmd->gpu_first, pbgpu_strerror(rc));
        return rc;
    }
    (void)pbgpu_set_timing(D.ctx, PBGPU_TIMING_SPAN); /* nobody reads per-launch timings here */
    D.fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (D.fd < 0)
    {
        fprintf(stderr, "Cannot open pcap file %s.\n", path);
        pbgpu_close(D.ctx);
        return PBGPU_EIO;
    }
    uint64_t verified[PB_MAX_SEQUENCES] = {0}, bad[PB_MAX_SEQUENCES] = {0}, written[PB_MAX_SEQUENCES] = {0};
    uint64_t packed[PB_MAX_SEQUENCES] = {0}, packed_b[PB_MAX_SEQUENCES] = {0};
    time_t secs[PB_MAX_SEQUENCES] = {0};
    pb_wire_tally_t wire[PB_MAX_SEQUENCES];
    memset(wire, 0, sizeof wire);
    int ran = 0;
    for (int i = 0; i < seq_cnt && rc == 0 && !pb_stop_requested(); ++i)
    {
        const pb_sequence_t *seq = &cfg->seq[i];
        ran = i + 1;
        if (seq->ip.dst_ip == NULL) /* sequence.c:723-728 */
        {
            fprintf(stderr, "Destination IP not set on sequence #%d. Not moving forward with this sequence.\n", i + 1);
            continue;
        }
        const uint64_t step_ps = seq->pps > 0 ? 1000000000000ull / seq->pps : 0;
        uint64_t n = 0;
        const time_t t_start = time(NULL);
        rc = dump_sequence(&D, seq, (uint16_t)i, t0_ns, step_ps, &n, &verified[i], &bad[i], &packed[i], &packed_b[i],
                           &wire[i]);
        secs[i] = time(NULL) - t_start;
        /* the next sequence continues where this one's clock stopped */
        t0_ns += (uint64_t)((unsigned __int128)packed[i] * step_ps / 1000u);
        written[i] = n;
    }
    if (D.header_due && rc == 0) /* nothing was packed: still a well-formed (empty) capture */
    {
        const uint32_t hdr[6] = {0xA1B2C3D4u, 0x00040002u, 0, 0, 65535, 1};
        if (write_all(D.fd, (const uint8_t *)hdr, sizeof hdr) != 0)
            rc = PBGPU_EIO;
    }
    if (close(D.fd) != 0 && rc == 0)
        rc = PBGPU_EIO;
    /* the end-of-run lines (sequence.c:779-824): the frames built and bytes stored, as the
     * library counted them */
    uint64_t p[PB_MAX_SEQUENCES] = {0}, b[PB_MAX_SEQUENCES] = {0};
    const int crc = ran ? pbgpu_counters(D.ctx, p, b, ran) : 0;
    if (crc != 0 && rc == 0)
        rc = crc;
    fprintf(stdout, "Completed %d sequences!\n", ran);
    /* --encap: the library counts the frames as built; the file holds the header bytes as well */
    if (pb_get_encap() && !pb_get_fragment())
        for (int i = 0; i < ran; ++i)
            b[i] += written[i] * (pb_get_encap()->mode == PBGPU_ENCAP_VLAN ? 4u : 50u);
    /* --xlat6: and the 20 bytes the IPv6 header is longer by */
    if (pb_get_xlat())
        for (int i = 0; i < ran; ++i)
            b[i] += written[i] * 20u;
    for (int i = 0; i < ran; ++i)
    {
        /* --fragment: the packets are the built ones (the quota's), the bytes what the file holds, and
         * the frames packed follow on a line of their own */
        pb_print_sequence_total(i + 1, p[i], pb_get_fragment() || pb_get_segment() ? packed_b[i] : b[i], secs[i]);
        if (pb_get_fragment())
            fprintf(stdout, "[%d] Fragmented into %llu frames.\n", i + 1, (unsigned long long)packed[i]);
        else if (pb_get_segment()) /* --segment likewise: built packets, the file's bytes, the frames packed */
            fprintf(stdout, "[%d] Segmented into %llu frames.\n", i + 1, (unsigned long long)packed[i]);
    }
    for (int i = 0; i < ran && cmd->verify; ++i)
        pb_print_verified(verified[i], bad[i]);
    for (int i = 0; i < ran && pb_get_verify_wire(); ++i)
        pb_print_verified_wire(&wire[i]);
    fflush(stdout);
    pbgpu_close(D.ctx);
    return rc;
}
