/*
 * sequence_gpu.h — the reference's sequence surface (src/sequence.h:52-53)
 * driven by the MI355X build.
 *
 * seq_send() starts the sequence's TX threads — `threads` of them as in the
 * reference (sequence.c:741; 0 = one per GPU here, where the reference takes
 * get_nprocs()), spread round robin over --gpus GPUs.  Thread t owns a UMEM of
 * NUM_FRAMES x FRAME_SIZE slots (af_xdp.h:23-24; with --sharedumem its own
 * power-of-two slot range of one UMEM per sequence), a TX ring + completion ring
 * (an AF_XDP socket on queue t, or the in-memory loopback), and shard t of the
 * iteration space.  It builds batches of iterations with pbgpu_build() into two
 * device buffers alternately — batch n + 1 builds on the GPU while batch n is
 * landed in the UMEM slots and its TX descriptors are filled and submitted,
 * completions reaped as send_packet()/complete_tx() do (af_xdp.c:25-53,
 * 178-241).
 *
 * Differences from the reference prototypes (sequence.h:52-53), kept because
 * PB-Common's headers are not in the reference snapshot: the sequence and
 * config types are this build's mirrors (include/pb_config.h), and seq_send's
 * last argument is the AF_XDP + GPU command line (struct cmd_line_af_xdp)
 * where the reference passes PB-Common's struct cmd_line.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <time.h>

#include "../../include/pb_config.h"
#include "../../include/pbgpu.h"
#include "cmd_line.h"

#define PB_NUM_FRAMES 4096 /* af_xdp.h:23 */
#define PB_FRAME_SIZE 4096 /* af_xdp.h:24, XSK_UMEM__DEFAULT_FRAME_SIZE */

/* Called for every frame the TX side consumes (loopback / pcap backends), in
 * send order; a nonzero return is reported on stderr and the loop continues
 * (sequence.c:607-610). */
typedef int (*pb_tx_fn)(void *tx_ctx, int thread_id, const uint8_t *frame, uint16_t len);

void pb_set_tx_hook(pb_tx_fn fn, void *tx_ctx);
void pb_request_stop(void); /* async-signal-safe: workers stop after their current batch */
int pb_stop_requested(void);
void pb_set_verbose(int verbose);
/* --encap (main_gpu.c's own option, like --pcapdump): every sequence's frames are encapsulated on
 * the GPU (pbgpu_encap) before they are landed or packed.  The mode and its fields as parsed; the
 * outer MACs are filled in per sequence from the ones pb_seq_prepare resolves, TTL 64, TOS 0, the
 * source port hashed.  NULL: none (the default). */
void pb_set_encap(const pbgpu_encap_opts *opts);
const pbgpu_encap_opts *pb_get_encap(void);
/* --fragment MTU[:ignoredf] (main_gpu.c's own option): every built batch is fragmented on the GPU
 * (pbgpu_fragment) before it is verified again, encapsulated, landed or packed.  NULL: none (the
 * default). */
void pb_set_fragment(const pbgpu_frag_opts *opts);
const pbgpu_frag_opts *pb_get_fragment(void);
/* --segment MSS[:fixedid] (main_gpu.c's own option): every built batch's TCP and UDP frames are cut
 * into segments of at most MSS payload bytes on the GPU (pbgpu_segment) after the batch is stamped and
 * verified and before it is verified again, fragmented, translated, encapsulated, landed or packed.
 * NULL: none (the default). */
void pb_set_segment(const pbgpu_seg_opts *opts);
const pbgpu_seg_opts *pb_get_segment(void);
/* What --segment makes of a sequence's frames, the longest of which is `longest` bytes: NO_L4_CSUM is
 * added to *opts exactly when the sequence's l4_csum is 0; *per_frame = the segments a frame can
 * become at the most, *piece = the longest frame afterwards (an ICMP sequence is not cut). */
void pb_seg_plan_for(const pb_sequence_t *seq, pbgpu_seg_opts *opts, uint32_t longest, uint32_t *per_frame,
                     uint32_t *piece);
/* --stamp head[:OFF] | tail[:OFF] (main_gpu.c's own option): every built batch is stamped on the GPU
 * (pbgpu_stamp) before it is verified, fragmented, encapsulated, landed or packed, so --verify proves
 * the updated checksums and the fragments of one packet share one stamp.  `opts` carries the offset,
 * PBGPU_STAMP_TAIL and, with t0_set, t0_ns (--pcapt0); without t0_set t0 is the realtime clock at the
 * sequence's start.  The driver fills in the rest per batch: step_ps = 10^12 / pps (0 for pps 0),
 * first_index = the batch's global frame index ((step * n_shards + shard) * batch * frames per
 * iteration on the TX path, so shards and GPUs never collide; under --pcapdump the pack's own
 * first_index, t0_ns and step_ps), NO_CSUM exactly when the sequence's l4_csum is 0.  On the TX path T
 * is the frame's scheduled time, not its wire time.  NULL: none (the default). */
void pb_set_stamp(const pbgpu_stamp_opts *opts, int t0_set);
const pbgpu_stamp_opts *pb_get_stamp(void);
/* --xlat6 SRC6/96[,DST6/96][:hashflow] (main_gpu.c's own option): every built batch is translated to
 * IPv6 on the GPU (pbgpu_xlat46) after it is stamped and verified and before it is encapsulated,
 * landed or packed.  NULL: none (the default). */
void pb_set_xlat(const pbgpu_xlat_opts *opts);
const pbgpu_xlat_opts *pb_get_xlat(void);
/* What --xlat6 refuses of a sequence, with the reason on stderr: --fragment beside it (an IPv6
 * frame is not one the fragmenter splits), a UDP sequence without an L4 checksum (its zero
 * checksum would leave wrong: IPv6 has no "none").  0: the sequence can be translated. */
int pb_xlat_refuses(const pb_sequence_t *seq, int seq_num);
/* --verifywire (main_gpu.c's own option): every batch is checked on the GPU as it leaves
 * (pbgpu_verify_wire) - the buffer that lands or is packed, after the last repack, whatever --stamp,
 * --fragment, --xlat6 and --encap made of it - once per batch and independent of --verify.  A bad frame
 * stops the sequence as --verify's does.  0: off (the default). */
void pb_set_verify_wire(int on);
int pb_get_verify_wire(void);
/* What --verifywire asks of a sequence's frames: L3_CSUM | L3_LEN with ip.csum (L3_LEN always under
 * --xlat6, whose header has nothing else), L4_CSUM with l4_csum, UDP_LEN always; a VXLAN inner frame
 * is looked for behind --encap vxlan's destination port. */
void pb_wire_opts_for(const pb_sequence_t *seq, pbgpu_wire_opts *opts);
/* a sequence's --verifywire totals and its end-of-run line */
typedef struct pb_wire_tally
{
    uint64_t frames, bad, ipv4, ipv6, inner, nol4, other;
} pb_wire_tally_t;
void pb_wire_tally_add(pb_wire_tally_t *t, const pbgpu_wire_result *r);
void pb_print_verified_wire(const pb_wire_tally_t *t);
void pb_verify_wire_failed_msg(int seq_num, uint64_t bad, uint64_t first_bad, uint64_t first_iter);

void seq_send(const char *interface, pb_sequence_t seq, uint16_t seqc, struct cmd_line_af_xdp cmd);
/* sequence.c:779-824: stop and join the workers, print the end-of-run lines,
 * free cfg, exit(). */
void shutdown_prog(pb_config_t *cfg);
/* The same without freeing cfg or exiting (library / test use); returns the
 * last worker error (0 = none). */
int pb_shutdown_stats(pb_config_t *cfg);

int pb_sequence_totals(uint16_t seq, uint64_t *pckts, uint64_t *bytes);
int pb_last_error(void);
/* Forget all sequences, totals and errors (tests run several programs' worth
 * of sequences in one process). */
void pb_reset(void);

/* TX descriptor / wakeup / completion counts summed over the finished workers
 * of a sequence (the ring protocol's own accounting). */
int pb_sequence_tx_stats(uint16_t seq, uint64_t *descs, uint64_t *completions, uint64_t *wakeups);
/* UMEMs allocated for a sequence: one per thread, or one in all with --sharedumem. */
int pb_sequence_umems(uint16_t seq, uint64_t *umems);

/* ---- the frame builder behind the workers ----
 * Default: libpbgpu (pbgpu_open / _load_sequence / _build / _copy_to_umem).
 * The table exists so host-side tests can run the worker loop (quotas, pacing,
 * stop conditions, rings) on a CPU without a GPU by installing their own. */
typedef struct pb_builder
{
    int (*open)(int gpu, void **h);
    int (*load)(void *h, uint16_t seq_idx, const pb_sequence_t *seq, const uint8_t *smac, const uint8_t *dmac,
                const pb_rules_t *rules, uint64_t seed_base);
    int (*alloc)(void *h, uint16_t seq_idx, uint64_t n_iter, void **frames);
    /* asynchronous; the frames are ready for land() */
    int (*build)(void *h, uint16_t seq_idx, uint64_t first_iter, uint64_t n_iter, void *frames);
    uint64_t (*n_frames)(void *frames);
    /* queue frames [first, first + n) -> slots first_slot.. of `umem` (stride bytes apart),
     * lengths to lens once land_wait(keep) has left at most `keep` landings queued */
    int (*land)(void *h, void *frames, uint8_t *umem, uint32_t stride, uint32_t first_slot, uint64_t first,
                uint32_t n, uint16_t *lens);
    int (*land_wait)(void *h, uint32_t keep);
    int (*host_register)(void *h, void *p, size_t n);
    int (*host_unregister)(void *h, void *p);
    void (*free_frames)(void *h, void *frames);
    void (*close)(void *h);
    /* GPUs present (pbgpu_device_count); NULL: not checked.  seq_send refuses a --gpu / --gpus
     * range past it before starting any thread. */
    int (*device_count)(int *n);
    /* --verify: the batch in `frames` checked where it was built (pbgpu_verify with `checks`): the
     * bad frames and the first one's index.  NULL: --verify is refused. */
    int (*verify)(void *h, void *frames, uint32_t checks, uint64_t *n_bad, uint64_t *first_bad);
    /* --encap: a buffer for n_iter iterations' frames with `extra` more bytes each, and the sequence's
     * longest frame; the built batch `src` encapsulated into such a buffer (pbgpu_encap), which then
     * lands and verifies like a built one.  NULL: --encap is refused. */
    int (*alloc_encap)(void *h, uint16_t seq_idx, uint64_t n_iter, uint32_t extra, void **frames, uint32_t *max_len);
    int (*encap)(void *h, void *src, const pbgpu_encap_opts *opts, void *dst);
    /* --fragment: a buffer for the fragments of n_iter iterations' frames (pbgpu_fragment_bound's
     * frames and bytes for the sequence's longest frame) with `extra` more bytes per fragment, and the
     * longest frame a fragmented batch can hold; the built batch `src` fragmented into such a buffer
     * (pbgpu_fragment), which then verifies, encapsulates and lands like a built one.  NULL:
     * --fragment is refused. */
    int (*alloc_frag)(void *h, uint16_t seq_idx, uint64_t n_iter, const pbgpu_frag_opts *opts, uint32_t extra,
                      void **frames, uint32_t *max_len);
    int (*fragment)(void *h, void *src, const pbgpu_frag_opts *opts, void *dst);
    /* --stamp: the built batch `frames` stamped in place (pbgpu_stamp over all its frames).  NULL:
     * --stamp is refused. */
    int (*stamp)(void *h, void *frames, const pbgpu_stamp_opts *opts);
    /* --xlat6: a buffer for n_iter iterations' frames with `extra` more bytes each (20, and the
     * encapsulation's when one follows), and the sequence's longest frame; the built batch `src`
     * translated into such a buffer (pbgpu_xlat46), which then encapsulates and lands like a built
     * one.  NULL: --xlat6 is refused. */
    int (*alloc_xlat)(void *h, uint16_t seq_idx, uint64_t n_iter, uint32_t extra, void **frames, uint32_t *max_len);
    int (*xlat)(void *h, void *src, const pbgpu_xlat_opts *opts, void *dst);
    /* --verifywire: the batch in `frames` checked as it leaves (pbgpu_verify_wire over all of its
     * frames).  NULL: --verifywire is refused. */
    int (*verify_wire)(void *h, void *frames, const pbgpu_wire_opts *opts, pbgpu_wire_result *res);
    /* --segment: a buffer for n_iter iterations' frames when each can become up to per_frame frames and
     * `extra` more bytes in all (the segments' headers, and what fragmenting, translating and
     * encapsulating them adds); the built batch `src` segmented into such a buffer (pbgpu_segment),
     * which then verifies, fragments, translates, encapsulates and lands like a built one.  NULL:
     * --segment is refused. */
    int (*alloc_seg)(void *h, uint16_t seq_idx, uint64_t n_iter, uint32_t per_frame, uint32_t extra, void **frames);
    int (*segment)(void *h, void *src, const pbgpu_seg_opts *opts, void *dst);
} pb_builder_t;

void pb_set_builder(const pb_builder_t *b); /* NULL: libpbgpu */

/* ---- pieces of the worker and of the end-of-run lines shared with the --pcapdump mode
 * (host/pcap_dump.c) ---- */
/* What a sequence is loaded with: the declared rules (--literal, --singlefold) and the MACs, a
 * zero source MAC resolved from `device`, a zero destination MAC from the default gateway
 * (sequence.c:111-136), with the reference's warnings and verbose lines. */
void pb_seq_prepare(const pb_sequence_t *seq, const char *device, const struct cmd_line_af_xdp *cmd, int seq_num,
                    pb_rules_t *rules, uint8_t smac[6], uint8_t dmac[6]);
/* "[n] Completed sequence with a total of ..." (sequence.c:806-820) and the --verify lines */
void pb_print_sequence_total(int seq_num, uint64_t pckts, uint64_t bytes, time_t secs);
void pb_print_verified(uint64_t frames, uint64_t bad);
void pb_verify_failed_msg(int seq_num, uint64_t bad, uint64_t first_bad, uint64_t first_iter);

/* pcap (LINKTYPE_ETHERNET) TX hook */
typedef struct pb_pcap pb_pcap_t;
pb_pcap_t *pb_pcap_open(const char *path);
int pb_pcap_tx(void *pcap, int thread_id, const uint8_t *frame, uint16_t len);
void pb_pcap_close(pb_pcap_t *p);
