/*
 * pbgpu.h — C ABI of the MI355X packet-build library (libpbgpu.so).
 *
 * Drop-in seam: the reference builds one frame per loop iteration inside
 * thread_hdl() (src/sequence.c:433-602) and hands each one to
 * send_packet(xsk, thread_id, buffer, len, verbose) (src/af_xdp.h:59,
 * src/sequence.c:607).  This library replaces the build side of that seam:
 * a batch of iterations is built on the GPU into device-resident frames, then
 * landed in the (pinned) AF_XDP UMEM, after which the host fills TX
 * descriptors exactly as af_xdp.c:217-227 does.
 *
 * Conventions follow the reference's C code: plain C, int
 * returns (0 = ok, negative errno-style codes), pointer out-params for setup,
 * no exit(), diagnostics on stderr only when PBGPU_VERBOSE is set.
 *
 *   reference interface                         replaced / mirrored by
 *   ------------------------------------------  ----------------------------
 *   thread_hdl() prologue: MAC/proto parse,     pbgpu_load_sequence()
 *     template + payload prep (sequence.c:66-374)
 *   thread_hdl() hot loop body                  pbgpu_build()
 *     (sequence.c:433-602), one call per batch
 *   send_packet() memcpy into UMEM slot          pbgpu_copy_to_umem()
 *     (af_xdp.c:200-214)
 *   total_pckts/total_bytes __sync counters     pbgpu_counters()
 *     (sequence.c:12-14, 633-642)
 *   pthread fan-out, one socket per thread      one pbgpu_ctx per GPU
 *     (sequence.c:741-762)                        (packets sharded by index)
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "pb_config.h"

#ifdef __cplusplus
extern "C" {
#endif

/* error codes (negative errno values, as the reference reports errno) */
#define PBGPU_OK 0
#define PBGPU_ENOENT (-2)     /* sequence slot not loaded */
#define PBGPU_EIO (-5)        /* HIP runtime error */
#define PBGPU_ENOMEM (-12)
#define PBGPU_EINVAL (-22)    /* bad config (e.g. min > max, no dst_ip) */
#define PBGPU_ENOSPC (-28)    /* frames buffer too small */
#define PBGPU_ENODEV (-19)    /* no such GPU */
#define PBGPU_ENOTSUP (-95)   /* reserved: a valid config this build would not run on the GPU (none since round 2) */

typedef struct pbgpu_ctx pbgpu_ctx;

/* Device-resident output of one pbgpu_build() call.
 * Frame f (0 <= f < n_frames) occupies bytes
 *   [offset(f), offset(f) + len(f)) of `data`, packed back to back, where
 *   fixed_len > 0 : offset(f) = f * fixed_len, len(f) = fixed_len
 *   fixed_len == 0: offset(f) = offsets[f], len(f) = offsets[f+1] - offsets[f]
 * Frames are numbered iteration-major: f = (k - first_iter) * pl_cnt + i for
 * payload i of iteration k (the reference's inner loop, sequence.c:530).
 * Variable length: offsets[n_frames] (the total) is written by every build; the
 * packed-frame kernel writes the other offsets as 4-B low words plus one 8-B start
 * per workgroup region, and offsets[] is filled from them on first use —
 * pbgpu_copy_offsets(), pbgpu_copy_to_umem[_async]() — or by pbgpu_frames_offsets()
 * for a caller that reads offsets[] on the device itself. */
typedef struct pbgpu_frames
{
    uint8_t *data;          /* device pointer, capacity_bytes (16-B padded) */
    uint64_t *offsets;      /* device pointer, capacity_frames + 1 entries */
    void *reserved;         /* library-internal: the buffer's build-completion event */
    uint64_t *scan_tmp;     /* device scratch (length scan) */
    uint64_t capacity_frames;
    uint64_t capacity_bytes;

    /* filled by pbgpu_build() */
    uint16_t seq_idx;
    uint64_t first_iter;
    uint64_t n_frames;
    uint32_t fixed_len;     /* 0 -> variable length, see offsets */
    uint64_t total_bytes;   /* exact for fixed length; UINT64_MAX until
                               pbgpu_frames_total() for variable length */
} pbgpu_frames;

/* ---- context (one per GPU; not thread-safe within one ctx) ---- */
int pbgpu_open(int device, pbgpu_ctx **out);
void pbgpu_close(pbgpu_ctx *ctx);
const char *pbgpu_strerror(int err);
int pbgpu_device_count(int *n);

/* ---- setup: compile one sequence into its GPU template ----
 * src_mac / dst_mac: resolved MACs (the reference resolves missing ones with
 * get_src_mac_address / get_gw_mac, sequence.c:111-130); NULL -> parse
 * seq->eth strings, unset -> 00:00:00:00:00:00.
 * rules: NULL -> { PB_PAYLOAD_STREAM, PB_FOLD_FULL }. */
int pbgpu_load_sequence(pbgpu_ctx *ctx, uint16_t seq_idx, const pb_sequence_t *seq,
                        const uint8_t *src_mac, const uint8_t *dst_mac, const pb_rules_t *rules,
                        uint64_t seed_base);

/* Upper bounds of frames / bytes produced by n_iter iterations. */
int pbgpu_build_size(pbgpu_ctx *ctx, uint16_t seq_idx, uint64_t n_iter,
                     uint64_t *max_frames, uint64_t *max_bytes);

int pbgpu_frames_alloc(pbgpu_ctx *ctx, uint64_t capacity_frames, uint64_t capacity_bytes,
                       pbgpu_frames **out);
void pbgpu_frames_free(pbgpu_ctx *ctx, pbgpu_frames *frames);

/* ---- hot path: build iterations [first_iter, first_iter + n_iter) ----
 * Asynchronous on the context's stream.  Seeds: pb_config.h seed stream with
 * the seed_base given to pbgpu_load_sequence().  first_iter + n_iter must stay below
 * PB_STATIC_SEED_K (2^48 - 1); otherwise -EINVAL, with `out` and the counters unchanged.
 *
 * What a build writes (tests/test_gpu_build_bounds.py), with n_frames = n_iter * payloads per
 * iteration and total = the frames' bytes:
 *   out->data[0, total)            the frames, packed from byte 0.
 *   out->data[total, round16(total))  the pad bytes up to the next multiple of 16: zeros, or left as
 *                                  they were.  The page, line and one-lane-per-frame kernels
 *                                  (pb_xpage_kernel, pb_ximg_kernel, pb_batch_kernel, pb_small_kernel,
 *                                  pb_vline_kernel, pb_vpage_kernel) store the last 16-B chunk whole,
 *                                  zero-filled; the staged and group kernels (pb_fstage_kernel,
 *                                  pb_stage_kernel, pb_vstage_kernel, pb_gpf_kernel) mask it to the
 *                                  frame's bytes; pb_xsmall_kernel's streams (64 / 128-B frames) have
 *                                  no pad.  A caller must not rely on either.
 *   nothing else in data           not a byte before data, none at or past round16(total): neither the
 *                                  unused rest of a variable-length build's capacity nor whatever lies
 *                                  behind the buffer.
 *   out->offsets                   fixed length: not written.  Variable length: offsets[n_frames] by
 *                                  the build, offsets[0 .. n_frames) by the build or on first use
 *                                  (see pbgpu_frames); no entry past offsets[n_frames].
 *   out->scan_tmp and the buffer's library-internal side arrays are scratch.
 * So capacity_frames == n_frames and capacity_bytes == round16(n_frames * longest frame) are
 * sufficient, and a caller may carve one allocation into several buffers (checked with data
 * pointers that are 4-KiB aligned, as pbgpu_frames_alloc gives them).
 * pbgpu_build_size's max_bytes has 16 B more than that; pbgpu_frames_alloc adds 64 B for readers. */
int pbgpu_build(pbgpu_ctx *ctx, uint16_t seq_idx, uint64_t first_iter, uint64_t n_iter,
                pbgpu_frames *out);

/* Several sequences' builds at once: part i builds iterations [first_iter[i],
 * first_iter[i] + n_iter[i]) of sequence seq_idx[i] into outs[i], exactly as
 * pbgpu_build() would (same frames, offsets and counters).  The reference runs
 * its sequences side by side (sequence.c:741-762, one thread group per
 * sequence).  One fused launch (pb_batch_kernel) builds a call of n == 3 distinct
 * sequences, in any order, one of each kind, each with one payload and one frame length:
 *   1  UDP, random payload, 64 B;
 *   2  TCP, random payload, 56 or 60 B (64 B when loaded under PBGPU_XP_FORCE=1);
 *   3  ICMP, static payload (exact, string or isstatic), 66, 70, ... 126 B (2 mod 4); its part
 *      copies the stream's image (pb_ximg_body) unless the sequence was loaded under
 *      PBGPU_XP_IMG=0, PBGPU_XP_FORCE=1 or PBGPU_KERNEL = gpf, stage, vstage or vpage (the page
 *      body then; a value PBGPU_KERNEL does not know is the default).
 * configs[4]'s three (64-B UDP, 60-B TCP SYN, 98-B ICMP echo) are one such set; header fields,
 * checksum options and rules do not matter.  Environment, read when a sequence is loaded: no
 * fused form under PBGPU_BATCH=0 or PBGPU_KERNEL=linear, for a 64-B UDP sequence under
 * PBGPU_XP_FORCE=1, for kinds 2 and 3 under PBGPU_KERNEL=nopage and for kind 3 under
 * PBGPU_XP_STATIC=0 (PBGPU_XP_FORCE=1 overrides the last two); read at pbgpu_open:
 * PBGPU_BATCH_WGT=256 (the launch's block size, 512 otherwise).  The call must also give every
 * part n_iter > 0 and a buffer of its own whose data is 4-KiB aligned.  Any other call is built by
 * one launch per part that has frames, with identical frames, offsets and counters.  Every
 * part's arguments are checked first: on an error no part is built and the counters are
 * unchanged. */
int pbgpu_build_batch(pbgpu_ctx *ctx, uint32_t n, const uint16_t *seq_idx, const uint64_t *first_iter,
                      const uint64_t *n_iter, pbgpu_frames *const *outs);

int pbgpu_sync(pbgpu_ctx *ctx);
int pbgpu_frames_total(pbgpu_ctx *ctx, pbgpu_frames *frames, uint64_t *total_bytes);
/* Fills offsets[0 .. n_frames) of a variable-length build (ordered on the context's
 * stream; a no-op when they are already there). */
int pbgpu_frames_offsets(pbgpu_ctx *ctx, pbgpu_frames *frames);

/* ---- landing: device -> host ---- */
int pbgpu_copy_packed(pbgpu_ctx *ctx, const pbgpu_frames *frames, void *host_dst,
                      uint64_t byte_offset, uint64_t nbytes);
int pbgpu_copy_offsets(pbgpu_ctx *ctx, const pbgpu_frames *frames, uint64_t *host_dst);
/* UMEM landing (af_xdp.c:200-214 geometry): frame first_frame + j lands at
 * umem + (first_slot + j) * slot_stride; lens_out[j] = its length.  `umem`
 * may be any host pointer; pbgpu_host_register() it first for full speed.
 * Nothing past a frame in its slot is written, except in a tight slot (fixed
 * length, slot_stride no longer than the frame rounded up to 64 B: 64-B slots
 * for 60- or 64-B frames), which registered UMEM receives whole, the bytes past
 * the frame unspecified: back-to-back slots then cross the host link as
 * contiguous writes.
 * Runs on the context's landing stream after the build of `frames` only, so a
 * build of another buffer queued meanwhile overlaps it (double buffering);
 * returns when the frames are in place.  A frame longer than slot_stride is
 * refused (-EINVAL) before anything is written: the check uses the buffer's
 * recorded longest frame (its fixed length, or what its build, upload or repack
 * noted), so reloading a sequence slot does not change it. */
int pbgpu_copy_to_umem(pbgpu_ctx *ctx, const pbgpu_frames *frames, void *umem, uint32_t slot_stride,
                       uint32_t first_slot, uint64_t first_frame, uint32_t n, uint16_t *lens_out);
/* The same, asynchronous: returns once the landing is queued (registered UMEM;
 * unregistered memory lands synchronously).  lens_out must stay valid until
 * pbgpu_land_wait() returns for it: that call waits until at most `keep`
 * landings are still queued, oldest first, and fills their lens_out.
 * A later pbgpu_build() into the same frames buffer is ordered after the
 * landings queued from it (the build stream waits on the last one), so a
 * caller may rebuild a buffer without waiting; builds into other buffers
 * overlap the landing. */
int pbgpu_copy_to_umem_async(pbgpu_ctx *ctx, const pbgpu_frames *frames, void *umem, uint32_t slot_stride,
                             uint32_t first_slot, uint64_t first_frame, uint32_t n, uint16_t *lens_out);
int pbgpu_land_wait(pbgpu_ctx *ctx, uint32_t keep);
int pbgpu_host_register(pbgpu_ctx *ctx, void *ptr, size_t bytes);
int pbgpu_host_unregister(pbgpu_ctx *ctx, void *ptr);

/* ---- verification: check built (or uploaded) frames on the device ---- */
#define PBGPU_VERIFY_IP_CSUM 1u   /* IPv4 header words fold to 0xFFFF            */
#define PBGPU_VERIFY_TOT_LEN 2u   /* tot_len == frame length - 14                */
#define PBGPU_VERIFY_L4_CSUM 4u   /* L4 segment (+ pseudo header for proto 6/17) */
#define PBGPU_VERIFY_ALL     7u
#define PBGPU_VERIFY_SHORT   8u   /* code bit only: frame shorter than 34 B; always checked */

typedef struct pbgpu_verify_result {
    uint64_t n_checked;
    uint64_t n_bad;        /* frames failing at least one enabled check            */
    uint64_t bad_short, bad_ip_csum, bad_tot_len, bad_l4_csum;  /* per check        */
    uint64_t first_bad;    /* lowest failing frame index, UINT64_MAX if none        */
    double   device_ms;    /* device time of the verify launches (HIP events)       */
} pbgpu_verify_result;

/* Checks frames [first_frame, first_frame + n) of a built or uploaded buffer as the CPU checker's
 * verify_one does (Ethernet + IPv4 without options; the IPv4 header is the 20 bytes at 14, the
 * protocol byte 23; protocols 6 and 17 add the pseudo header; a stored UDP checksum of 0 gets no
 * special case).  A frame shorter than 34 B is bad (SHORT) whatever `checks` says and nothing else
 * is evaluated for it.  Bits above 7 in `checks` are ignored.  codes_out[j] (host memory, n bytes, or NULL) = the OR of the failed bits
 * of frame first_frame + j; first_bad is an index into the buffer.  Ordered on the context's
 * stream after the build or upload of `frames`; returns with the result.  Reads no environment
 * variable and never writes to frames->data.  -EINVAL: a range past n_frames, res == NULL, a
 * buffer never built or uploaded. */
int pbgpu_verify(pbgpu_ctx *ctx, pbgpu_frames *frames, uint64_t first_frame, uint64_t n,
                 uint32_t checks, pbgpu_verify_result *res, uint8_t *codes_out);
/* Puts the caller's n frames into an allocated buffer, packed as a build packs them: frame j is
 * host_data[host_offsets[j] - host_offsets[0] ..] (n + 1 entries), or with host_offsets == NULL
 * host_data[j * fixed_len ..].  Fills n_frames, fixed_len (0 with host_offsets), total_bytes and
 * the device offsets[]; the buffer then behaves as a built one for pbgpu_verify and the landing
 * calls.  Synchronous.  -ENOSPC: buffer too small; -EINVAL: decreasing offsets, a frame longer
 * than PB_MAX_PCKT_LEN, neither offsets nor a fixed length. */
int pbgpu_frames_upload(pbgpu_ctx *ctx, pbgpu_frames *frames, const void *host_data,
                        const uint64_t *host_offsets, uint32_t fixed_len, uint64_t n);

/* ---- pcap stream: built (or uploaded) frames packed into a capture file's bytes on the device
 *  ---- */
#define PBGPU_PCAP_FILE_HEADER 1u  /* stream starts with the 24-B pcap file header            */
#define PBGPU_PCAP_NSEC        2u  /* nanosecond file magic 0xA1B23C4D and ts_frac in ns;
                                      else 0xA1B2C3D4 and ts_frac in us                         */
typedef struct pbgpu_pcap_opts {
    uint64_t t0_ns;        /* time of index 0, ns since the epoch                               */
    uint64_t step_ps;      /* picoseconds between consecutive frames (10^12 / pps); 0 = all at t0 */
    uint64_t first_index;  /* global index of frame first_frame (so batches concatenate exactly) */
    uint32_t flags;        /* PBGPU_PCAP_*; any other bit: -EINVAL                              */
    uint32_t reserved;     /* must be 0                                                         */
} pbgpu_pcap_opts;

/* The stream of frames [first_frame, first_frame + n) of `src`, with H = 24 under FILE_HEADER, else 0:
 *   file header, little-endian u32 words: magic, 0x00040002, 0, 0, 65535, 1 (as pb_pcap_open writes);
 *   then for j in [0, n), T = t0_ns + floor((first_index + j) * step_ps / 1000):
 *     ts_sec = (T / 10^9) mod 2^32, ts_frac = T mod 10^9 (NSEC) or (T mod 10^9) / 1000,
 *     caplen = len = the frame's length, then the frame's bytes (no snaplen truncation).
 * nbytes = H + 16 n + the frames' bytes.  pbgpu_pcap_size gives nbytes alone.
 * pbgpu_pcap_pack writes the stream to dst->data[0, nbytes), zeros from nbytes up to the next
 * multiple of 16 and nothing past that; dst is an allocated frames buffer used as plain device
 * bytes: afterwards n_frames = 0, fixed_len = 0, total_bytes = nbytes (pbgpu_verify and the landing
 * calls see no frames) and pbgpu_copy_packed(ctx, dst, host, 0, nbytes) fetches the stream.  src is
 * only read.  Runs on the context's stream after the build or upload of src and after earlier work
 * on dst; returns when the stream is in place.  n == 0: nbytes = H, only the file header written.
 * -EINVAL: NULL arguments, src never built or uploaded, a range past src->n_frames, src == dst or
 * overlapping data, unknown flag bits, reserved != 0, (first_index + n - 1) * step_ps >= 2^64 (the
 * device computes it in 64 bits) or a last timestamp past 2^64 ns.  -ENOSPC: dst->capacity_bytes
 * below nbytes rounded up to 16. */
int pbgpu_pcap_size(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                    uint32_t flags, uint64_t *nbytes);
int pbgpu_pcap_pack(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                    const pbgpu_pcap_opts *opts, pbgpu_frames *dst,
                    uint64_t *nbytes, double *device_ms /* may be NULL */);

/* ---- encapsulation: built (or uploaded) frames repacked with an 802.1Q tag or a VXLAN outer
 * header on the device ---- */
#define PBGPU_ENCAP_VLAN  1u
#define PBGPU_ENCAP_VXLAN 2u
typedef struct pbgpu_encap_opts {
    uint32_t mode;         /* PBGPU_ENCAP_VLAN or PBGPU_ENCAP_VXLAN; anything else: -EINVAL        */
    uint32_t flags;        /* must be 0                                                            */
    /* VLAN */
    uint16_t tpid;         /* 0 -> 0x8100                                                          */
    uint16_t tci;          /* PCP << 13 | DEI << 12 | VID                                          */
    /* VXLAN (RFC 7348) */
    uint16_t src_port;     /* outer UDP source port; 0 -> hashed from the inner frame, see below   */
    uint16_t dst_port;     /* 0 -> 4789                                                            */
    uint32_t vni;          /* < 2^24                                                               */
    uint8_t dst_mac[6];    /* outer addresses, wire order                                          */
    uint8_t src_mac[6];
    uint8_t src_ip[4];
    uint8_t dst_ip[4];
    uint8_t ttl;           /* 0 -> 64                                                              */
    uint8_t tos;
    uint16_t reserved;     /* must be 0                                                            */
} pbgpu_encap_opts;

/* Output frame j of frames [first_frame, first_frame + n) of `src`, L the source frame's length:
 *   VLAN  (P = 4):  src[0:12] + BE16(tpid) + BE16(tci) + src[12:L]
 *   VXLAN (P = 50): dst_mac, src_mac, 08 00;
 *                   45, tos, BE16(L + 36), 00 00, 40 00, ttl, 11, csum, src_ip, dst_ip   (csum: RFC 1071)
 *                   BE16(sport), BE16(dst_port), BE16(L + 16), 00 00                     (UDP checksum 0)
 *                   08 00 00 00, vni as 3 bytes big-endian, 00;  then src[0:L]
 *     sport = src_port, or for src_port == 0: source bytes 26..37 (a missing byte counts as 0) as three
 *     little-endian u32 w0 w1 w2; x = w0^w1^w2; x ^= x >> 16; x *= 0x7FEB352D (mod 2^32); x ^= x >> 15;
 *     sport = 49152 + (x & 0x3FFF).
 * pbgpu_encap_size gives the output's frame count (n) and bytes (the frames' bytes + n * P).
 * pbgpu_encap writes the frames packed from byte 0 of dst->data, zeros up to the next multiple of 16
 * and nothing past that.  dst is then a frames buffer as after an upload: n_frames = n, fixed_len =
 * src->fixed_len + P (0 for a variable-length source), total_bytes, and for variable length the device
 * offsets[j] = off(first_frame + j) - off(first_frame) + j * P, j in [0, n]; pbgpu_verify, the landing
 * calls, pbgpu_pcap_pack and another pbgpu_encap take it like any built buffer.  src is only read.
 * Runs on the context's stream after the build or upload of src and after earlier work on dst and
 * the landings queued from it; returns when the frames are in place.  n == 0: dst becomes empty,
 * nothing is written.  pbgpu_counters is unchanged.
 * -EINVAL: NULL arguments, src never built or uploaded, a range past src->n_frames, src == dst or
 * overlapping data, unknown mode, flags or reserved nonzero, vni >= 2^24, src's shortest frame below
 * 14 B or its longest above 65535 - P (a buffer's shortest and longest frame are recorded by its build
 * or upload).  -ENOSPC: dst->capacity_frames < n or dst->capacity_bytes below the output rounded up
 * to 16.  On any error dst is unchanged. */
int pbgpu_encap_size(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                     const pbgpu_encap_opts *opts, uint64_t *frames, uint64_t *bytes);
int pbgpu_encap(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                const pbgpu_encap_opts *opts, pbgpu_frames *dst, double *device_ms /* may be NULL */);

/* ---- IPv4 fragmentation: built (or uploaded) frames repacked so that no IPv4 packet exceeds an
 * MTU, on the device ---- */
#define PBGPU_FRAG_IGNORE_DF 1u
typedef struct pbgpu_frag_opts {
    uint32_t mtu;      /* largest IPv4 packet (tot_len) allowed, 68..65535; else -EINVAL */
    uint32_t flags;    /* PBGPU_FRAG_IGNORE_DF; any other bit: -EINVAL */
    uint64_t reserved; /* must be 0 */
} pbgpu_frag_opts;
typedef struct pbgpu_frag_result {
    uint64_t n_in, n_out;      /* source frames taken, frames written */
    uint64_t n_split;          /* source frames written as 2 or more fragments */
    uint64_t n_df;             /* oversize, DF set, copied whole (no IGNORE_DF) */
    uint64_t n_other;          /* oversize but not Ethernet + IPv4 without options, copied whole */
    uint64_t out_bytes;
    uint32_t out_min_len, out_max_len;
    double   device_ms;        /* all launches of the call, one event pair */
} pbgpu_frag_result;

/* For a source frame of length L: fo = BE16 of bytes 20..21, C = (mtu - 20) & ~7, D = L - 34.
 * The frame is copied as one output frame, unchanged, when L < 34, bytes 12..13 are not 08 00, byte
 * 14 is not 0x45, L - 14 <= mtu (the frame length decides, not the stored tot_len, as in
 * pbgpu_verify), or fo & 0x4000 is set and IGNORE_DF is not.  Otherwise it becomes K = ceil(D / C)
 * output frames: fragment i carries source bytes 34 + iC .. 34 + min(D, (i + 1) C) behind src[0:14]
 * and the source's 20 header bytes with tot_len = 20 + its data bytes, the fragment field =
 * (fo & 0xC000) | MF | (((fo & 0x1FFF) + iC / 8) & 0x1FFF), MF = 0x2000 for i < K - 1 and fo & 0x2000
 * for the last, and the header checksum recomputed (RFC 1071); a source that is itself a fragment
 * is so split correctly.
 * pbgpu_fragment writes the output frames packed from byte 0 of dst->data in source and fragment
 * order, zeros up to the next multiple of 16 and nothing past that.  dst is then a frames buffer as
 * after an upload: n_frames = n_out, fixed_len = 0 with the device offsets[0 .. n_out] written
 * (fixed_len = src->fixed_len for a fixed-length source with src->fixed_len - 14 <= mtu, none of
 * whose frames can split), total_bytes, and the exact shortest and longest output frame recorded;
 * pbgpu_verify, the landing calls, pbgpu_pcap_pack, pbgpu_encap and another pbgpu_fragment take it
 * like any built buffer.  src is only read; pbgpu_counters is unchanged.  Runs on the context's
 * stream after the build or upload of src and after earlier work on dst and the landings queued
 * from it; returns when the frames are in place.  n == 0: dst becomes empty.
 * pbgpu_fragment_size gives the exact output frame count and bytes (the count and scan passes
 * only).  pbgpu_fragment_bound answers from src's recorded longest frame with no device work: with
 * Kmax = max(1, ceil((max_len - 34) / C)), frames <= n * Kmax and bytes <= n * max_len +
 * 34 n (Kmax - 1) for a variable-length source (the range's exact bytes + 34 n (Kmax - 1) for a
 * fixed-length one).
 * -EINVAL: NULL arguments, src never built or uploaded, a range past src->n_frames, src == dst or
 * overlapping data, mtu outside 68..65535, unknown flag bits, reserved != 0, src's shortest frame
 * below 14 B.  -ENOSPC: dst->capacity_frames < n_out or dst->capacity_bytes below the output rounded
 * up to 16.  On any error dst is unchanged. */
int pbgpu_fragment_size(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                        const pbgpu_frag_opts *opts, uint64_t *frames, uint64_t *bytes);
int pbgpu_fragment_bound(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                         const pbgpu_frag_opts *opts, uint64_t *frames, uint64_t *bytes);
int pbgpu_fragment(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                   const pbgpu_frag_opts *opts, pbgpu_frames *dst, pbgpu_frag_result *res /* may be NULL */);

/* ---- stamping: a sequence number and a timestamp written into built (or uploaded) frames in place,
 * the L4 checksum kept valid, on the device ---- */
#define PBGPU_STAMP_TAIL    1u  /* position counted back from the frame's end; else forward from the L4 payload */
#define PBGPU_STAMP_NO_CSUM 2u  /* leave the L4 checksum as it is */
typedef struct pbgpu_stamp_opts {
    uint64_t t0_ns;        /* time of index 0, ns since the epoch (as pbgpu_pcap_opts)                  */
    uint64_t step_ps;      /* picoseconds between consecutive frames; 0 = all at t0                     */
    uint64_t first_index;  /* global index of frame first_frame                                         */
    uint32_t offset;       /* bytes, <= 65535                                                           */
    uint32_t flags;        /* PBGPU_STAMP_*; any other bit: -EINVAL                                     */
} pbgpu_stamp_opts;
typedef struct pbgpu_stamp_result {
    uint64_t n_in;         /* frames of the range                                                       */
    uint64_t n_stamped;
    uint64_t n_short;      /* eligible, but the 16 bytes do not fit: unchanged                          */
    uint64_t n_other;      /* not Ethernet + IPv4 without options + unfragmented ICMP/TCP/UDP: unchanged */
    double   device_ms;    /* the stamp launch, one event pair                                          */
} pbgpu_stamp_result;

/* For frame first_frame + j of `frames`, bytes F, length L:
 *   other (unchanged): L < 34, F[12:14] != 08 00, F[14] != 0x45, BE16(F[20:22]) & 0x3FFF != 0 (a
 *     fragment has no L4 header of its own), F[23] not 1, 6 or 17, or TCP with L >= 47 and
 *     4 * (F[46] >> 4) < 20.
 *   H = 8 for ICMP and UDP, 4 * (F[46] >> 4) for TCP (a TCP frame with L < 47 is short); P0 = 34 + H;
 *   S = P0 + offset, or with TAIL S = L - 16 - offset.
 *   short (unchanged) unless P0 <= S and S + 16 <= L (the frame length decides, not the stored
 *     tot_len, as in pbgpu_verify).
 *   Otherwise F[S : S + 16] = BE64(first_index + j), BE64(T), T = t0_ns + floor((first_index + j) *
 *     step_ps / 1000): the T that pbgpu_pcap_pack gives record j under the same three values.
 *   Unless NO_CSUM is set the L4 checksum follows incrementally (RFC 1624 eq. 3): C = BE16 at Q, Q = 40
 *     for UDP, 50 for TCP, 36 for ICMP; a = S - 34; W = the big-endian 16-bit words of the L4 segment
 *     at even segment offsets that intersect [a, a + 16) (8 words for even a, 9 for odd a; a byte at or
 *     past L counts as 0); s = (~C & 0xFFFF) + sum over W of (~old & 0xFFFF) + sum over W of new, folded
 *     (s = (s & 0xFFFF) + (s >> 16)) until no carry is left; ~s & 0xFFFF is stored at Q.  A stored 0
 *     gets no special case, as in pbgpu_verify.
 * No other byte of frames->data changes value: not in the frame, its neighbours, the pad or past it;
 * n_frames, fixed_len, total_bytes, offsets[], the recorded shortest and longest frame and
 * pbgpu_counters are unchanged.  Runs on the context's stream after the build or upload of `frames`
 * and, being a writer, after the landings queued from it; later verifies, landings and repacks see the
 * stamped bytes.  Returns with the result (res may be NULL).  n == 0 writes nothing.  Reads no
 * environment variable.
 * -EINVAL: NULL ctx, frames or opts, a buffer never built or uploaded, a range past n_frames,
 * unknown flag bits, offset > 65535, (first_index + n - 1) * step_ps >= 2^64 or a last timestamp past
 * 2^64 ns (as pbgpu_pcap_pack).  On any error nothing is written. */
int pbgpu_stamp(pbgpu_ctx *ctx, pbgpu_frames *frames, uint64_t first_frame, uint64_t n,
                const pbgpu_stamp_opts *opts, pbgpu_stamp_result *res /* may be NULL */);

/* ---- IPv4-to-IPv6 translation: built (or uploaded) frames repacked as IPv6 on the device, stateless
 * (RFC 7915) with RFC 6052 addresses under a /96 prefix ---- */
#define PBGPU_XLAT_HASH_FLOW 1u   /* flow label hashed per frame, see below; else opts->flow_label */
typedef struct pbgpu_xlat_opts {
    uint8_t  src_prefix[12];   /* the /96 in front of the IPv4 source address, wire order */
    uint8_t  dst_prefix[12];   /* the same for the destination                            */
    uint32_t flow_label;       /* < 2^20; else -EINVAL                                    */
    uint32_t flags;            /* PBGPU_XLAT_*; any other bit: -EINVAL                    */
    uint64_t reserved;         /* must be 0                                               */
} pbgpu_xlat_opts;
typedef struct pbgpu_xlat_result {
    uint64_t n_in, n_udp, n_tcp, n_icmp;
    uint64_t n_other;          /* frames of the range that cannot be translated */
    uint64_t first_other;      /* lowest such index into src, UINT64_MAX if none */
    double   device_ms;        /* all launches of the call, one event pair */
} pbgpu_xlat_result;

/* A source frame F of length L (the frame length decides, not the stored tot_len, as in pbgpu_verify)
 * is translatable when L >= 34, F[12:14] = 08 00, F[14] = 0x45, BE16(F[20:22]) & 0x3FFF = 0 (not a
 * fragment) and it is UDP (F[23] = 17, L >= 42), TCP (F[23] = 6, L >= 54) or an ICMP echo or echo
 * reply (F[23] = 1, F[34] = 8 or 0, L >= 42).  Every other frame is `other`.  The output frame has
 * L + 20 bytes, with tc = F[15] and NH = 17, 6 or 58:
 *   F[0:12], 86 DD,
 *   0x60 | tc >> 4, (tc & 15) << 4 | fl >> 16, BE16(fl & 0xFFFF), BE16(L - 34), NH, F[22] (hop limit = TTL),
 *   src_prefix, F[26:30], dst_prefix, F[30:34],
 *   F[34:L] with the patches below.
 * fl = flow_label, or under HASH_FLOW pbgpu_encap's hash x of source bytes 26..37 (up to and including
 * x ^= x >> 15; for ICMP w2 counts as 0) & 0xFFFFF.
 * With K = the six big-endian 16-bit words of src_prefix plus the six of dst_prefix, every sum folded
 * (s = (s & 0xFFFF) + (s >> 16)) until no carry is left:
 *   UDP:  C = BE16(F[40:42]); s = fold((~C & 0xFFFF) + K); ~s & 0xFFFF goes to output bytes 60..61, a
 *         result of 0x0000 as 0xFFFF (RFC 8200 8.1).
 *   TCP:  the same with C = BE16(F[50:52]) to output bytes 70..71; a result of 0x0000 is kept.
 *   ICMP: output byte 54 = 128 for type 8, 129 for type 0; C = BE16(F[36:38]), w = BE16(F[34:36]), w' = w
 *         with the new type, PS = the 16 words of the two IPv6 addresses + (L - 34) + 58;
 *         s = fold((~C & 0xFFFF) + (~w & 0xFFFF) + w' + PS); ~s & 0xFFFF goes to output bytes 56..57, a
 *         result of 0x0000 kept.
 * No payload byte is summed.  A stored source checksum of 0 gets no special case, as in pbgpu_verify
 * and pbgpu_stamp: a UDP frame built without an L4 checksum (l4_csum off) leaves with a wrong one.
 * This version is strict: if one frame of the range is `other` the call returns -EINVAL and dst stays
 * byte for byte and field for field as it was; res, if given, still holds the counts, first_other
 * and device_ms (then the classify pass alone).  Otherwise pbgpu_xlat46 writes the frames packed
 * from byte 0 of dst->data, zeros up to the next multiple of 16 and nothing past that, and dst is a
 * frames buffer as after pbgpu_encap: n_frames = n, fixed_len = src->fixed_len + 20 (0 for a
 * variable-length source), total_bytes, the device offsets[j] = off(first_frame + j) -
 * off(first_frame) + 20 j for j in [0, n], the shortest and longest frame recorded.  src is only
 * read; pbgpu_counters is unchanged; no environment variable is read.  Runs on the context's stream
 * after the build or upload of src and after earlier work on dst and the landings queued from it;
 * returns when the frames are in place.  n == 0: dst becomes empty, nothing is written.
 * pbgpu_xlat46_size gives n and the range's bytes + 20 n with no device work beyond reading two
 * offsets of a variable-length source; it does not look at the frames.
 * -EINVAL: NULL arguments (res may be NULL), src never built or uploaded, a range past src->n_frames,
 * src == dst or overlapping data, flow_label >= 2^20, unknown flag bits, reserved != 0, src's longest
 * frame above 65515, an `other` frame.  -ENOSPC: dst->capacity_frames < n or dst->capacity_bytes below
 * the output rounded up to 16 (checked before the frames are looked at).  On any error dst is
 * unchanged. */
int pbgpu_xlat46_size(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                      const pbgpu_xlat_opts *opts, uint64_t *frames, uint64_t *bytes);
int pbgpu_xlat46(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                 const pbgpu_xlat_opts *opts, pbgpu_frames *dst, pbgpu_xlat_result *res /* may be NULL */);

/* ---- verification as sent: frames of any shape this library produces, parsed from their own bytes
 * on the device ---- */
#define PBGPU_WIRE_L3_CSUM   1u   /* every IPv4 header parsed folds to 0xFFFF (all 4*IHL bytes)        */
#define PBGPU_WIRE_L3_LEN    2u   /* IPv4 tot_len / IPv6 payload length agree with the frame's length  */
#define PBGPU_WIRE_L4_CSUM   4u   /* UDP / TCP / ICMP / ICMPv6 checksum, pseudo header where defined   */
#define PBGPU_WIRE_UDP_LEN   8u   /* a UDP header's length field == its segment's bytes                */
#define PBGPU_WIRE_ALL      15u
#define PBGPU_WIRE_MALFORMED 16u  /* code bit only, always checked: a header does not fit or is not what its type says */
#define PBGPU_WIRE_NOL4      32u  /* info bit: IP, but no level had an L4 checksum that can be evaluated */
#define PBGPU_WIRE_INNER     64u  /* info bit: a VXLAN inner frame was parsed                          */
#define PBGPU_WIRE_OTHER    128u  /* info bit: outermost ethertype neither 08 00 nor 86 DD; nothing checked */

typedef struct pbgpu_wire_opts {
    uint32_t checks;       /* PBGPU_WIRE_* bits 0..3; any other bit: -EINVAL */
    uint32_t flags;        /* must be 0 */
    uint16_t vxlan_port;   /* UDP destination port behind which a VXLAN inner frame is looked for; 0 = never */
    uint16_t reserved[3];  /* must be 0 */
} pbgpu_wire_opts;
typedef struct pbgpu_wire_result {
    uint64_t n_checked, n_bad;      /* n_bad: frames with any of code bits 0..4 */
    uint64_t bad_malformed, bad_l3_csum, bad_l3_len, bad_l4_csum, bad_udp_len;
    uint64_t first_bad;             /* lowest bad index into the buffer, UINT64_MAX if none */
    uint64_t n_ipv4, n_ipv6;        /* by the outermost ethertype (08 00 / 86 DD), malformed or not */
    uint64_t n_inner, n_nol4, n_other;  /* frames carrying that info bit */
    double   device_ms;
} pbgpu_wire_result;

/* A frame's code is the OR of what level(F, 0, L, 0) yields, F its bytes and L its length (the frame
 * length decides everywhere, never a stored length).  level(F, b, e, depth), for the bytes F[b:e):
 *   1. Ethernet.  e - b < 14: MALFORMED.  o = b + 12; while o + 2 <= e, BE16(F[o:o+2]) is 0x8100 or
 *      0x88A8 and fewer than two tags have been skipped: o += 4.  o + 2 > e: MALFORMED.
 *      et = BE16(F[o:o+2]), l3 = o + 2.
 *   2. et neither 0x0800 nor 0x86DD: OTHER at depth 0; nothing more is checked at either depth.
 *   3. IPv4.  MALFORMED if l3 + 20 > e, F[l3] >> 4 != 4, ihl = 4 * (F[l3] & 15) < 20 or l3 + ihl > e.
 *      L3_CSUM: the ihl header bytes as big-endian words fold to 0xFFFF.  L3_LEN: BE16(F[l3+2:l3+4]) ==
 *      e - l3.  l4 = l3 + ihl, S = e - l4.  BE16(F[l3+6:l3+8]) & 0x3FFF != 0 is a fragment: no L4 at this
 *      level.  Otherwise by F[l3+9]:
 *        UDP (17): S < 8 MALFORMED.  UDP_LEN: BE16(F[l4+4:l4+6]) == S.  A stored checksum 00 00: no L4
 *          evaluation at this level, not an error.  Else L4_CSUM: pseudo header (source, destination,
 *          17, S) plus the segment folds to 0xFFFF, an odd last byte padded as the high byte.
 *        TCP (6): S < 20 MALFORMED; L4_CSUM with the pseudo header of 6; 00 00 gets no special case.
 *        ICMP (1): S < 8 MALFORMED; L4_CSUM over the segment alone.
 *        any other protocol: no L4 at this level.
 *   4. IPv6.  l3 + 40 > e or F[l3] >> 4 != 6: MALFORMED.  L3_LEN: BE16(F[l3+4:l3+6]) == e - l3 - 40.
 *      l4 = l3 + 40, S = e - l4, nh = F[l3+6].  17: as IPv4's UDP with the RFC 8200 8.1 pseudo header
 *      (the two addresses, S as 32 bits, nh); a stored 00 00 is an L4_CSUM failure (and counts as an
 *      evaluation).  6: as IPv4's TCP with that pseudo header.  58 (ICMPv6): S < 4 MALFORMED; L4_CSUM
 *      with the pseudo header.  Anything else, extension headers included (not walked): no L4.
 *   5. VXLAN, at depth 0 only: vxlan_port != 0, the level is a non-fragment UDP, BE16(F[l4+2:l4+4]) ==
 *      vxlan_port, S >= 16 and F[l4+8] & 0x08: INNER, and OR in level(F, l4 + 16, e, 1).  The outer UDP
 *      checksum is still evaluated when it is not 00 00 (it covers the inner frame).
 *   6. MALFORMED at a level: that level contributes MALFORMED and none of its other bits, and no deeper
 *      level is parsed; what an outer level found stays.
 *   7. NOL4: the frame is not OTHER, no level is malformed and no level reached an L4_CSUM evaluation
 *      (a fragment, an IPv4 UDP 00 00, an unknown protocol, a non-IP inner frame under an outer 00 00).
 * The three info bits do not depend on `checks`; failure bits 0..3 appear only where enabled.  Every
 * header byte these rules read lies in a frame's first 200 bytes (22 + 60 + 8 + 8 + 22 + 60 + 20).
 * codes_out[j] (host memory, n bytes, or NULL) = the code of frame first_frame + j; first_bad is an
 * index into the buffer.  Ordered on the context's stream after the build, upload or repack of
 * `frames`; makes offsets[] present for variable length; returns with the result.  Never writes
 * frames->data, reads no environment variable, leaves pbgpu_counters alone.  n == 0: a zero result,
 * first_bad = UINT64_MAX.  A fixed length under 14 is answered on the host (every frame MALFORMED).
 * -EINVAL: NULL ctx, frames, opts or res; a buffer never built or uploaded; a range past n_frames;
 * unknown `checks` bits; flags or reserved nonzero. */
int pbgpu_verify_wire(pbgpu_ctx *ctx, pbgpu_frames *frames, uint64_t first_frame, uint64_t n,
                      const pbgpu_wire_opts *opts, pbgpu_wire_result *res, uint8_t *codes_out);

/* ---- L4 segmentation: built (or uploaded) TCP and UDP frames cut into MSS-sized segments, each
 * with headers and checksums of its own (TSO / UDP_SEGMENT), on the device ---- */
#define PBGPU_SEG_NO_L4_CSUM 1u  /* the L4 checksum field is copied from the source as it is; no payload byte is summed */
#define PBGPU_SEG_FIXED_ID   2u  /* every segment keeps the source's IPv4 ID; else ID + i */
typedef struct pbgpu_seg_opts {
    uint32_t mss;      /* L4 payload bytes per segment, 8..65535; else -EINVAL */
    uint32_t flags;    /* PBGPU_SEG_*; any other bit: -EINVAL */
    uint64_t reserved; /* must be 0 */
} pbgpu_seg_opts;
typedef struct pbgpu_seg_result {
    uint64_t n_in, n_out;      /* source frames taken, frames written */
    uint64_t n_split_tcp;      /* TCP source frames written as 2 or more segments */
    uint64_t n_split_udp;      /* UDP ones */
    uint64_t n_other;          /* L - 42 > mss but not eligible (see below), copied whole */
    uint64_t out_bytes;
    uint32_t out_min_len, out_max_len;
    double   device_ms;        /* all launches of the call, one event pair */
} pbgpu_seg_result;

/* A source frame F of length L is eligible when L >= 34, F[12:14] = 08 00, F[14] = 0x45,
 * BE16(F[20:22]) & 0x3FFF = 0 (not a fragment) and it is UDP (F[23] = 17, L >= 42, H = 8) or TCP
 * (F[23] = 6, L >= 54, H = 4 (F[46] >> 4), 20 <= H, 34 + H <= L; options allowed).  The frame length
 * decides, never a stored length.  P = L - 34 - H.  A frame that is not eligible or has P <= mss is
 * copied as one output frame, unchanged; n_other counts the ineligible ones with L - 42 > mss (a
 * frame with L - 42 <= mss cannot split and is not read).  Otherwise it becomes K = ceil(P / mss)
 * frames; segment i carries Pi = min(mss, P - i mss) payload bytes F[34+H+i mss : 34+H+i mss+Pi]
 * behind F[0:14], the 20 IPv4 header bytes with tot_len = 20 + H + Pi, ID = (ID + i) mod 2^16
 * (unchanged under FIXED_ID) and the header checksum recomputed (RFC 1071), all else kept, and
 *   TCP: the H header bytes with the sequence number + i mss (mod 2^32), FIN and PSH cleared in every
 *        segment but the last, CWR cleared in every segment but the first, options copied, and the
 *        checksum over the pseudo header (addresses, 6, H + Pi) and the segment, 0x0000 kept;
 *   UDP: the ports, length 8 + Pi and the checksum over the pseudo header (17, 8 + Pi) and the
 *        datagram, 0x0000 stored as 0xFFFF (RFC 768).
 * Under NO_L4_CSUM the two checksum bytes are the source's in every segment.
 * pbgpu_segment writes the output frames packed from byte 0 of dst->data in source and segment order,
 * zeros up to the next multiple of 16 and nothing past that.  dst is then a frames buffer as after
 * an upload: n_frames = n_out, fixed_len = 0 with the device offsets[0 .. n_out] written (fixed_len =
 * src->fixed_len for a fixed-length source with src->fixed_len - 42 <= mss: a plain copy, no count
 * pass), total_bytes, and the exact shortest and longest output frame recorded.  src is only read;
 * pbgpu_counters is unchanged; no environment variable is read.  Ordering on the context's stream,
 * n == 0 and "dst unchanged on any error" as pbgpu_fragment.
 * pbgpu_segment_size gives the exact output frame count and bytes (the count and scan passes only).
 * pbgpu_segment_bound answers from src's recorded longest frame with no device work: with Kmax =
 * max(1, ceil((max_len - 42) / mss)), frames <= n Kmax and bytes <= n max_len + 94 n (Kmax - 1) for a
 * variable-length source (the range's exact bytes + 94 n (Kmax - 1) for a fixed-length one).
 * -EINVAL: NULL arguments, src never built or uploaded, a range past src->n_frames, src == dst or
 * overlapping data, mss outside 8..65535, unknown flag bits, reserved != 0, src's shortest frame
 * below 14 B (and a range that ends past byte 2^44 of src->data).  -ENOSPC: dst->capacity_frames <
 * n_out or dst->capacity_bytes below the output rounded up to 16. */
int pbgpu_segment_size(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                       const pbgpu_seg_opts *opts, uint64_t *frames, uint64_t *bytes);
int pbgpu_segment_bound(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                        const pbgpu_seg_opts *opts, uint64_t *frames, uint64_t *bytes);
int pbgpu_segment(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                  const pbgpu_seg_opts *opts, pbgpu_frames *dst, pbgpu_seg_result *res /* may be NULL */);

/* ---- counters (sequence.c:12-14, 633-642): frames built / bytes stored per
 * sequence since open, recorded by the build kernels' workgroups as they finish
 * their share (a skipped or short build shows here) and folded into the totals
 * here, when a sequence's record ring fills and when its slot is reloaded;
 * multi-GPU callers all-reduce these over RCCL. ---- */
int pbgpu_counters(pbgpu_ctx *ctx, uint64_t *pckts, uint64_t *bytes, int n_seq);

/* ---- measurement ---- */
/* Device time of the frame-build kernels launched since the last call, from
 * HIP events on the ctx stream, and the launch count.  PBGPU_TIMING_LAUNCH
 * (default): an event pair around every launch, ms_total = the sum of the
 * kernels' durations.  PBGPU_TIMING_SPAN: one event before the first launch
 * after the last call and one at this call, ms_total = the span on the device
 * (launch gaps included).  Each timing event is a release to system scope that
 * writes back the L2's dirty lines: the per-launch pair costs ~9 us between
 * back-to-back 2-GiB launches, so a continuously sending caller
 * runs in span mode. */
#define PBGPU_TIMING_LAUNCH 0
#define PBGPU_TIMING_SPAN 1
int pbgpu_set_timing(pbgpu_ctx *ctx, int mode);
int pbgpu_kernel_time(pbgpu_ctx *ctx, double *ms_total, uint32_t *n_launches);
/* PBGPU_TIMING_LAUNCH only: each launch's own device time since the last call
 * (the first `cap` of them into ms_each, oldest first) and the launch count. */
int pbgpu_kernel_times(pbgpu_ctx *ctx, double *ms_each, uint32_t cap, uint32_t *n_launches);
/* Write-only roofline probe: `reps` launches (best of two trials) of each of
 * PBGPU_FILL_SHAPES fill shapes over `bytes` — 16-B stores per lane at 16 / 4 /
 * 8 KiB per workgroup, plain and non-temporal, workgroups per CU capped by LDS, linear or
 * XCD-contiguous workgroup regions,
 * and the runtime's hipMemsetD32Async (probes/wbench.hip found the fastest plain
 * fills).  pbgpu_fill_probe returns the fastest shape's mean
 * device time per launch; _ex returns every shape's and the fastest's index,
 * pbgpu_fill_shape_name names a shape. */
#define PBGPU_FILL_SHAPES 15
int pbgpu_fill_probe(pbgpu_ctx *ctx, uint64_t bytes, uint32_t reps, double *ms_per_launch);
int pbgpu_fill_probe_ex(pbgpu_ctx *ctx, uint64_t bytes, uint32_t reps, double *ms_per_shape, int *best_shape);
/* The same shapes over the caller's device buffer `dst` (e.g. a pbgpu_frames data buffer): the
 * write rate of each shape at that buffer's physical placement. */
int pbgpu_fill_probe_at(pbgpu_ctx *ctx, void *dst, uint64_t bytes, uint32_t reps, double *ms_per_shape);
const char *pbgpu_fill_shape_name(int shape);
/* Read-only counterpart over the caller's device buffer `src` (16-B aligned): reps launches of one
 * plain read shape - aligned 16-B loads, 4 KiB per workgroup, an XOR of the loaded words stored
 * once per workgroup - and their mean device time.  What pbgpu_verify is measured against. */
int pbgpu_read_probe_at(pbgpu_ctx *ctx, const void *src, uint64_t bytes, uint32_t reps, double *ms_per_launch);
/* The launch shape of the repack writers (pcap pack, encap, fragment, segment, xlat46) of this
 * context over an output of `npages` 4-KiB pages: pages per workgroup and workgroups.  per is
 * clamp(npages / 16384, 1, 32), or PBGPU_RP_PER (1 to 32) as read at pbgpu_open, and more where the
 * grid would pass 2^24.  Launches nothing. */
int pbgpu_page_grid(pbgpu_ctx *ctx, uint64_t npages, uint32_t *per, uint32_t *grid);

/* Name of the frame-build kernel variant a loaded sequence launches
 * (as rocprofv3 reports it). */
int pbgpu_kernel_name(pbgpu_ctx *ctx, uint16_t seq_idx, char *buf, size_t n);
/* Test hook: what pbgpu_load_sequence would choose for this sequence under the present PBGPU_*
 * environment, with no context and no device.  One line: the kernel's name as pbgpu_kernel_name
 * prints it, " | ", then key=value pairs (flags, fixed_len, min_flen, max_flen, fpi, batch, orbit,
 * img_np, img_solo, then the shape fields the chosen kernel reads).  -EINVAL exactly where
 * pbgpu_load_sequence refuses the sequence. */
int pbgpu_plan_describe(uint16_t seq_idx, const pb_sequence_t *seq, const pb_rules_t *rules, uint64_t seed_base,
                        char *buf, size_t n);

/* ABI self-description for FFI bindings: sizes / offsets of the structs above.
 * which: 0 sizeof(pb_sequence_t), 1 sizeof(pb_payload_opt_t), 2 sizeof(pbgpu_frames),
 *        3 offsetof(pb_sequence_t, ip.ranges), 4 offsetof(pb_sequence_t, pls),
 *        5 offsetof(pb_sequence_t, pl_cnt), 6 offsetof(pbgpu_frames, total_bytes),
 *        7 sizeof(pbgpu_verify_result), 8 sizeof(pbgpu_pcap_opts), 9 sizeof(pbgpu_encap_opts),
 *        10 sizeof(pbgpu_frag_opts), 11 sizeof(pbgpu_frag_result),
 *        12 sizeof(pbgpu_stamp_opts), 13 sizeof(pbgpu_stamp_result),
 *        14 sizeof(pbgpu_xlat_opts), 15 sizeof(pbgpu_xlat_result),
 *        16 sizeof(pbgpu_wire_opts), 17 sizeof(pbgpu_wire_result),
 *        18 sizeof(pbgpu_seg_opts), 19 sizeof(pbgpu_seg_result);
 * returns 0 for an unknown index. */
size_t pbgpu_abi_size(int which);

#ifdef __cplusplus
}
#endif
