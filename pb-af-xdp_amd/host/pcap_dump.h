/*
 * pcap_dump.h — pcktbatch-gpu --pcapdump FILE [--pcapt0 NS]: the sequences' frames written as a
 * pcap capture without a TX path.  Every batch is built on the GPU, packed into the file's bytes
 * there (pbgpu_pcap_pack), copied to the host in one piece and written with one write().  No UMEM,
 * no TX ring, no worker threads; one GPU (--gpu I).
 *
 * Frames are the ones `--pcap FILE` with one thread records: iterations 0, 1, 2, ... of each
 * sequence in order, max_pckts frames per sequence.  Timestamps are synthetic: frame j of a
 * sequence is stamped t0 + floor(j * step / 1000) ns with step = 10^12 / pps ps (0 without pps);
 * the first sequence's t0 is --pcapt0 (else CLOCK_REALTIME at start), the next one's the previous
 * one's t0 + floor(N_prev * step_prev / 1000).  Microsecond format, pb_pcap_open's file header.
 * With --stamp (pb_set_stamp) a batch's frames are stamped in place before anything else is done
 * with them, with the t0, step and first index its pack then takes: a record's timestamp is the T
 * its frame carries.
 */
#pragma once

#include <stdint.h>

#include "sequence_gpu.h"

/* The mode's refusals, before any GPU is opened or the file created: 0, or -EINVAL after one line
 * on stderr.  Every sequence needs max_pckts > 0 (the stop condition, in frames) and neither
 * max_bytes nor time; --pcap, --tx xsk and --gpus above 1 do not combine with it. */
int pb_pcap_dump_check(const pb_config_t *cfg, int seq_cnt, const struct cmd_line_af_xdp *cmd);

/* Runs the mode: creates `path`, dumps sequences [0, seq_cnt) and prints the end-of-run lines
 * (the per-sequence totals from pbgpu_counters, the --verify lines).  t0_set == 0: t0 is the
 * current CLOCK_REALTIME.  A stop request (pb_request_stop) finishes the current batch and leaves
 * a well-formed file.  Returns 0 or a negative PBGPU_* code after a line on stderr. */
int pb_pcap_dump(const pb_config_t *cfg, int seq_cnt, const struct cmd_line_af_xdp *cmd, const char *path, int t0_set,
                 uint64_t t0_ns);
