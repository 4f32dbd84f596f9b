// pb_plan.h — the host-only planner of pbgpu_load_sequence (pb_plan.cpp): a sequence compiled into
// the header template, the payload list and the static blob (pb_compile), and the build kernel and
// its shape chosen from that and the PBGPU_* overrides (pb_make_plan).  No HIP runtime call: both
// run on a machine without a GPU (pbgpu_plan_describe, tests/test_plan_cpu.py).  The choice is one
// value, pb_kern, kept in the sequence's slot and read by the launch (pbk_launch_build), the grid
// (pbk_build_grid), the name (pb_plan_name) and pbgpu_build (pb_plan_launch, pb_plan_len_wgf).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/pbgpu.h"
#include "pb_device.h"

#define PB_VST_SCAN_MIN_WGF 32 // smallest pb_vstage_kernel workgroup the scratch is sized for

// Shape overrides for the parity tests and A/B runs (PBGPU_* environment).  They are read in
// one place, read_opts() (pbgpu.cpp): at pbgpu_open into the context (landing, batch and repack
// options) and at pbgpu_load_sequence into the slot (kernel shapes), so the build path never reads
// the environment and a loaded sequence's shape is fixed.  Every selectable shape is parity-tested
// (tests/test_gpu_kernels.py).
enum pb_kern_force
{
    PBO_K_AUTO = 0,
    PBO_K_GPF,    // PBGPU_KERNEL=gpf: the group-per-frame kernel for frames > 128 B
    PBO_K_STAGE,  // =stage: pb_stage_kernel
    PBO_K_VSTAGE, // =vstage: pb_vstage_kernel for packed variable lengths
    PBO_K_NOPAGE, // =nopage: no pb_xpage_kernel (linear small kernel)
    PBO_K_LINEAR, // =linear: neither page kernel
    PBO_K_VPAGE,  // =vpage: the page-shaped packed writer (pb_vrec_kernel + pb_vpage_kernel)
};

struct pb_opts
{
    int kernel = PBO_K_AUTO;
    uint32_t g = 0;          // PBGPU_G: lanes per frame of the staged / group kernels (8, 16, 32, 64)
    uint32_t fpw = 0;        // PBGPU_FPW: frames per workgroup of the group kernel / staged window
    uint32_t wgt = 0;        // PBGPU_WGT=64: one-wave staged workgroups
    uint32_t wgf = 0;        // PBGPU_WGF: staged frames per workgroup
    uint32_t stage_kb = 0;   // PBGPU_STAGE_KB: staged window
    uint32_t small_wgt = 0;  // PBGPU_SMALL_WGT: linear small kernel's workgroup (64 / 128 / 256)
    uint32_t fst_g = 0, fst_wgf = 0, fst_nbuf = 0; // PBGPU_FST_G / _WGF / _NBUF
    uint32_t vl_wgf = 0;     // PBGPU_VL_WGF: pb_vline_kernel's own frames per workgroup
    uint32_t vst_shape = 0;  // PBGPU_VST_SHAPE: pb_vstage_kernel shape bits (pb_kargs.vst_shape)
    bool vst_scan3 = false;  // PBGPU_VST_SCAN=3pass: pb_vstage_kernel after the 3-pass length scan
    bool xp_force = false;   // PBGPU_XP_FORCE=1: pb_xpage_kernel for every even length <= 128 B
    bool xp_static = true;   // PBGPU_XP_STATIC=0: no page kernel for static payloads
    bool xp_fa64 = false;    // PBGPU_XP_FA64=1: pb_xpage_kernel's 64-bit first-frame path at any size
    uint32_t xp_wgt = 0;     // PBGPU_XP_WGT: 256 / 512
    uint32_t xp_np = 0;      // PBGPU_XP_NP: pages per workgroup
    uint32_t xp_img = 1;     // static-payload ICMP frames: 1 pb_ximg_body in pb_batch_kernel only,
                             // 2 pb_ximg_kernel for single builds too, 0 never (PBGPU_XP_IMG)
    bool ctr_atomic = false; // PBGPU_CTR_ATOMIC=1: counts by one atomic per workgroup, no record ring
    uint32_t ctr_ring = 0;   // PBGPU_CTR_RING: record ring words (small: the fold-when-full path)
    bool batch = true;       // PBGPU_BATCH=0: pbgpu_build_batch launches every part on its own
    uint32_t batch_wgt = 512; // PBGPU_BATCH_WGT=256: pb_batch_kernel's 256-thread form
    bool seq_streams = true; // PBGPU_SEQ_STREAMS=0: span-mode builds all on the context's stream
    bool land_spin = true;   // PBGPU_LAND_SPIN=0: blocking landing waits
    bool umem_dma = false;   // PBGPU_UMEM_DMA=1: land through DMA copies, not the mapped scatter
    bool alloc_vmm = true;   // PBGPU_ALLOC=malloc: frame buffers from hipMalloc (fb_alloc)
    uint32_t alloc_chunk_mb = 64; // PBGPU_ALLOC_CHUNK_MB: fb_alloc's physical chunk
    uint32_t land_dma_min = 0xFFFFFFFFu; // PBGPU_LAND_DMA_MIN: fixed frames of at least this many bytes
                                  // land in registered UMEM by strided DMA instead of the scatter kernel
                                  // (off by default: 1500 B read 56 vs 52 GB/s landing alone on one box,
                                  // 43 vs 49 GB/s in bench.py's build + land on another)
    uint32_t vp_pages_pct = 0; // PBGPU_VP_PAGES_PCT: pb_vpage_kernel's grid as a percentage of the
                               // expected pages (tests: a short grid, so waves take several pages)
    uint32_t rp_per = 0;       // PBGPU_RP_PER: pages per workgroup of the five repack writers, 1 to 32
                               // (tests: several pages per workgroup at outputs of a few MB)
};

// The build kernel of a loaded sequence, or of one launch (pb_plan_launch)
enum pb_kern
{
    PB_KERN_NONE = 0,
    PB_KERN_SMALL,  // pb_small_kernel: one lane per frame, frames in order
    PB_KERN_XSMALL, // pb_xsmall_kernel: pages of whole frames (64 / 128 B)
    PB_KERN_XPAGE,  // pb_xpage_kernel: frames cut at the page edges
    PB_KERN_XIMG,   // pb_ximg_kernel: pages copied from the load-time image
    PB_KERN_GPF,    // pb_gpf_kernel
    PB_KERN_STAGE,  // pb_stage_kernel
    PB_KERN_VSTAGE, // pb_vstage_kernel
    PB_KERN_FSTAGE, // pb_fstage_kernel
    PB_KERN_VLINE,  // pb_vline_kernel
    PB_KERN_VPAGE,  // pb_vrec_kernel + pb_vpage_kernel
};

// pb_compile's result: pb_kargs' scalar fields (every pointer null) and the tables to upload
struct pb_compiled
{
    pb_kargs K;
    std::vector<uint2> ranges;
    std::vector<pb_pl> pls;
    std::vector<uint32_t> lit_stop;
    std::vector<uint8_t> blob;
    uint32_t min_flen = 0, max_flen = 0;
    uint32_t fpi = 1; // frames per iteration
    int n_random = 0; // random payloads
    bool icmp00 = false; // ICMP type 0 / code 0
};

// pb_make_plan's result beside the shape fields it sets in pb_compiled.K: the kernel, and what
// the caller must still do on the device
struct pb_plan
{
    pb_kern kern = PB_KERN_NONE;
    bool orbit = false;    // K.orbit, K.orbit_tot: the orbit prefix-sum table
    uint32_t img_np = 0;   // > 0: K.img, an image of this many pages, built with pb_xpage_kernel
    bool img_solo = false; // ... that single builds launch too (pb_ximg_kernel), not only the batch's part
};

pb_div make_div(uint32_t d);

// sequence_t -> the host side of the GPU template (thread_hdl() prologue, sequence.c:66-374);
// PBGPU_EINVAL for a sequence the reference refuses or leaves undefined
int pb_compile(uint16_t seq_idx, const pb_sequence_t *seq, const uint8_t *src_mac, const uint8_t *dst_mac,
               const pb_rules_t *rules, uint64_t seed_base, pb_compiled *out);
// The build kernel and its shape (C.K's small_*, xs_*, lds_pad, xp*, gpf_*, stage_*, vst*, fst_*,
// vl_*, vp, vp_nfp, stail)
pb_plan pb_make_plan(pb_compiled &C, const pb_opts &O);
// The kernel one build launches, and its page arithmetic in K (xs_*, xp_fa_hi, img, lds_pad) once
// K.out and K.total_bytes are set; batch_wgt: the block size of pbgpu_build_batch's fused launch
// when the build is a part of it, else 0
pb_kern pb_plan_launch(const pb_plan &P, const pb_opts &O, uint32_t batch_wgt, pb_kargs &K);
// Frames per workgroup of the kernel's own length pass (pbk_launch_vst_lengths); 0: a variable-length
// build scans the offsets beforehand (pbk_launch_lengths)
uint32_t pb_plan_len_wgf(const pb_plan &P, const pb_opts &O, const pb_kargs &K);
// The kernel's name as rocprofv3 reports it (pbgpu_kernel_name)
void pb_plan_name(const pb_plan &P, const pb_kargs &K, char *buf, size_t n);
// One line: the name, then key=value pairs of the sequence and of the shape fields the kernel, its
// linear fallback, its launch line and its grid read (pbgpu_plan_describe)
void pb_plan_describe(const pb_compiled &C, const pb_plan &P, const pb_opts &O, int batch_kind, char *buf, size_t n);
