// pbgpu.cpp — C-ABI shim of libpbgpu.so (include/pbgpu.h).
//
// Host side of the drop-in seam: compiles a sequence (PB-Common sequence_t
// mirror, include/pb_config.h) into the GPU template once — the work the
// reference does in thread_hdl()'s prologue, src/sequence.c:66-374 — then
// launches the frame-build kernels per batch (the loop body,
// sequence.c:433-602) and lands frames in host memory for the AF_XDP TX path
// (af_xdp.c:200-227).  The product path has no CPU frame builder: if the HIP
// runtime or the device is missing every entry point fails with an error.
#include <arpa/inet.h>
#include <ctype.h>
#include <stddef.h>
#include <hip/hip_runtime.h>
#include <sched.h>
#include <stdio.h>
#include <time.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <unordered_map>
#include <new>
#include <deque>
#include <vector>

#include "../../include/pbgpu.h"
#include "pb_device.h"
#include "pb_plan.h"

extern "C" hipError_t pbk_launch_build(const pb_kargs *K, pb_kern kern, hipStream_t st);
extern "C" uint32_t pbk_build_grid(const pb_kargs *K, pb_kern kern);
extern "C" int pbk_batch_kind(const pb_kargs *K);
extern "C" hipError_t pbk_launch_batch(const pb_kargs *Ks, uint32_t wgt, hipStream_t st);
extern "C" hipError_t pbk_launch_ctr_fold(const uint32_t *slots, uint64_t n, uint32_t pairs,
                                          unsigned long long *counters, hipStream_t st);
extern "C" hipError_t pbk_launch_ctr_read(const unsigned long long *counters, uint32_t n_seq, unsigned long long *out,
                                          hipStream_t st);
extern "C" hipError_t pbk_launch_lengths(const pb_kargs *K, unsigned long long *block_sums, uint32_t nblocks,
                                         uint64_t *offsets, hipStream_t st);
extern "C" hipError_t pbk_launch_vst_lengths(const pb_kargs *K, uint32_t wgf, uint32_t *bsum, uint32_t nblk,
                                             unsigned long long *l2, uint32_t n_l2, uint64_t *offsets, hipStream_t st);
extern "C" hipError_t pbk_launch_expand_offsets(const uint32_t *off32, const unsigned long long *rstart, uint32_t wf,
                                                uint64_t n, uint64_t *offsets, hipStream_t st);
extern "C" hipError_t pbk_launch_scatter(const uint8_t *src, const uint64_t *offsets, uint64_t first, uint32_t n,
                                         uint8_t *dst, uint32_t stride, uint16_t *lens, hipStream_t st);
extern "C" hipError_t pbk_launch_fill(void *dst, uint64_t bytes, int mode, hipStream_t st);
extern "C" const char *pbk_fill_shape_name(int mode);
extern "C" hipError_t pbk_launch_verify(const pb_vargs *A, int shape, uint32_t grid, hipStream_t st);
extern "C" hipError_t pbk_launch_vfold(const uint32_t *rec, uint32_t nrec, uint32_t ncnt, unsigned long long *out,
                                       hipStream_t st);
extern "C" hipError_t pbk_launch_wire(const pb_wargs *A, int G, uint32_t grid, hipStream_t st);
extern "C" hipError_t pbk_launch_read(const void *src, uint64_t bytes, uint32_t *out, hipStream_t st);
extern "C" hipError_t pbk_launch_pcap(const pb_pcargs *A, uint32_t grid, hipStream_t st);
extern "C" hipError_t pbk_launch_encap(const pb_enargs *A, uint32_t grid, hipStream_t st);
extern "C" hipError_t pbk_launch_frag(const pb_cutargs *A, int stage, uint32_t grid, hipStream_t st);
extern "C" hipError_t pbk_launch_seg(const pb_cutargs *A, int stage, int G, uint32_t grid, hipStream_t st);
extern "C" hipError_t pbk_launch_cut_copy(const uint8_t *src, uint8_t *dst, uint64_t a0, uint64_t total,
                                          uint64_t end16, uint32_t per, uint32_t grid, hipStream_t st);
extern "C" hipError_t pbk_launch_stamp(const pb_spargs *A, hipStream_t st);
extern "C" hipError_t pbk_launch_xlat(const pb_xlargs *A, int stage, uint32_t grid, hipStream_t st);
extern "C" hipError_t pbk_launch_scatter_fixed(const uint8_t *src, uint32_t flen, uint32_t wlen, uint32_t n,
                                               uint64_t src_lim, uint8_t *dst, uint32_t stride, hipStream_t st);

#define PB_JUMP_N (65536 + 256) // entries j = -PB_JNEG .. 65536 + 175
#define PB_SCAN_FRAMES_PER_BLOCK (256 * 8)
#define PB_CTR_WORDS ((size_t)PB_CTR_SHARDS * PB_CTR_STRIDE) // u64 counter words per sequence
#define PB_CTR_BYTES (sizeof(unsigned long long) * PB_CTR_WORDS * PB_MAX_SEQUENCES)

// device scratch of a frames buffer: the 3-pass length scan's block sums, or pb_vstage_kernel's
// per-workgroup length sums (u32) + their per-PB_VL_GRP group sums (u64)
static uint64_t vst_bsum_bytes(uint64_t nblk)
{
    return (nblk * 4 + 15) & ~15ull;
}
static uint64_t scan_tmp_bytes(uint64_t capacity_frames)
{
    const uint64_t a = (capacity_frames / PB_SCAN_FRAMES_PER_BLOCK + 1) * 8;
    const uint64_t nblk = capacity_frames / PB_VST_SCAN_MIN_WGF + 1;
    const uint64_t b = vst_bsum_bytes(nblk) + (nblk / PB_VL_GRP + 1) * 8;
    return a > b ? a : b;
}

namespace
{

// The PBGPU_* overrides (pb_opts, pb_plan.h), read here alone
uint32_t opt_u32(const char *name)
{
    const char *e = getenv(name);
    return e != NULL && atoi(e) > 0 ? (uint32_t)atoi(e) : 0u;
}

bool opt_is(const char *name, const char *value)
{
    const char *e = getenv(name);
    return e != NULL && strcmp(e, value) == 0;
}

pb_opts read_opts()
{
    pb_opts o;
    const char *k = getenv("PBGPU_KERNEL");
    if (k)
        o.kernel = !strcmp(k, "gpf") ? PBO_K_GPF
                   : !strcmp(k, "stage") ? PBO_K_STAGE
                   : !strcmp(k, "vstage") ? PBO_K_VSTAGE
                   : !strcmp(k, "nopage") ? PBO_K_NOPAGE
                   : !strcmp(k, "linear") ? PBO_K_LINEAR
                   : !strcmp(k, "vpage") ? PBO_K_VPAGE
                                          : PBO_K_AUTO;
    o.g = opt_u32("PBGPU_G");
    if (o.g != 8 && o.g != 16 && o.g != 32 && o.g != 64)
        o.g = 0;
    o.fpw = opt_u32("PBGPU_FPW");
    o.wgt = opt_u32("PBGPU_WGT");
    o.wgf = opt_u32("PBGPU_WGF");
    o.stage_kb = opt_u32("PBGPU_STAGE_KB");
    o.small_wgt = opt_u32("PBGPU_SMALL_WGT");
    o.fst_g = opt_u32("PBGPU_FST_G");
    o.fst_wgf = opt_u32("PBGPU_FST_WGF");
    o.fst_nbuf = opt_u32("PBGPU_FST_NBUF");
    o.vl_wgf = opt_u32("PBGPU_VL_WGF");
    o.vst_shape = opt_u32("PBGPU_VST_SHAPE");
    o.vst_scan3 = opt_is("PBGPU_VST_SCAN", "3pass");
    o.xp_force = opt_is("PBGPU_XP_FORCE", "1");
    o.xp_static = !opt_is("PBGPU_XP_STATIC", "0");
    o.xp_fa64 = opt_is("PBGPU_XP_FA64", "1");
    o.xp_wgt = opt_u32("PBGPU_XP_WGT");
    o.xp_np = opt_u32("PBGPU_XP_NP");
    if (getenv("PBGPU_XP_IMG"))
        o.xp_img = opt_is("PBGPU_XP_IMG", "2") ? 2u : opt_is("PBGPU_XP_IMG", "0") ? 0u : 1u;
    o.ctr_atomic = opt_is("PBGPU_CTR_ATOMIC", "1");
    o.ctr_ring = opt_u32("PBGPU_CTR_RING");
    o.batch = !opt_is("PBGPU_BATCH", "0");
    o.batch_wgt = opt_u32("PBGPU_BATCH_WGT") == 256 ? 256u : 512u;
    o.seq_streams = !opt_is("PBGPU_SEQ_STREAMS", "0");
    o.land_spin = !opt_is("PBGPU_LAND_SPIN", "0");
    o.umem_dma = getenv("PBGPU_UMEM_DMA") != NULL;
    o.alloc_vmm = !opt_is("PBGPU_ALLOC", "malloc");
    o.vp_pages_pct = opt_u32("PBGPU_VP_PAGES_PCT");
    o.rp_per = opt_u32("PBGPU_RP_PER");
    if (o.rp_per > 32)
        o.rp_per = 0;
    if (getenv("PBGPU_LAND_DMA_MIN"))
        o.land_dma_min = (uint32_t)atoi(getenv("PBGPU_LAND_DMA_MIN"));
    if (opt_u32("PBGPU_ALLOC_CHUNK_MB"))
        o.alloc_chunk_mb = opt_u32("PBGPU_ALLOC_CHUNK_MB");
    return o;
}

int verbose()
{
    static int v = -1;
    if (v < 0)
        v = getenv("PBGPU_VERBOSE") != NULL;
    return v;
}

#define HIPCHK(call)                                                                         \
    do                                                                                       \
    {                                                                                        \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess)                                                                \
        {                                                                                    \
            if (verbose())                                                                   \
                fprintf(stderr, "[pbgpu] %s:%d %s -> %s\n", __FILE__, __LINE__, #call,       \
                        hipGetErrorString(e_));                                              \
            return PBGPU_EIO;                                                                \
        }                                                                                    \
    } while (0)

struct seq_slot
{
    bool loaded = false;
    pb_kargs K;              // template part; per-launch fields patched in pbgpu_build
    uint32_t fpi = 1;        // frames per iteration
    uint32_t min_flen = 0, max_flen = 0;
    uint2 *d_ranges = nullptr;
    pb_pl *d_pls = nullptr;
    uint32_t *d_lit_stop = nullptr;
    uint8_t *d_blob = nullptr;
    uint32_t *d_img = nullptr; // pb_ximg_kernel's pages (K.img)
    // per-workgroup counts of the launches not yet folded into the counters (pb_count): a
    // linear ring of u32 words, folded (pb_ctr_fold) when full, on reload and by pbgpu_counters
    uint32_t *d_ctr_slots = nullptr;
    uint64_t ctr_cap = 0, ctr_used = 0, ctr_pairs = 1; // words; words per record
    hipStream_t ctr_last = nullptr; // the stream of the last launch that wrote or folded the ring
    hipEvent_t ctr_ev = nullptr;
    pb_opts opt; // shape overrides, read when the sequence was loaded
    pb_plan plan; // the build kernel chosen from them (pb_make_plan)
};

struct timing_pair
{
    hipEvent_t a, b;
};

#define PB_SEQ_STREAMS 4

// What pbgpu_frames.reserved points to: the buffer's build-completion event (the landing
// stream waits on it) and the completion event of the last landing queued from it (the
// next build into the buffer waits on that, so a landing never reads frames being rebuilt)
struct frames_events
{
    hipEvent_t built = nullptr;
    hipEvent_t landed = nullptr;
    bool land_pending = false;
    hipStream_t last = nullptr; // the stream the buffer was last built on
    hipEvent_t moved = nullptr; // a build on another stream waits on this (recorded on `last`)
    // pb_vline_kernel writes 4-B offsets and region starts here; offsets[] is expanded from them
    // on first use (packed32 set until then)
    uint32_t *d_off32 = nullptr;
    unsigned long long *d_rstart = nullptr;
    // pb_vrec_kernel's records and page table (pb_vpage_kernel), allocated on first use
    uint2 *d_vrec = nullptr;
    uint2 *d_vpt = nullptr;
    bool packed32 = false;
    uint32_t wf = 0;
    // the buffer's shortest and longest frame: the building sequence's, or the uploaded frames'
    // (pbgpu_encap refuses frames it cannot encapsulate, a landing frames longer than its slot);
    // both 0 while the buffer holds no frames
    uint32_t min_len = 0, max_len = 0;
};

frames_events *frames_ev(pbgpu_frames *f)
{
    if (f->reserved == NULL)
        f->reserved = new (std::nothrow) frames_events();
    return (frames_events *)f->reserved;
}

} // namespace

struct pbgpu_ctx
{
    int device = 0;
    hipStream_t stream = nullptr;      // frame builds
    hipStream_t land_stream = nullptr; // UMEM landing: overlaps the next build (pbgpu_copy_to_umem)
    bool land_events = false;          // set by the first landing: builds then record a completion event
    pb_opts opt;                       // read at pbgpu_open: landing, stream, batch and repack options
    uint2 *d_jump = nullptr;
    uint2 *d_lcg48 = nullptr;
    uint32_t *d_orbit = nullptr; // pb_vline_kernel: LCG-orbit prefix sums (built on first use, 2 MiB)
    uint32_t *d_dlog12 = nullptr; // pb_orbit_sum's discrete log mod 2^12 (16 KiB)
    uint2 *d_lcg48i = nullptr;    // pb_vpage_kernel: L^(-48 c), c < PB_VP_NCI
    uint4 *d_m16 = nullptr;       // pb_vpage_kernel: chunk byte masks by plo + phi
    uint32_t orbit_tot = 0;
    unsigned long long *d_counters = nullptr; // [PB_MAX_SEQUENCES][PB_CTR_SHARDS][PB_CTR_STRIDE]
    // the shard sums {frames, bytes} per sequence, written by pb_ctr_read into mapped pinned host
    // memory (h_ctr_sum; d_ctr_sum its device address)
    unsigned long long *h_ctr_sum = nullptr, *d_ctr_sum = nullptr;
    unsigned long long *d_img_ctr = nullptr; // counters of the load-time pb_ximg_kernel page builds (never read)
    // pbgpu_verify and pbgpu_verify_wire (run_check): the workgroups' records, the folded result in
    // mapped pinned host memory (written by pb_vfold_kernel, as h_ctr_sum is by pb_ctr_read) and the
    // code bytes; records and codes grown on demand
    uint32_t *d_vfy_rec = nullptr;
    uint64_t vfy_rec_cap = 0; // bytes
    unsigned long long *h_vres = nullptr, *d_vres = nullptr; // PB_CHECK_RES words
    uint8_t *d_vcodes = nullptr;
    uint64_t vcodes_cap = 0;
    // pbgpu_fragment and pbgpu_segment: the count pass's scratch (result words, one or two row
    // sums, K and H per source frame), the map (one entry per output record) and segment's slice
    // sums of the output records, each grown on demand.  The two calls share them: every call that
    // queues work on them synchronises the stream before it returns, so none finds them in use.
    // The two count layouts differ, hence that capacity in bytes.
    uint8_t *d_cut_cnt = nullptr;
    uint64_t cut_cnt_cap = 0; // bytes
    uint64_t *d_cut_map = nullptr;
    uint64_t cut_map_cap = 0; // output records
    uint32_t *d_cut_psum = nullptr;
    uint64_t cut_psum_cap = 0; // output records
    unsigned long long *d_sp_res = nullptr; // pbgpu_stamp: the result words
    unsigned long long *d_xl_res = nullptr; // pbgpu_xlat46: the classify pass's result words
    seq_slot seqs[PB_MAX_SEQUENCES];
    std::vector<timing_pair> pending;
    std::vector<timing_pair> pool;
    int timing_mode = PBGPU_TIMING_LAUNCH;
    timing_pair span = {nullptr, nullptr}; // PBGPU_TIMING_SPAN: first-launch / call events
    uint32_t span_n = 0;                    // launches in the open span (0: none open)
    // PBGPU_TIMING_SPAN: the builds of sequence i run on seq_stream[i % PB_SEQ_STREAMS], so the
    // kernels of different sequences overlap (as the reference's non-blocking sequences run
    // their threads side by side, sequence.c:741-765); every other call first joins them
    // into `stream` (one event per stream that built since the last join)
    // counts of a slot's earlier sequences (folded in when the slot is loaded again)
    uint64_t ctr_base[PB_MAX_SEQUENCES][2] = {};
    hipStream_t seq_stream[PB_SEQ_STREAMS] = {};
    hipEvent_t seq_join[PB_SEQ_STREAMS] = {};
    bool seq_dirty[PB_SEQ_STREAMS] = {};
    bool seq_in_span[PB_SEQ_STREAMS] = {}; // has waited on span.a since it was recorded
    uint8_t *h_stage = nullptr;
    uint16_t *d_lens = nullptr; // landing: frame lengths of the mapped scatter (device), a ring
    uint16_t *h_lens = nullptr; // ... and their pinned host copy
    uint32_t lens_cap = 0;
    uint32_t lens_head = 0;     // next free entry of the ring
    size_t h_stage_bytes = 0;
    struct land_op
    {
        hipEvent_t ev;
        uint16_t *lens_out;
        uint32_t n;
        uint32_t lens_off; // variable length: entries [lens_off, lens_off + n) of the lens ring
        uint32_t fixed_len;
    };
    std::deque<land_op> landings;      // queued, not yet waited for (FIFO)
    std::vector<hipEvent_t> land_pool; // recycled landing events
    struct reg
    {
        uint8_t *host;
        size_t bytes;
        uint8_t *dev;
    };
    std::vector<reg> regs; // pbgpu_host_register'ed ranges and their device addresses
};

namespace
{

// jump[j + PB_JNEG] = L^(3(j+1)) as (A, C), j = -PB_JNEG ..
std::vector<uint2> make_jump_table()
{
    const uint32_t a = PB_LCG_A, c = PB_LCG_C;
    uint32_t ainv = a; // Newton: a * ainv == 1 mod 2^32
    for (int i = 0; i < 5; ++i)
        ainv *= 2u - a * ainv;
    // inverse step y -> ainv * (y - c)
    const uint32_t ia = ainv, ic = (uint32_t)(0u - ainv * c);
    // first entry: j = -PB_JNEG -> L^(3(1 - PB_JNEG))
    uint32_t A = 1, C = 0;
    for (int i = 0; i < 3 * (PB_JNEG - 1); ++i)
    {
        A = ia * A;
        C = ia * C + ic;
    }
    const uint32_t a3 = a * a * a, c3 = c * (a * a + a + 1u);
    std::vector<uint2> t(PB_JUMP_N);
    for (int j = 0; j < PB_JUMP_N; ++j)
    {
        t[j] = make_uint2(A, C);
        A = a3 * A;
        C = a3 * C + c3;
    }
    return t;
}

// pb_vline_kernel's payload sums (pbgpu_kernels.hip, pb_orbit_sum): M = L^3 mod 2^24 walks one
// orbit of all 2^24 states from 0 (full period: c odd, a = 1 mod 4); entry t holds the sums of
// the bytes (bits 16-23) at the even and the odd positions before t << PB_ORB_SH, mod 0xFFFF,
// as two u16.
std::vector<uint32_t> make_orbit_table(uint32_t *total)
{
    const uint32_t m = 0xFFFFFFu;
    const uint32_t a3 = (PB_LCG_A * PB_LCG_A * PB_LCG_A) & m, c3 = (PB_LCG_C * (PB_LCG_A * PB_LCG_A + PB_LCG_A + 1u)) & m;
    std::vector<uint32_t> t((1u << (24 - PB_ORB_SH)) + 1);
    uint32_t y = 0, pe = 0, po = 0;
    for (uint32_t k = 0; k < (1u << 24); ++k)
    {
        if ((k & ((1u << PB_ORB_SH) - 1u)) == 0)
            t[k >> PB_ORB_SH] = pe | (po << 16);
        const uint32_t b = (y >> 16) & 0xFFu;
        if (k & 1u)
            po = (po + b) % 0xFFFFu;
        else
            pe = (pe + b) % 0xFFFFu;
        y = (a3 * y + c3) & m;
    }
    t[1u << (24 - PB_ORB_SH)] = pe | (po << 16);
    *total = pe; // the even and odd totals are equal (each byte value 2^15 times per parity)
    return t;
}

template <typename T>
int upload(T **dptr, const T *src, size_t n)
{
    if (*dptr)
        (void)hipFree(*dptr);
    *dptr = nullptr;
    if (n == 0)
    {
        // an empty table is a zeroed 256-B allocation, never a null device pointer
        HIPCHK(hipMalloc((void **)dptr, 256));
        HIPCHK(hipMemset(*dptr, 0, 256));
        return PBGPU_OK;
    }
    HIPCHK(hipMalloc((void **)dptr, n * sizeof(T)));
    HIPCHK(hipMemcpy(*dptr, src, n * sizeof(T), hipMemcpyHostToDevice));
    return PBGPU_OK;
}

void slot_free(seq_slot &s)
{
    if (s.d_ranges)
        (void)hipFree(s.d_ranges);
    if (s.d_pls)
        (void)hipFree(s.d_pls);
    if (s.d_lit_stop)
        (void)hipFree(s.d_lit_stop);
    if (s.d_blob)
        (void)hipFree(s.d_blob);
    if (s.d_img)
        (void)hipFree(s.d_img);
    s = seq_slot();
}

} // namespace

extern "C" {

const char *pbgpu_strerror(int err)
{
    switch (err)
    {
    case PBGPU_OK: return "ok";
    case PBGPU_ENOENT: return "sequence not loaded";
    case PBGPU_EIO: return "HIP runtime error";
    case PBGPU_ENOMEM: return "out of memory";
    case PBGPU_EINVAL: return "invalid argument or sequence";
    case PBGPU_ENOSPC: return "frames buffer too small";
    case PBGPU_ENODEV: return "no such GPU";
    case PBGPU_ENOTSUP: return "sequence not supported on the GPU path";
    default: return "unknown error";
    }
}

int pbgpu_device_count(int *n)
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess)
        c = 0;
    *n = c;
    return PBGPU_OK;
}

// The sequence builds issued since the last join, ordered before what follows on ctx->stream.
static int join_builds(pbgpu_ctx *ctx)
{
    for (int i = 0; i < PB_SEQ_STREAMS; ++i)
        if (ctx->seq_dirty[i])
        {
            if (ctx->seq_join[i] == nullptr)
                HIPCHK(hipEventCreateWithFlags(&ctx->seq_join[i], hipEventDisableTiming));
            HIPCHK(hipEventRecord(ctx->seq_join[i], ctx->seq_stream[i]));
            HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->seq_join[i], 0));
            ctx->seq_dirty[i] = false;
        }
    return PBGPU_OK;
}

static void slot_counts(const pbgpu_ctx *ctx, const unsigned long long *sum, int i, uint64_t *p, uint64_t *b);
static int read_counter_sums(pbgpu_ctx *ctx, int first, int n_seq);

// Launches that touch a sequence's count ring (its builds and folds) run in order, whatever
// stream each is issued on: the next one waits for the previous one's stream.
static int ctr_order(seq_slot &S, hipStream_t st)
{
    if (S.ctr_last && S.ctr_last != st)
    {
        if (S.ctr_ev == nullptr)
            HIPCHK(hipEventCreateWithFlags(&S.ctr_ev, hipEventDisableTiming));
        HIPCHK(hipEventRecord(S.ctr_ev, S.ctr_last));
        HIPCHK(hipStreamWaitEvent(st, S.ctr_ev, 0));
    }
    S.ctr_last = st;
    return PBGPU_OK;
}

// Adds the records of slot i's launches since the last fold into its counters (on st).
static int ctr_fold(pbgpu_ctx *ctx, int i, hipStream_t st)
{
    seq_slot &S = ctx->seqs[i];
    if (S.ctr_used == 0)
        return PBGPU_OK;
    const int rc = ctr_order(S, st);
    if (rc != PBGPU_OK)
        return rc;
    HIPCHK(pbk_launch_ctr_fold(S.d_ctr_slots, S.ctr_used / S.ctr_pairs, (uint32_t)S.ctr_pairs,
                               ctx->d_counters + PB_CTR_WORDS * (size_t)i, st));
    S.ctr_used = 0;
    return PBGPU_OK;
}

static void ctr_free(seq_slot &S)
{
    if (S.d_ctr_slots)
        (void)hipFree(S.d_ctr_slots);
    if (S.ctr_ev)
        (void)hipEventDestroy(S.ctr_ev);
    S.d_ctr_slots = nullptr;
    S.ctr_ev = nullptr;
    S.ctr_cap = S.ctr_used = 0;
    S.ctr_last = nullptr;
}

#define PB_CTR_RING_WORDS (8ull << 20) // count ring per sequence: 32 MiB, 64 launches of 2^25 64-B frames

#define PB_JOIN(ctx)                         \
    do                                       \
    {                                        \
        const int jrc_ = join_builds(ctx);   \
        if (jrc_ != PBGPU_OK)                \
            return jrc_;                     \
    } while (0)

int pbgpu_open(int device, pbgpu_ctx **out)
{
    if (out == NULL)
        return PBGPU_EINVAL;
    *out = NULL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n)
        return PBGPU_ENODEV;
    HIPCHK(hipSetDevice(device));
    pbgpu_ctx *ctx = new pbgpu_ctx();
    ctx->device = device;
    ctx->opt = read_opts();
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->land_stream, hipStreamNonBlocking) != hipSuccess)
    {
        if (ctx->stream)
            (void)hipStreamDestroy(ctx->stream);
        delete ctx;
        return PBGPU_EIO;
    }
    std::vector<uint2> jt = make_jump_table();
    std::vector<uint2> l48(PB_LCG48_N);
    {
        const uint32_t a3 = PB_LCG_A * PB_LCG_A * PB_LCG_A, c3 = PB_LCG_C * (PB_LCG_A * PB_LCG_A + PB_LCG_A + 1u);
        uint32_t A16 = 1, C16 = 0; // L^48 = (L^3)^16
        for (int i = 0; i < 16; ++i)
            C16 = a3 * C16 + c3, A16 = a3 * A16;
        uint32_t A = 1, C = 0;
        for (int m = 0; m < PB_LCG48_N; ++m)
        {
            l48[m] = make_uint2(A, C);
            A = A16 * A;
            C = A16 * C + C16;
        }
    }
    // L^(-48 c) (pb_vpage_kernel) and the discrete log of M = L^3 mod 2^12 (pb_orbit_sum)
    std::vector<uint2> l48i(PB_VP_NCI);
    std::vector<uint32_t> dlog12(4096);
    std::vector<uint4> m16(PB_VL_NMASK);
    for (int j = 0; j < PB_VL_NMASK; ++j) // bytes [lo, hi) of a 16-B chunk: j = lo + hi
    {
        const int lo = j > 16 ? j - 16 : 0, hi = j > 16 ? 16 : j;
        uint32_t w[4];
        for (int t = 0; t < 4; ++t)
        {
            w[t] = 0;
            for (int b = 0; b < 4; ++b)
                if (4 * t + b >= lo && 4 * t + b < hi)
                    w[t] |= 0xFFu << (8 * b);
        }
        m16[j] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    {
        uint32_t ai = PB_LCG_A; // PB_LCG_A^-1 mod 2^32 (Newton)
        for (int i = 0; i < 5; ++i)
            ai *= 2u - PB_LCG_A * ai;
        const uint32_t ci = 0u - ai * PB_LCG_C; // L^-1(x) = ai x + ci
        uint32_t A48 = 1, C48 = 0;
        for (int i = 0; i < 48; ++i)
            C48 = ai * C48 + ci, A48 = ai * A48;
        uint32_t A = 1, C = 0;
        for (uint32_t m = 0; m < PB_VP_NCI; ++m)
        {
            l48i[m] = make_uint2(A, C);
            A = A48 * A;
            C = A48 * C + C48;
        }
        const uint32_t a3 = (PB_LCG_A * PB_LCG_A * PB_LCG_A) & 0xFFFFFFu;
        const uint32_t c3 = (PB_LCG_C * (PB_LCG_A * PB_LCG_A + PB_LCG_A + 1u)) & 0xFFFFFFu;
        uint32_t x = 0;
        for (uint32_t j = 0; j < 4096; ++j)
        {
            dlog12[x & 0xFFFu] = j | (x & 0xFFF000u);
            x = (a3 * x + c3) & 0xFFFFFFu;
        }
    }
    if (upload(&ctx->d_jump, jt.data(), jt.size()) != PBGPU_OK || upload(&ctx->d_lcg48, l48.data(), l48.size()) != PBGPU_OK ||
        upload(&ctx->d_lcg48i, l48i.data(), l48i.size()) != PBGPU_OK ||
        upload(&ctx->d_dlog12, dlog12.data(), dlog12.size()) != PBGPU_OK ||
        upload(&ctx->d_m16, m16.data(), m16.size()) != PBGPU_OK ||
        hipMalloc((void **)&ctx->d_counters, PB_CTR_BYTES) != hipSuccess ||
        hipMemset(ctx->d_counters, 0, PB_CTR_BYTES) != hipSuccess ||
        hipHostMalloc((void **)&ctx->h_ctr_sum, 2 * sizeof(unsigned long long) * PB_MAX_SEQUENCES,
                      hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void **)&ctx->d_ctr_sum, ctx->h_ctr_sum, 0) != hipSuccess)
    {
        pbgpu_close(ctx);
        return PBGPU_EIO;
    }
    *out = ctx;
    return PBGPU_OK;
}

void pbgpu_close(pbgpu_ctx *ctx)
{
    if (ctx == NULL)
        return;
    (void)hipSetDevice(ctx->device);
    for (int i = 0; i < PB_SEQ_STREAMS; ++i)
        if (ctx->seq_stream[i])
            (void)hipStreamSynchronize(ctx->seq_stream[i]);
    if (ctx->stream)
        (void)hipStreamSynchronize(ctx->stream);
    if (ctx->land_stream)
        (void)hipStreamSynchronize(ctx->land_stream);
    (void)pbgpu_land_wait(ctx, 0);
    for (hipEvent_t e : ctx->land_pool)
        (void)hipEventDestroy(e);
    for (auto &s : ctx->seqs)
    {
        ctr_free(s);
        slot_free(s);
    }
    for (auto &p : ctx->pending)
        ctx->pool.push_back(p);
    for (auto &p : ctx->pool)
    {
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    if (ctx->span.a)
    {
        (void)hipEventDestroy(ctx->span.a);
        (void)hipEventDestroy(ctx->span.b);
    }
    if (ctx->d_jump)
        (void)hipFree(ctx->d_jump);
    if (ctx->d_lcg48)
        (void)hipFree(ctx->d_lcg48);
    if (ctx->d_orbit)
        (void)hipFree(ctx->d_orbit);
    if (ctx->d_dlog12)
        (void)hipFree(ctx->d_dlog12);
    if (ctx->d_lcg48i)
        (void)hipFree(ctx->d_lcg48i);
    if (ctx->d_m16)
        (void)hipFree(ctx->d_m16);
    if (ctx->d_counters)
        (void)hipFree(ctx->d_counters);
    if (ctx->h_ctr_sum)
        (void)hipHostFree(ctx->h_ctr_sum);
    if (ctx->d_img_ctr)
        (void)hipFree(ctx->d_img_ctr);
    if (ctx->d_vfy_rec)
        (void)hipFree(ctx->d_vfy_rec);
    if (ctx->h_vres)
        (void)hipHostFree(ctx->h_vres);
    if (ctx->d_vcodes)
        (void)hipFree(ctx->d_vcodes);
    if (ctx->d_cut_cnt)
        (void)hipFree(ctx->d_cut_cnt);
    if (ctx->d_cut_map)
        (void)hipFree(ctx->d_cut_map);
    if (ctx->d_cut_psum)
        (void)hipFree(ctx->d_cut_psum);
    if (ctx->d_sp_res)
        (void)hipFree(ctx->d_sp_res);
    if (ctx->d_xl_res)
        (void)hipFree(ctx->d_xl_res);
    if (ctx->h_stage)
        (void)hipHostFree(ctx->h_stage);
    if (ctx->d_lens)
        (void)hipFree(ctx->d_lens);
    if (ctx->h_lens)
        (void)hipHostFree(ctx->h_lens);
    for (int i = 0; i < PB_SEQ_STREAMS; ++i)
    {
        if (ctx->seq_join[i])
            (void)hipEventDestroy(ctx->seq_join[i]);
        if (ctx->seq_stream[i])
            (void)hipStreamDestroy(ctx->seq_stream[i]);
    }
    if (ctx->stream)
        (void)hipStreamDestroy(ctx->stream);
    if (ctx->land_stream)
        (void)hipStreamDestroy(ctx->land_stream);
    delete ctx;
}

// the orbit prefix-sum table (pb_orbit_sum, pb_vline_kernel): the 2^24-step
// walk runs once per process; each context uploads the result
static int upload_orbit(pbgpu_ctx *ctx)
{
    if (ctx->d_orbit != nullptr)
        return PBGPU_OK;
    static std::once_flag once;
    static std::vector<uint32_t> orb;
    static uint32_t tot = 0;
    std::call_once(once, [] { orb = make_orbit_table(&tot); });
    const int rc = upload(&ctx->d_orbit, orb.data(), orb.size());
    if (rc != PBGPU_OK)
        return rc;
    ctx->orbit_tot = tot;
    return PBGPU_OK;
}

// pb_ximg_kernel's image (pb_plan.img_np): the stream's first img_np pages, built once, here, with
// pb_xpage_kernel (counted into a scratch counter array, not the sequence's)
static int build_image(pbgpu_ctx *ctx, seq_slot &S, pb_kargs &K, const pb_plan &P, const pb_opts &O)
{
    const uint32_t np = P.img_np;
    const uint64_t bytes = (uint64_t)np * PB_XPG;
    HIPCHK(hipMalloc((void **)&S.d_img, bytes));
    if (ctx->d_img_ctr == nullptr)
    {
        HIPCHK(hipMalloc((void **)&ctx->d_img_ctr, PB_CTR_WORDS * sizeof(unsigned long long)));
        HIPCHK(hipMemset(ctx->d_img_ctr, 0, PB_CTR_WORDS * sizeof(unsigned long long)));
    }
    pb_kargs K2 = K;
    K2.first_iter = 0;
    K2.n_frames = (bytes + K.fixed_len - 1) / K.fixed_len + 1;
    K2.total_bytes = bytes;
    K2.out = (uint8_t *)S.d_img;
    K2.counters = ctx->d_img_ctr;
    K2.ctr_slots = nullptr;
    pb_plan P2 = P; // the same pages without an image: pb_xpage_kernel
    P2.kern = PB_KERN_XPAGE;
    P2.img_solo = false;
    const pb_kern kern = pb_plan_launch(P2, O, 0, K2);
    K2.xp_fa_hi = 0;
    HIPCHK(pbk_launch_build(&K2, kern, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    K.img = S.d_img;
    K.img_np = np;
    K.img_div = make_div(np);
    K.img_solo = P.img_solo;
    return PBGPU_OK;
}

// sequence_t -> GPU template: thread_hdl() prologue, sequence.c:66-374 (pb_compile), the build
// kernel and its shape (pb_make_plan), then the uploads and the device work the plan asks for.
int pbgpu_load_sequence(pbgpu_ctx *ctx, uint16_t seq_idx, const pb_sequence_t *seq, const uint8_t *src_mac,
                        const uint8_t *dst_mac, const pb_rules_t *rules, uint64_t seed_base)
{
    if (ctx == NULL || seq == NULL || seq_idx >= PB_MAX_SEQUENCES)
        return PBGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx);
    {
        const int frc = ctr_fold(ctx, seq_idx, ctx->stream); // the old sequence's pending counts
        if (frc != PBGPU_OK)
            return frc;
    }
    HIPCHK(hipStreamSynchronize(ctx->stream)); // no build still reads the slot's tables
    seq_slot &S = ctx->seqs[seq_idx];
    if (S.loaded) // the slot's counts so far (their frames follow the old sequence's length)
    {
        const int rrc = read_counter_sums(ctx, seq_idx, 1);
        if (rrc != PBGPU_OK)
            return rrc;
        uint64_t p = 0, b = 0;
        slot_counts(ctx, ctx->h_ctr_sum, seq_idx, &p, &b);
        ctx->ctr_base[seq_idx][0] = p;
        ctx->ctr_base[seq_idx][1] = b;
        HIPCHK(hipMemset(ctx->d_counters + PB_CTR_WORDS * seq_idx, 0, PB_CTR_WORDS * sizeof(unsigned long long)));
    }
    {
        // the count ring (empty now) stays with the slot
        uint32_t *ring = S.d_ctr_slots;
        const uint64_t cap = S.ctr_cap;
        hipEvent_t ev = S.ctr_ev;
        slot_free(S);
        S.d_ctr_slots = ring;
        S.ctr_cap = cap;
        S.ctr_ev = ev;
        S.ctr_last = ctx->stream;
    }

    const pb_opts O = read_opts();
    pb_compiled C;
    int rc = pb_compile(seq_idx, seq, src_mac, dst_mac, rules, seed_base, &C);
    if (rc != PBGPU_OK)
        return rc;
    const pb_plan P = pb_make_plan(C, O);
    pb_kargs &K = C.K;
    if (P.orbit) // (first, as the allocations have always been ordered)
    {
        if ((rc = upload_orbit(ctx)) != PBGPU_OK)
            return rc;
        K.orbit = ctx->d_orbit;
        K.orbit_tot = ctx->orbit_tot;
    }
    if ((rc = upload(&S.d_ranges, C.ranges.data(), C.ranges.size())) != PBGPU_OK)
        return rc;
    if ((rc = upload(&S.d_pls, C.pls.data(), C.pls.size())) != PBGPU_OK)
        return rc;
    if ((rc = upload(&S.d_lit_stop, C.lit_stop.data(), C.lit_stop.size())) != PBGPU_OK)
        return rc;
    if ((rc = upload(&S.d_blob, C.blob.data(), C.blob.size())) != PBGPU_OK)
        return rc;
    K.ranges = S.d_ranges;
    K.pls = S.d_pls;
    K.lit_stop = S.d_lit_stop;
    K.blob = S.d_blob;
    K.jump = ctx->d_jump;
    K.lcg48 = ctx->d_lcg48;
    K.lcg48i = ctx->d_lcg48i;
    K.m16 = ctx->d_m16;
    K.dlog12 = ctx->d_dlog12;
    K.counters = ctx->d_counters + PB_CTR_WORDS * seq_idx;
    if (P.img_np && (rc = build_image(ctx, S, K, P, O)) != PBGPU_OK)
        return rc;
    S.K = K;
    S.fpi = C.fpi;
    S.min_flen = C.min_flen;
    S.max_flen = C.max_flen;
    S.opt = O;
    S.plan = P;
    S.loaded = true;
    return PBGPU_OK;
}

int pbgpu_build_size(pbgpu_ctx *ctx, uint16_t seq_idx, uint64_t n_iter, uint64_t *max_frames, uint64_t *max_bytes)
{
    if (ctx == NULL || seq_idx >= PB_MAX_SEQUENCES)
        return PBGPU_EINVAL;
    const seq_slot &S = ctx->seqs[seq_idx];
    if (!S.loaded)
        return PBGPU_ENOENT;
    const uint64_t nf = n_iter * S.fpi;
    if (max_frames)
        *max_frames = nf;
    if (max_bytes)
        *max_bytes = ((nf * S.max_flen + 15) & ~15ull) + 16;
    return PBGPU_OK;
}

// Device memory of frame buffers.  A buffer of >= PB_VMM_MIN bytes is built from physical chunks
// (hipMemCreate, alloc_chunk_mb each) mapped in creation order into one reserved VA range,
// instead of one hipMalloc: the region kernels' slow mode follows the buffer's
// physical placement; in fresh processes hipMalloc drew it 3 times in 4 (pb_fstage_kernel 8.47 ms,
// pb_vline_kernel 5.06-5.08) and chunk-mapped buffers 2 times in 40 (7.24-7.30 / 4.36-4.40 otherwise;
// profiles/r05/ab/alloc_ab2.jsonl, vmm*.jsonl, lenpass_ab.log).  Falls back to hipMalloc when the virtual-memory
// calls fail.  The blocks are kept in a process-wide table, so fb_free needs no context; callers
// free only after the work that uses a block has completed (pbgpu_frames_free synchronises first).
#define PB_VMM_MIN (64ull << 20)

namespace
{
struct vmm_block
{
    size_t bytes;
    int device; // the GPU whose memory the chunks are (fb_free synchronises it before unmapping)
    std::vector<std::pair<hipMemGenericAllocationHandle_t, size_t>> chunks; // handle, size
};
std::mutex g_vmm_mu;
std::unordered_map<void *, vmm_block> g_vmm;

void vmm_release(void *va, vmm_block &B)
{
    size_t off = 0;
    for (auto &c : B.chunks)
    {
        (void)hipMemUnmap((char *)va + off, c.second);
        (void)hipMemRelease(c.first);
        off += c.second;
    }
    (void)hipMemAddressFree(va, B.bytes);
}
} // namespace

static hipError_t fb_alloc(const pbgpu_ctx *ctx, void **p, size_t bytes)
{
    *p = nullptr;
    const size_t chunk = (size_t)ctx->opt.alloc_chunk_mb << 20;
    if (!ctx->opt.alloc_vmm || bytes < PB_VMM_MIN || chunk == 0)
        return hipMalloc(p, bytes);
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = ctx->device;
    size_t gran = 0;
    if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum) != hipSuccess || gran == 0 ||
        chunk % gran)
    {
        if (verbose())
            fprintf(stderr, "pbgpu: allocation granularity %zu B does not divide %zu-B chunks; hipMalloc\n", gran, chunk);
        (void)hipGetLastError();
        return hipMalloc(p, bytes);
    }
    vmm_block B;
    B.bytes = (bytes + gran - 1) / gran * gran;
    B.device = ctx->device;
    void *va = nullptr;
    if (hipMemAddressReserve(&va, B.bytes, chunk, nullptr, 0) != hipSuccess)
    {
        if (verbose())
            fprintf(stderr, "pbgpu: no %zu-B address reservation; hipMalloc\n", B.bytes);
        (void)hipGetLastError();
        return hipMalloc(p, bytes);
    }
    bool ok = true;
    for (size_t off = 0; off < B.bytes && ok; off += chunk)
    {
        const size_t sz = B.bytes - off < chunk ? B.bytes - off : chunk;
        hipMemGenericAllocationHandle_t h;
        if (hipMemCreate(&h, sz, &prop, 0) != hipSuccess)
        {
            ok = false;
            break;
        }
        if (hipMemMap((char *)va + off, sz, 0, h, 0) != hipSuccess)
        {
            (void)hipMemRelease(h);
            ok = false;
            break;
        }
        B.chunks.push_back({h, sz});
    }
    hipMemAccessDesc acc = {};
    acc.location = prop.location;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    if (ok && hipMemSetAccess(va, B.bytes, &acc, 1) != hipSuccess)
        ok = false;
    if (!ok)
    {
        if (verbose())
            fprintf(stderr, "pbgpu: chunk mapping failed after %zu chunks (%s); hipMalloc\n", B.chunks.size(),
                    hipGetErrorString(hipGetLastError()));
        vmm_release(va, B); // the chunks mapped so far, then the reservation
        (void)hipGetLastError();
        return hipMalloc(p, bytes);
    }
    if (verbose())
        fprintf(stderr, "pbgpu: %zu-B buffer at %p: %zu physical chunks of <= %zu B mapped in order\n", B.bytes, va,
                B.chunks.size(), chunk);
    {
        std::lock_guard<std::mutex> lk(g_vmm_mu);
        g_vmm.emplace(va, std::move(B));
    }
    *p = va;
    return hipSuccess;
}

// hipFree waits for the device; unmapping does not, so a chunk-mapped block first waits for every
// stream of its device (work queued on a caller's stream, or a free without a context, must not
// find its pages gone: a GPU page fault instead of hipFree's implicit wait)
static void fb_free(void *p)
{
    if (p == nullptr)
        return;
    {
        std::lock_guard<std::mutex> lk(g_vmm_mu);
        auto it = g_vmm.find(p);
        if (it != g_vmm.end())
        {
            int cur = -1;
            (void)hipGetDevice(&cur);
            if (hipSetDevice(it->second.device) == hipSuccess)
                (void)hipDeviceSynchronize();
            if (cur >= 0)
                (void)hipSetDevice(cur);
            vmm_release(p, it->second);
            g_vmm.erase(it);
            return;
        }
    }
    (void)hipFree(p);
}

int pbgpu_frames_alloc(pbgpu_ctx *ctx, uint64_t capacity_frames, uint64_t capacity_bytes, pbgpu_frames **out)
{
    if (ctx == NULL || out == NULL)
        return PBGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    pbgpu_frames *f = (pbgpu_frames *)calloc(1, sizeof *f);
    if (f == NULL)
        return PBGPU_ENOMEM;
    capacity_bytes = (capacity_bytes + 15) & ~15ull;
    // +64 B: word-granular readers (UMEM scatter) may touch a few bytes past the last frame
    if (fb_alloc(ctx, (void **)&f->data, capacity_bytes + 64) != hipSuccess ||
        fb_alloc(ctx, (void **)&f->offsets, (capacity_frames + 1) * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc((void **)&f->scan_tmp, scan_tmp_bytes(capacity_frames)) != hipSuccess)
    {
        pbgpu_frames_free(ctx, f);
        return PBGPU_ENOMEM;
    }
    f->capacity_frames = capacity_frames;
    f->capacity_bytes = capacity_bytes;
    f->total_bytes = 0;
    *out = f;
    return PBGPU_OK;
}

void pbgpu_frames_free(pbgpu_ctx *ctx, pbgpu_frames *f)
{
    if (f == NULL)
        return;
    if (ctx)
    {
        (void)hipSetDevice(ctx->device);
        (void)pbgpu_land_wait(ctx, 0);
        (void)join_builds(ctx);
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamSynchronize(ctx->land_stream);
    }
    if (f->reserved)
    {
        frames_events *fe = (frames_events *)f->reserved;
        if (fe->built)
            (void)hipEventDestroy(fe->built);
        if (fe->moved)
            (void)hipEventDestroy(fe->moved);
        if (fe->d_off32)
            fb_free(fe->d_off32);
        if (fe->d_rstart)
            (void)hipFree(fe->d_rstart);
        if (fe->d_vrec)
            fb_free(fe->d_vrec);
        if (fe->d_vpt)
            (void)hipFree(fe->d_vpt);
        if (fe->landed)
            (void)hipEventDestroy(fe->landed);
        delete fe;
    }
    if (f->data)
        fb_free(f->data);
    if (f->offsets)
        fb_free(f->offsets);
    if (f->scan_tmp)
        (void)hipFree(f->scan_tmp);
    free(f);
}

static int timed_pair(pbgpu_ctx *ctx, timing_pair *p)
{
    if (!ctx->pool.empty())
    {
        *p = ctx->pool.back();
        ctx->pool.pop_back();
        return PBGPU_OK;
    }
    HIPCHK(hipEventCreate(&p->a));
    HIPCHK(hipEventCreate(&p->b));
    return PBGPU_OK;
}

// The frames' build-completion event (kept in pbgpu_frames.reserved): the
// landing stream waits on it, so landing one buffer overlaps building the next.
static int mark_built(pbgpu_ctx *ctx, pbgpu_frames *out, hipStream_t st)
{
    // only for callers that land frames: an event record per launch would cost a
    // release between back-to-back builds that are never landed (bench)
    if (!ctx->land_events)
        return PBGPU_OK;
    frames_events *fe = frames_ev(out);
    if (fe == NULL)
        return PBGPU_ENOMEM;
    if (fe->built == nullptr)
        HIPCHK(hipEventCreateWithFlags(&fe->built, hipEventDisableTiming));
    HIPCHK(hipEventRecord(fe->built, st));
    return PBGPU_OK;
}

// offsets[] of a build that wrote 4-B offsets, expanded on the context's stream (after the
// sequence streams are joined); later builds of the buffer follow it (fe->last)
static int materialize_offsets(pbgpu_ctx *ctx, const pbgpu_frames *f)
{
    frames_events *fe = (frames_events *)f->reserved;
    if (fe == NULL || !fe->packed32)
        return PBGPU_OK;
    PB_JOIN(ctx);
    HIPCHK(pbk_launch_expand_offsets(fe->d_off32, fe->d_rstart, fe->wf, f->n_frames, f->offsets, ctx->stream));
    fe->packed32 = false;
    fe->last = ctx->stream;
    if (fe->built) // a landing waits for the expansion too
        HIPCHK(hipEventRecord(fe->built, ctx->stream));
    return PBGPU_OK;
}

// ---- shared by the builds, the upload, verify and the repackers (pcap pack, encap, fragment) ----

#define PBCHK(call)             \
    do                          \
    {                           \
        const int r_ = (call);  \
        if (r_ != PBGPU_OK)     \
            return r_;          \
    } while (0)

// A timed stretch of the context's stream: begin takes a pair and records its start, stop records
// its end, ms waits for the stream and reads the time. The pair is back in the pool from the
// start, whatever follows: it is used only until the call that took it returns.
static int timed_begin(pbgpu_ctx *ctx, timing_pair *tp)
{
    PBCHK(timed_pair(ctx, tp));
    ctx->pool.push_back(*tp);
    HIPCHK(hipEventRecord(tp->a, ctx->stream));
    return PBGPU_OK;
}

static int timed_stop(pbgpu_ctx *ctx, const timing_pair &tp)
{
    HIPCHK(hipEventRecord(tp.b, ctx->stream));
    return PBGPU_OK;
}

static int timed_ms(pbgpu_ctx *ctx, const timing_pair &tp, float *ms)
{
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipEventElapsedTime(ms, tp.a, tp.b));
    return PBGPU_OK;
}

// A grow-only device scratch buffer: at least `need` units (`bytes` for them) after this; no
// buffer and no capacity when the allocation fails.
static int scratch_reserve(void **ptr, uint64_t *cap, uint64_t need, size_t bytes)
{
    if (need <= *cap)
        return PBGPU_OK;
    if (*ptr)
        (void)hipFree(*ptr);
    *ptr = nullptr;
    *cap = 0;
    if (hipMalloc(ptr, bytes) != hipSuccess)
        return PBGPU_ENOMEM;
    *cap = need;
    return PBGPU_OK;
}

// Pages per workgroup of a launch over 4-KiB pages: they grow with the launch (at least 16384
// workgroups in a large one, 32 pages at the most), or are `forced` (1 to 32; 0: by the rule), and
// grow further where the grid would pass 2^24.
static int page_grid(uint64_t npages, uint32_t forced, uint32_t *per_out, uint32_t *grid)
{
    uint64_t per = npages / 16384;
    per = per < 1 ? 1 : (per > 32 ? 32 : per);
    if (forced)
        per = forced;
    if ((npages + per - 1) / per > (1ull << 24))
        per = (npages + (1ull << 24) - 1) >> 24;
    if (per > 0xFFFFFFFFull)
        return PBGPU_EINVAL;
    *per_out = (uint32_t)per;
    *grid = (uint32_t)((npages + per - 1) / per);
    return PBGPU_OK;
}

int pbgpu_page_grid(pbgpu_ctx *ctx, uint64_t npages, uint32_t *per, uint32_t *grid)
{
    if (ctx == NULL || per == NULL || grid == NULL)
        return PBGPU_EINVAL;
    return page_grid(npages, ctx->opt.rp_per, per, grid);
}

// The device computes (first_index + j) * step_ps and t0_ns + that / 1000 for j < n in 64 bits:
// whether the last of them fits
static bool stamps_fit(uint64_t first_index, uint64_t n, uint64_t step_ps, uint64_t t0_ns)
{
    if (n == 0)
        return true;
    if (first_index > UINT64_MAX - (n - 1))
        return false;
    const uint64_t last = first_index + (n - 1);
    if (step_ps && last > UINT64_MAX / step_ps)
        return false;
    return last * step_ps / 1000u <= UINT64_MAX - t0_ns;
}

// A byte template as little-endian dwords
static void pack_le32(uint32_t *dw, const uint8_t *t, uint32_t ndw)
{
    for (uint32_t i = 0; i < ndw; ++i)
        dw[i] = (uint32_t)t[4 * i] | ((uint32_t)t[4 * i + 1] << 8) | ((uint32_t)t[4 * i + 2] << 16) |
                ((uint32_t)t[4 * i + 3] << 24);
}

// Frames [first, first + n) of a buffer that holds frames (reserved: set by the first build or upload)
static bool frames_range_ok(const pbgpu_frames *f, uint64_t first, uint64_t n)
{
    return f->reserved != NULL && first <= f->n_frames && n <= f->n_frames - first;
}

// The bytes of frames [first, first + n) and where they end in the buffer: from the fixed length,
// or offsets[first + n] - offsets[first] read back (after materialising them).
static int range_bytes(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first, uint64_t n, uint64_t *body,
                       uint64_t *src_end)
{
    if (ctx == NULL || src == NULL || !frames_range_ok(src, first, n))
        return PBGPU_EINVAL;
    *body = 0;
    *src_end = 0;
    if (n == 0)
        return PBGPU_OK;
    if (src->fixed_len)
    {
        *body = n * src->fixed_len;
        *src_end = (first + n) * src->fixed_len;
        return PBGPU_OK;
    }
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx);
    PBCHK(materialize_offsets(ctx, src));
    uint64_t o[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&o[0], src->offsets + first, sizeof o[0], hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&o[1], src->offsets + first + n, sizeof o[1], hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (o[1] < o[0])
        return PBGPU_EIO;
    *body = o[1] - o[0];
    *src_end = o[1];
    return PBGPU_OK;
}

// A repacker's source and destination must be apart: the allocations, the readers' 64-B slack included
static bool buffers_overlap(const pbgpu_frames *src, const pbgpu_frames *dst)
{
    const uintptr_t s0 = (uintptr_t)src->data, s1 = s0 + src->capacity_bytes + 64;
    const uintptr_t d0 = (uintptr_t)dst->data, d1 = d0 + dst->capacity_bytes + 64;
    return s0 < d1 && d0 < s1;
}

// Taking a buffer over as the destination of a build, an upload or a repack on `st`: the work
// follows the buffer's last writer on another stream, and the landings queued from the buffer (a
// landing never reads frames being overwritten). The lengths are those of the frames to come.
static int take_inplace(pbgpu_frames *dst, hipStream_t st, frames_events **fe_out);

static int take_dst(pbgpu_frames *dst, hipStream_t st, uint32_t min_len, uint32_t max_len, frames_events **fe_out)
{
    frames_events *fe = nullptr;
    PBCHK(take_inplace(dst, st, &fe));
    fe->packed32 = false;
    fe->min_len = min_len;
    fe->max_len = max_len;
    if (fe_out)
        *fe_out = fe;
    return PBGPU_OK;
}

// Its sibling for a writer that changes bytes of the frames in place (pbgpu_stamp): the same
// ordering, while the frames, their offsets and the recorded lengths stay what they are.
static int take_inplace(pbgpu_frames *dst, hipStream_t st, frames_events **fe_out)
{
    frames_events *fe = frames_ev(dst);
    if (fe == NULL)
        return PBGPU_ENOMEM;
    if (fe->last && fe->last != st)
    {
        if (fe->moved == nullptr)
            HIPCHK(hipEventCreateWithFlags(&fe->moved, hipEventDisableTiming));
        HIPCHK(hipEventRecord(fe->moved, fe->last));
        HIPCHK(hipStreamWaitEvent(st, fe->moved, 0));
    }
    fe->last = st;
    if (fe->land_pending)
    {
        HIPCHK(hipStreamWaitEvent(st, fe->landed, 0));
        fe->land_pending = false;
    }
    if (fe_out)
        *fe_out = fe;
    return PBGPU_OK;
}

int pbgpu_frames_offsets(pbgpu_ctx *ctx, pbgpu_frames *f)
{
    if (ctx == NULL || f == NULL)
        return PBGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    return materialize_offsets(ctx, f);
}

// A part of pbgpu_build_batch's fused launch: the stream it runs on and its block size in; the
// build's kargs out (built = false: no frames, nothing to launch)
struct batch_part
{
    hipStream_t st;
    uint32_t wgt;
    pb_kargs K;
    bool built;
    uint64_t ctr_words; // count-ring words the part reserved (returned if the launch fails)
};

// Every argument check of a build, before anything is changed (pbgpu_build_batch checks all its
// parts first, so a part that cannot be built leaves the others untouched).
static int build_check(pbgpu_ctx *ctx, uint16_t seq_idx, uint64_t first_iter, uint64_t n_iter,
                       const pbgpu_frames *out)
{
    if (ctx == NULL || out == NULL || seq_idx >= PB_MAX_SEQUENCES)
        return PBGPU_EINVAL;
    const seq_slot &S = ctx->seqs[seq_idx];
    if (!S.loaded)
        return PBGPU_ENOENT;
    const uint64_t nf = n_iter * S.fpi;
    if (nf > out->capacity_frames || nf > 0xFFFFFFFFull)
        return PBGPU_ENOSPC;
    if (first_iter + n_iter >= PB_STATIC_SEED_K)
        return PBGPU_EINVAL;
    const uint64_t max_bytes = nf * S.max_flen;
    if (((max_bytes + 15) & ~15ull) > out->capacity_bytes)
        return PBGPU_ENOSPC;
    return PBGPU_OK;
}

// pbgpu_build, or with bp: every step of it but the launch (and its timing), on bp->st
static int build_impl(pbgpu_ctx *ctx, uint16_t seq_idx, uint64_t first_iter, uint64_t n_iter, pbgpu_frames *out,
                      batch_part *bp)
{
    {
        const int crc = build_check(ctx, seq_idx, first_iter, n_iter, out);
        if (crc != PBGPU_OK)
            return crc;
    }
    seq_slot &S = ctx->seqs[seq_idx];
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t nf = n_iter * S.fpi;

    // the stream this build runs on: the sequence's own in span mode (builds of different
    // sequences overlap), the context's otherwise (each launch timed on its own)
    hipStream_t st = ctx->stream;
    const bool span = ctx->timing_mode == PBGPU_TIMING_SPAN;
    int si = -1;
    if (bp)
        st = bp->st, bp->built = false;
    else if (span && ctx->opt.seq_streams)
    {
        si = seq_idx % PB_SEQ_STREAMS;
        if (ctx->seq_stream[si] == nullptr)
            HIPCHK(hipStreamCreateWithFlags(&ctx->seq_stream[si], hipStreamNonBlocking));
        st = ctx->seq_stream[si];
    }
    frames_events *fe = nullptr;
    PBCHK(take_dst(out, st, S.min_flen, S.max_flen, &fe));
    pb_kargs K = S.K;
    K.first_iter = first_iter;
    K.n_frames = nf;
    K.out = out->data;
    K.offsets = out->offsets;
    out->seq_idx = seq_idx;
    out->first_iter = first_iter;
    out->n_frames = nf;
    out->fixed_len = K.fixed_len;
    if (nf == 0)
    {
        out->total_bytes = 0;
        return PBGPU_OK;
    }
    if (K.fixed_len)
    {
        K.total_bytes = nf * K.fixed_len;
        out->total_bytes = K.total_bytes;
    }
    else
    {
        out->total_bytes = UINT64_MAX;
        K.vblk_sum = nullptr;
        K.vblk_l2 = nullptr;
        K.offsets_w = nullptr;
        const bool vp = S.plan.kern == PB_KERN_VPAGE, vl = S.plan.kern == PB_KERN_VLINE;
        const uint32_t wgf = pb_plan_len_wgf(S.plan, S.opt, K);
        if (wgf)
        {
            // pb_vline_kernel / pb_vstage_kernel: per-workgroup length sums, their scan, offsets
            // written by the build
            const uint64_t nblk = (nf + wgf - 1) / wgf;
            const uint64_t n_l2 = (nblk + PB_VL_GRP - 1) / PB_VL_GRP;
            uint32_t *bsum = reinterpret_cast<uint32_t *>(out->scan_tmp);
            unsigned long long *l2 =
                reinterpret_cast<unsigned long long *>(reinterpret_cast<uint8_t *>(out->scan_tmp) + vst_bsum_bytes(nblk));
            HIPCHK(pbk_launch_vst_lengths(&K, wgf, bsum, (uint32_t)nblk, l2, (uint32_t)n_l2, out->offsets, st));
            K.vblk_sum = bsum;
            K.vblk_l2 = l2;
            K.offsets_w = out->offsets;
            if (vp)
            {
                // the record pass's records (8 B per frame) and page table (8 B per page of the
                // buffer's capacity); the page grid covers the longest stream these frames can make
                if (fe->d_vrec == nullptr)
                    HIPCHK(fb_alloc(ctx, (void **)&fe->d_vrec, out->capacity_frames * sizeof(uint2)));
                // (every wave of the grid below loads its first page's entry before it looks at the
                // stream's length, and the grid is whole groups of 32 pages: up to 31 entries past
                // the buffer's last page are read, never used)
                if (fe->d_vpt == nullptr)
                    HIPCHK(hipMalloc((void **)&fe->d_vpt,
                                     ((out->capacity_bytes / 4096 + 2 + 31) / 32 * 32) * sizeof(uint2)));
                K.vp_rec = fe->d_vrec;
                K.vp_pt = fe->d_vpt;
                // the grid covers the expected stream (one random payload of uniform length: the
                // mean frame) plus 1% and 64 pages; a longer stream is built by the same waves in
                // later rounds.  (A grid for the longest possible stream, 1.87x configs[2]'s, spent
                // ~2 ms per 2^25 frames on workgroups past the stream's end.)
                const uint64_t pages_max = (nf * S.max_flen + 4095) / 4096;
                uint64_t pages_est = (uint64_t)((double)nf * 0.5 * (S.min_flen + S.max_flen) * 1.01 / 4096.0) + 64;
                if (S.opt.vp_pages_pct)
                    pages_est = pages_est * S.opt.vp_pages_pct / 100 + 1;
                const uint64_t pages = pages_est < pages_max ? pages_est : pages_max;
                const uint64_t ppg = 32; // pages per group of 8 workgroups (4 per workgroup)
                if ((pages + ppg - 1) / ppg * 8 > 0x7FFFFFFFull)
                    return PBGPU_ENOSPC;
                K.vp_grid = (uint32_t)((pages + ppg - 1) / ppg * 8);
            }
            if (vl || vp)
            {
                // 4 B per frame and 8 B per region instead of 8 B per frame
                // (each checked on its own: a failed second allocation must not leave the pair
                // half set for the next build to launch with a null region-start array)
                if (fe->d_off32 == nullptr)
                    HIPCHK(fb_alloc(ctx, (void **)&fe->d_off32, (out->capacity_frames + 1) * sizeof(uint32_t)));
                if (fe->d_rstart == nullptr)
                    HIPCHK(hipMalloc((void **)&fe->d_rstart, (out->capacity_frames / 32 + 2) * sizeof(unsigned long long)));
                K.offsets32 = fe->d_off32;
                K.vl_rstart = fe->d_rstart;
                fe->packed32 = true;
                fe->wf = wgf;
            }
        }
        else
        {
            const uint64_t nblocks = (nf + PB_SCAN_FRAMES_PER_BLOCK - 1) / PB_SCAN_FRAMES_PER_BLOCK;
            HIPCHK(pbk_launch_lengths(&K, (unsigned long long *)out->scan_tmp, (uint32_t)nblocks, out->offsets, st));
        }
    }
    // the kernel this build launches (the small family falls back to pb_small_kernel on an output
    // not 4-KiB aligned) and its page arithmetic
    const pb_kern kern = pb_plan_launch(S.plan, S.opt, bp ? bp->wgt : 0u, K);
    timing_pair tp = {nullptr, nullptr};
    int rc = PBGPU_OK;
    // this launch's per-workgroup count records (pb_count): the next words of the sequence's
    // ring, folded into the counters first when it is full (PBGPU_CTR_ATOMIC=1: one atomic per
    // workgroup instead).  Reserved last, after everything that can fail but the launch itself;
    // a launch that fails returns them (its records would never be written)
    K.ctr_slots = nullptr;
    uint64_t words = 0;
    if (!S.opt.ctr_atomic)
    {
        const uint64_t pairs = K.fixed_len ? 1 : 2;
        words = (uint64_t)pbk_build_grid(&K, kern) * pairs;
        if (S.ctr_pairs != pairs || S.ctr_used + words > S.ctr_cap)
        {
            if ((rc = ctr_fold(ctx, seq_idx, st)) != PBGPU_OK)
                return rc;
            S.ctr_pairs = pairs;
            if (words > S.ctr_cap)
            {
                HIPCHK(hipStreamSynchronize(st)); // the old ring's fold has read it
                if (S.d_ctr_slots)
                    (void)hipFree(S.d_ctr_slots);
                S.d_ctr_slots = nullptr;
                S.ctr_cap = 0;
                // (PBGPU_CTR_RING = words: a small ring, so the tests reach the fold-when-full path)
                const uint64_t ring = S.opt.ctr_ring ? (uint64_t)S.opt.ctr_ring : PB_CTR_RING_WORDS;
                const uint64_t cap = words > ring ? words : ring;
                HIPCHK(hipMalloc((void **)&S.d_ctr_slots, cap * sizeof(uint32_t)));
                S.ctr_cap = cap;
            }
        }
        if ((rc = ctr_order(S, st)) != PBGPU_OK)
            return rc;
        K.ctr_slots = S.d_ctr_slots + S.ctr_used;
        S.ctr_used += words;
    }
    if (bp)
    {
        bp->K = K;
        bp->built = true;
        bp->ctr_words = words;
        return PBGPU_OK;
    }
    // every error exit from here on returns the reserved count-ring words (their records would
    // never be written, and the next fold would read stale ones) and the timing pair
    auto undo = [&]() {
        S.ctr_used -= words;
        if (tp.a)
            ctx->pool.push_back(tp);
    };
#define HIPCHK_UNDO(call)                                                                    \
    do                                                                                       \
    {                                                                                        \
        const hipError_t u_ = (call);                                                        \
        if (u_ != hipSuccess)                                                                \
        {                                                                                    \
            undo();                                                                          \
            HIPCHK(u_);                                                                      \
        }                                                                                    \
    } while (0)
    if (span)
    {
        if (ctx->span_n == 0)
        {
            if (ctx->span.a == nullptr)
            {
                HIPCHK_UNDO(hipEventCreate(&ctx->span.a));
                HIPCHK_UNDO(hipEventCreate(&ctx->span.b));
            }
            HIPCHK_UNDO(hipEventRecord(ctx->span.a, ctx->stream));
            for (bool &j : ctx->seq_in_span)
                j = false;
        }
        if (si >= 0)
        {
            if (!ctx->seq_in_span[si]) // the span starts before this stream's first launch in it
            {
                HIPCHK_UNDO(hipStreamWaitEvent(st, ctx->span.a, 0));
                ctx->seq_in_span[si] = true;
            }
            ctx->seq_dirty[si] = true;
        }
        HIPCHK_UNDO(pbk_launch_build(&K, kern, st));
        ++ctx->span_n;
        return mark_built(ctx, out, st);
    }
    if ((rc = timed_pair(ctx, &tp)) != PBGPU_OK)
    {
        undo();
        return rc;
    }
    HIPCHK_UNDO(hipEventRecord(tp.a, ctx->stream));
    HIPCHK_UNDO(pbk_launch_build(&K, kern, ctx->stream));
#undef HIPCHK_UNDO
    // launched: its records will be written; a failing end event drops only this timing
    HIPCHK(hipEventRecord(tp.b, ctx->stream));
    if ((rc = mark_built(ctx, out, st)) != PBGPU_OK)
        return rc;
    ctx->pending.push_back(tp);
    if (ctx->pending.size() >= 4096)
    {
        double ms; // bound the pending list (this drops the older timings)
        uint32_t n;
        rc = pbgpu_kernel_time(ctx, &ms, &n);
        if (rc)
            return rc;
    }
    return PBGPU_OK;
}

int pbgpu_build(pbgpu_ctx *ctx, uint16_t seq_idx, uint64_t first_iter, uint64_t n_iter, pbgpu_frames *out)
{
    return build_impl(ctx, seq_idx, first_iter, n_iter, out, nullptr);
}


// The fused form applies: three distinct sequences of kinds 1, 2, 3 (pbk_batch_kind), into three
// distinct 4-KiB-aligned buffers, each with frames to build; order[k] = the part of kind k + 1
static bool batch_fusable(pbgpu_ctx *ctx, uint32_t n, const uint16_t *seq_idx, const uint64_t *n_iter,
                          pbgpu_frames *const *outs, uint32_t order[3])
{
    if (n != 3)
        return false;
    bool seen[3] = {false, false, false};
    for (uint32_t i = 0; i < 3; ++i)
    {
        const seq_slot &S = ctx->seqs[seq_idx[i]];
        if (!S.loaded || !S.opt.batch || S.opt.kernel == PBO_K_LINEAR)
            return false;
        const int kd = pbk_batch_kind(&S.K);
        if (kd < 1 || kd > 3 || seen[kd - 1] || n_iter[i] == 0 || ((uintptr_t)outs[i]->data & 4095u) != 0)
            return false;
        seen[kd - 1] = true;
        order[kd - 1] = i;
        for (uint32_t j = 0; j < i; ++j)
            if (seq_idx[j] == seq_idx[i] || outs[j] == outs[i])
                return false;
    }
    return true;
}

int pbgpu_build_batch(pbgpu_ctx *ctx, uint32_t n, const uint16_t *seq_idx, const uint64_t *first_iter,
                      const uint64_t *n_iter, pbgpu_frames *const *outs)
{
    if (ctx == NULL || (n && (seq_idx == NULL || first_iter == NULL || n_iter == NULL || outs == NULL)))
        return PBGPU_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
        if (outs[i] == NULL || seq_idx[i] >= PB_MAX_SEQUENCES)
            return PBGPU_EINVAL;
    // every part's arguments first: a part that cannot be built fails the call before any part
    // is launched or reserves count records
    for (uint32_t i = 0; i < n; ++i)
    {
        const int rc = build_check(ctx, seq_idx[i], first_iter[i], n_iter[i], outs[i]);
        if (rc != PBGPU_OK)
            return rc;
    }
    HIPCHK(hipSetDevice(ctx->device));
    uint32_t order[3];
    if (!batch_fusable(ctx, n, seq_idx, n_iter, outs, order))
    {
        // no fused form: one launch per part, as pbgpu_build
        for (uint32_t i = 0; i < n; ++i)
        {
            const int rc = pbgpu_build(ctx, seq_idx[i], first_iter[i], n_iter[i], outs[i]);
            if (rc != PBGPU_OK)
                return rc;
        }
        return PBGPU_OK;
    }
    // every part on the context's stream, then one launch
    hipStream_t st = ctx->stream;
    const bool span = ctx->timing_mode == PBGPU_TIMING_SPAN;
    timing_pair tp = {nullptr, nullptr};
    if (!span)
    {
        const int rc = timed_pair(ctx, &tp);
        if (rc != PBGPU_OK)
            return rc;
    }
    batch_part bp[3]; // (build_impl orders each part after its buffer's and count ring's last stream)
    pb_kargs Ks[3];
    // a failure after parts reserved count records returns them (those records are never written)
    auto unreserve = [&](uint32_t parts) {
        for (uint32_t k = 0; k < parts; ++k)
            ctx->seqs[seq_idx[order[k]]].ctr_used -= bp[k].ctr_words;
        if (tp.a)
            ctx->pool.push_back(tp);
    };
    for (uint32_t k = 0; k < 3; ++k)
    {
        const uint32_t i = order[k];
        bp[k].st = st;
        bp[k].wgt = ctx->opt.batch_wgt;
        bp[k].ctr_words = 0;
        const int rc = build_impl(ctx, seq_idx[i], first_iter[i], n_iter[i], outs[i], &bp[k]);
        if (rc != PBGPU_OK || !bp[k].built)
        {
            unreserve(k + (rc == PBGPU_OK ? 1u : 0u));
            return rc != PBGPU_OK ? rc : PBGPU_EINVAL; // (n_iter > 0 was checked: not built is unreachable)
        }
        Ks[k] = bp[k].K;
    }
    // (every error exit from here to the launch returns the three parts' reservations)
#define HIPCHK_UNRES(call)                                                                   \
    do                                                                                       \
    {                                                                                        \
        const hipError_t u_ = (call);                                                        \
        if (u_ != hipSuccess)                                                                \
        {                                                                                    \
            unreserve(3);                                                                    \
            HIPCHK(u_);                                                                      \
        }                                                                                    \
    } while (0)
    if (span && ctx->span_n == 0)
    {
        if (ctx->span.a == nullptr)
        {
            HIPCHK_UNRES(hipEventCreate(&ctx->span.a));
            HIPCHK_UNRES(hipEventCreate(&ctx->span.b));
        }
        HIPCHK_UNRES(hipEventRecord(ctx->span.a, ctx->stream));
        for (bool &j : ctx->seq_in_span)
            j = false;
    }
    if (!span)
        HIPCHK_UNRES(hipEventRecord(tp.a, st));
    HIPCHK_UNRES(pbk_launch_batch(Ks, ctx->opt.batch_wgt, st));
#undef HIPCHK_UNRES
    if (span)
        ++ctx->span_n;
    else
    {
        HIPCHK(hipEventRecord(tp.b, st));
        ctx->pending.push_back(tp);
    }
    for (uint32_t i = 0; i < 3; ++i)
    {
        const int rc = mark_built(ctx, outs[i], st);
        if (rc != PBGPU_OK)
            return rc;
    }
    return PBGPU_OK;
}

int pbgpu_sync(pbgpu_ctx *ctx)
{
    if (ctx == NULL)
        return PBGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBGPU_OK;
}

int pbgpu_frames_total(pbgpu_ctx *ctx, pbgpu_frames *f, uint64_t *total)
{
    if (ctx == NULL || f == NULL)
        return PBGPU_EINVAL;
    if (f->fixed_len || f->n_frames == 0)
    {
        if (total)
            *total = f->total_bytes;
        return PBGPU_OK;
    }
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx);
    uint64_t t = 0;
    HIPCHK(hipMemcpyAsync(&t, f->offsets + f->n_frames, sizeof t, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    f->total_bytes = t;
    if (total)
        *total = t;
    return PBGPU_OK;
}

int pbgpu_copy_packed(pbgpu_ctx *ctx, const pbgpu_frames *f, void *dst, uint64_t byte_offset, uint64_t nbytes)
{
    if (ctx == NULL || f == NULL || dst == NULL || byte_offset + nbytes > f->capacity_bytes)
        return PBGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx);
    HIPCHK(hipMemcpyAsync(dst, f->data + byte_offset, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBGPU_OK;
}

int pbgpu_copy_offsets(pbgpu_ctx *ctx, const pbgpu_frames *f, uint64_t *dst)
{
    if (ctx == NULL || f == NULL || dst == NULL)
        return PBGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    if (f->fixed_len)
    {
        for (uint64_t i = 0; i <= f->n_frames; ++i)
            dst[i] = i * f->fixed_len;
        return PBGPU_OK;
    }
    PB_JOIN(ctx);
    {
        const int mrc = materialize_offsets(ctx, f);
        if (mrc != PBGPU_OK)
            return mrc;
    }
    HIPCHK(hipMemcpyAsync(dst, f->offsets, (f->n_frames + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                          ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBGPU_OK;
}

// ---- verification ----

// pb_vst_kernel's (and pb_wire_kernel's) launch of n frames of mean length `mean`: G lanes per frame,
// frames per workgroup and per stage window
static int vst_shape(const pbgpu_frames *f, uint64_t n, uint64_t mean, uint32_t *wgf, uint32_t *bf_out,
                     uint32_t *grid)
{
    const int G = mean <= 192 ? 8 : (mean <= 768 ? 16 : (mean <= 3072 ? 32 : 64));
    const uint32_t ng = PB_VST_WT / (uint32_t)G;
    // a window fills the stage (fixed length), or three quarters of it: a variable-length window of
    // longer frames then still fits (one that does not is summed from global memory)
    const uint64_t target = f->fixed_len ? PB_VS_STAGE - 16 : PB_VS_STAGE / 4 * 3;
    uint64_t bf = target / (mean ? mean : 1) / ng * ng;
    bf = bf < ng ? ng : (bf > PB_VS_BF_MAX ? PB_VS_BF_MAX : bf);
    uint64_t nw = n / (bf * 16384); // windows per workgroup
    nw = nw < 1 ? 1 : (nw > 64 ? 64 : nw);
    *bf_out = (uint32_t)bf;
    *wgf = (uint32_t)(bf * nw);
    *grid = (uint32_t)((n + *wgf - 1) / *wgf);
    return G;
}

// The verify launch of frames [first, first + n): pb_vpg_kernel for fixed lengths up to 128 B,
// pb_vst_kernel with G lanes per frame by the mean length otherwise.
static int verify_shape(const pbgpu_frames *f, uint64_t first, uint64_t n, uint64_t mean, pb_vargs *A, uint32_t *grid)
{
    if (f->fixed_len && f->fixed_len <= 128)
    {
        const uint64_t b0 = first * f->fixed_len, b1 = (first + n) * f->fixed_len;
        A->page0 = b0 >> 12;
        A->npages = ((b1 - 1) >> 12) - A->page0 + 1;
        // pages per wave. n <= n_frames < 2^32 of at most 128 B: npages <= 2^27 + 1, far from
        // page_grid's grid cap and its refusal
        (void)page_grid(A->npages, 0, &A->wgf, grid);
        return 0;
    }
    return vst_shape(f, n, mean, &A->wgf, &A->bf, grid);
}

// One check of frames [first, first + n), for pbgpu_verify and pbgpu_verify_wire.  A is the kernel's
// argument block, its fields from `checks` on filled by the caller; shape(mean, &grid) chooses the
// launch by the mean length and returns what launch(shape, grid) wants.  After it ctx->h_vres holds
// the ncnt counts in the record's order, then the first bad index.
#define PB_CHECK_RES 12 // the most: pbgpu_verify_wire's eleven counts and the index
extern "C++" template <class ARGS, class SHAPE, class LAUNCH>
static int run_check(pbgpu_ctx *ctx, pbgpu_frames *f, uint64_t first, uint64_t n, ARGS &A, uint32_t ncnt,
                     SHAPE shape, LAUNCH launch, uint8_t *codes_out, double *device_ms)
{
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx);
    uint64_t mean = f->fixed_len;
    if (!f->fixed_len)
    {
        const int mrc = materialize_offsets(ctx, f);
        if (mrc != PBGPU_OK)
            return mrc;
        uint64_t total = 0;
        const int trc = pbgpu_frames_total(ctx, f, &total);
        if (trc != PBGPU_OK)
            return trc;
        mean = total / f->n_frames;
    }
    A.data = f->data;
    A.offsets = f->fixed_len ? nullptr : f->offsets;
    A.first = first;
    A.n = n;
    A.fixed_len = f->fixed_len;
    uint32_t grid = 0;
    const int sh = shape(mean, &grid);
    const size_t rec_bytes = (size_t)grid * PB_REC_DW(ncnt) * sizeof(uint32_t);
    PBCHK(scratch_reserve((void **)&ctx->d_vfy_rec, &ctx->vfy_rec_cap, rec_bytes, rec_bytes));
    if (ctx->h_vres == nullptr)
    {
        HIPCHK(hipHostMalloc((void **)&ctx->h_vres, PB_CHECK_RES * sizeof(unsigned long long),
                             hipHostMallocMapped | hipHostMallocCoherent));
        HIPCHK(hipHostGetDevicePointer((void **)&ctx->d_vres, ctx->h_vres, 0));
    }
    if (codes_out)
        PBCHK(scratch_reserve((void **)&ctx->d_vcodes, &ctx->vcodes_cap, n, n));
    A.rec = ctx->d_vfy_rec;
    A.codes = codes_out ? ctx->d_vcodes : nullptr;
    timing_pair tp;
    PBCHK(timed_begin(ctx, &tp));
    HIPCHK(launch(sh, grid));
    HIPCHK(pbk_launch_vfold(ctx->d_vfy_rec, grid, ncnt, ctx->d_vres, ctx->stream));
    PBCHK(timed_stop(ctx, tp));
    if (codes_out) // after the timed stretch
        HIPCHK(hipMemcpyAsync(codes_out, ctx->d_vcodes, n, hipMemcpyDeviceToHost, ctx->stream));
    float ms = 0;
    PBCHK(timed_ms(ctx, tp, &ms));
    *device_ms = ms;
    return PBGPU_OK;
}

int pbgpu_verify(pbgpu_ctx *ctx, pbgpu_frames *f, uint64_t first_frame, uint64_t n, uint32_t checks,
                 pbgpu_verify_result *res, uint8_t *codes_out)
{
    if (ctx == NULL || f == NULL || res == NULL || !frames_range_ok(f, first_frame, n))
        return PBGPU_EINVAL;
    memset(res, 0, sizeof *res);
    res->first_bad = UINT64_MAX;
    if (n == 0)
        return PBGPU_OK;
    res->n_checked = n;
    if (f->fixed_len && f->fixed_len < 34) // every frame is short: nothing to read
    {
        res->n_bad = res->bad_short = n;
        res->first_bad = first_frame;
        if (codes_out)
            memset(codes_out, PBGPU_VERIFY_SHORT, n);
        return PBGPU_OK;
    }
    pb_vargs A;
    memset(&A, 0, sizeof A);
    A.checks = checks & PBGPU_VERIFY_ALL;
    PBCHK(run_check(
        ctx, f, first_frame, n, A, 5,
        [&](uint64_t mean, uint32_t *grid) { return verify_shape(f, first_frame, n, mean, &A, grid); },
        [&](int shape, uint32_t grid) { return pbk_launch_verify(&A, shape, grid, ctx->stream); }, codes_out,
        &res->device_ms));
    const unsigned long long *h = ctx->h_vres;
    res->n_bad = h[0];
    res->bad_short = h[1];
    res->bad_ip_csum = h[2];
    res->bad_tot_len = h[3];
    res->bad_l4_csum = h[4];
    res->first_bad = h[5];
    return PBGPU_OK;
}

// ---- verification as sent ----

int pbgpu_verify_wire(pbgpu_ctx *ctx, pbgpu_frames *f, uint64_t first_frame, uint64_t n, const pbgpu_wire_opts *opts,
                      pbgpu_wire_result *res, uint8_t *codes_out)
{
    if (ctx == NULL || f == NULL || opts == NULL || res == NULL || !frames_range_ok(f, first_frame, n))
        return PBGPU_EINVAL;
    if ((opts->checks & ~PBGPU_WIRE_ALL) || opts->flags || opts->reserved[0] || opts->reserved[1] || opts->reserved[2])
        return PBGPU_EINVAL;
    memset(res, 0, sizeof *res);
    res->first_bad = UINT64_MAX;
    if (n == 0)
        return PBGPU_OK;
    res->n_checked = n;
    if (f->fixed_len && f->fixed_len < 14) // no frame holds an Ethernet header: nothing to read
    {
        res->n_bad = res->bad_malformed = n;
        res->first_bad = first_frame;
        if (codes_out)
            memset(codes_out, PBGPU_WIRE_MALFORMED, n);
        return PBGPU_OK;
    }
    pb_wargs A;
    memset(&A, 0, sizeof A);
    A.checks = opts->checks;
    A.port = opts->vxlan_port;
    PBCHK(run_check(
        ctx, f, first_frame, n, A, 11,
        [&](uint64_t mean, uint32_t *grid) { return vst_shape(f, n, mean, &A.wgf, &A.bf, grid); },
        [&](int G, uint32_t grid) { return pbk_launch_wire(&A, G, grid, ctx->stream); }, codes_out, &res->device_ms));
    const unsigned long long *h = ctx->h_vres;
    res->n_bad = h[0];
    res->bad_malformed = h[1];
    res->bad_l3_csum = h[2];
    res->bad_l3_len = h[3];
    res->bad_l4_csum = h[4];
    res->bad_udp_len = h[5];
    res->n_ipv4 = h[6];
    res->n_ipv6 = h[7];
    res->n_inner = h[8];
    res->n_nol4 = h[9];
    res->n_other = h[10];
    res->first_bad = h[11];
    return PBGPU_OK;
}

int pbgpu_frames_upload(pbgpu_ctx *ctx, pbgpu_frames *f, const void *host_data, const uint64_t *host_offsets,
                        uint32_t fixed_len, uint64_t n)
{
    if (ctx == NULL || f == NULL)
        return PBGPU_EINVAL;
    uint64_t total = 0, max_len = 0, min_len = UINT64_MAX;
    if (host_offsets)
    {
        for (uint64_t i = 0; i < n; ++i)
        {
            if (host_offsets[i + 1] < host_offsets[i] || host_offsets[i + 1] - host_offsets[i] > PB_MAX_PCKT_LEN)
                return PBGPU_EINVAL;
            max_len = host_offsets[i + 1] - host_offsets[i] > max_len ? host_offsets[i + 1] - host_offsets[i] : max_len;
            min_len = host_offsets[i + 1] - host_offsets[i] < min_len ? host_offsets[i + 1] - host_offsets[i] : min_len;
        }
        total = host_offsets[n] - host_offsets[0];
        fixed_len = 0;
    }
    else
    {
        if (fixed_len == 0 || fixed_len > PB_MAX_PCKT_LEN)
            return PBGPU_EINVAL;
        total = n * fixed_len;
        min_len = max_len = fixed_len;
    }
    if (n == 0)
        min_len = max_len = 0;
    if (total && host_data == NULL)
        return PBGPU_EINVAL;
    if (n > f->capacity_frames || n > 0xFFFFFFFFull || ((total + 15) & ~15ull) > f->capacity_bytes)
        return PBGPU_ENOSPC;
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx);
    hipStream_t st = ctx->stream;
    PBCHK(take_dst(f, st, (uint32_t)min_len, (uint32_t)max_len, nullptr));
    if (total)
        HIPCHK(hipMemcpyAsync(f->data, host_data, total, hipMemcpyHostToDevice, st));
    std::vector<uint64_t> off;
    if (host_offsets) // frame 0 at byte 0, as a build packs them
    {
        off.resize(n + 1);
        for (uint64_t i = 0; i <= n; ++i)
            off[i] = host_offsets[i] - host_offsets[0];
        HIPCHK(hipMemcpyAsync(f->offsets, off.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    f->first_iter = 0;
    f->n_frames = n;
    f->fixed_len = fixed_len;
    f->total_bytes = total;
    return mark_built(ctx, f, st);
}

int pbgpu_read_probe_at(pbgpu_ctx *ctx, const void *src, uint64_t bytes, uint32_t reps, double *ms_per_launch)
{
    if (ctx == NULL || src == NULL || bytes < 16 || reps == 0 || ((uintptr_t)src & 15u))
        return PBGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx);
    uint32_t *out = nullptr;
    HIPCHK(hipMalloc((void **)&out, ((bytes / 16 + 255) / 256) * sizeof(uint32_t)));
    hipEvent_t a = nullptr, b = nullptr;
    float ms = 0;
    hipError_t e = hipEventCreate(&a);
    if (e == hipSuccess)
        e = hipEventCreate(&b);
    if (e == hipSuccess)
        e = pbk_launch_read(src, bytes, out, ctx->stream); // warm-up
    if (e == hipSuccess)
        e = hipEventRecord(a, ctx->stream);
    for (uint32_t r = 0; r < reps && e == hipSuccess; ++r)
        e = pbk_launch_read(src, bytes, out, ctx->stream);
    if (e == hipSuccess)
        e = hipEventRecord(b, ctx->stream);
    if (e == hipSuccess)
        e = hipEventSynchronize(b);
    if (e == hipSuccess)
        e = hipEventElapsedTime(&ms, a, b);
    if (a)
        (void)hipEventDestroy(a);
    if (b)
        (void)hipEventDestroy(b);
    (void)hipFree(out);
    if (e != hipSuccess)
        return PBGPU_EIO;
    if (ms_per_launch)
        *ms_per_launch = ms / reps;
    return PBGPU_OK;
}

// ---- the insert writers: pcap pack, encap, xlat46 ----
// Their output record is a source frame plus `add` bytes; they share their start and end, as the
// cut calls share cut_run.

static bool ins_pair_ok(const pbgpu_frames *src, const pbgpu_frames *dst)
{
    return src != dst && src->data != NULL && dst->data != NULL && !buffers_overlap(src, dst);
}

// What the shared body leaves for the call's launch and result
struct ins_state
{
    uint64_t total, end16; // output bytes, and rounded up to 16: what is written
    uint32_t per, grid;    // the writer's launch over the output's 4-KiB pages
    hipStream_t st;
    timing_pair tp;
    float ms;
};

// the arguments every writer's block has
extern "C++" template <class ARGS>
static void ins_args(ARGS *A, const pbgpu_frames *src, const pbgpu_frames *dst, uint64_t first, uint64_t n,
                     uint32_t add)
{
    memset(A, 0, sizeof *A);
    A->src = src->data;
    A->offsets = src->fixed_len ? nullptr : src->offsets;
    A->dst = dst->data;
    A->first = first;
    A->n = n;
    A->fixed_len = src->fixed_len;
    A->rec = make_div(src->fixed_len + add);
}

// The call after its own argument checks and range_bytes: `head` bytes (pcap's file header), then n
// records of a frame plus `add` bytes.  frames: dst holds frames afterwards (else a byte stream: no
// frame count, no lengths, no built event).  classify(r) runs once dst is known to be large enough
// and before anything of it is touched; it may refuse the call, and may begin the timed stretch
// (r.tp) itself.  launch(r) queues the writer.
extern "C++" template <class CLASSIFY, class LAUNCH>
static int ins_run(pbgpu_ctx *ctx, const pbgpu_frames *src, uint64_t n, pbgpu_frames *dst, uint64_t body,
                   uint64_t src_end, uint32_t head, uint32_t add, bool frames, CLASSIFY classify, LAUNCH launch,
                   ins_state *r)
{
    if (src_end > src->capacity_bytes)
        return PBGPU_EINVAL;
    r->total = head + (uint64_t)add * n + body;
    r->end16 = (r->total + 15) & ~15ull;
    if ((frames && n > dst->capacity_frames) || r->end16 > dst->capacity_bytes)
        return PBGPU_ENOSPC;
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx);
    r->st = ctx->stream;
    r->tp = {nullptr, nullptr};
    r->ms = 0;
    PBCHK(classify(*r));
    const frames_events *fs = (const frames_events *)src->reserved;
    const bool lens = frames && n; // a byte stream has no frames, so no lengths
    PBCHK(take_dst(dst, r->st, lens ? fs->min_len + add : 0, lens ? fs->max_len + add : 0, nullptr));
    if (r->end16)
    {
        PBCHK(page_grid((r->end16 + 4095) >> 12, ctx->opt.rp_per, &r->per, &r->grid));
        if (r->tp.a == nullptr)
            PBCHK(timed_begin(ctx, &r->tp));
        HIPCHK(launch(*r));
        PBCHK(timed_stop(ctx, r->tp));
        PBCHK(timed_ms(ctx, r->tp, &r->ms));
    }
    dst->first_iter = 0;
    dst->n_frames = frames ? n : 0;
    dst->fixed_len = frames && src->fixed_len ? src->fixed_len + add : 0;
    dst->total_bytes = r->total;
    return frames ? mark_built(ctx, dst, r->st) : PBGPU_OK;
}

// ---- pcap stream packing ----

#define PB_PCAP_FLAGS (PBGPU_PCAP_FILE_HEADER | PBGPU_PCAP_NSEC)

int pbgpu_pcap_size(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n, uint32_t flags,
                    uint64_t *nbytes)
{
    if (nbytes == NULL || (flags & ~PB_PCAP_FLAGS))
        return PBGPU_EINVAL;
    uint64_t body = 0, src_end = 0;
    PBCHK(range_bytes(ctx, src, first_frame, n, &body, &src_end));
    *nbytes = ((flags & PBGPU_PCAP_FILE_HEADER) ? 24u : 0u) + 16u * n + body;
    return PBGPU_OK;
}

int pbgpu_pcap_pack(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n, const pbgpu_pcap_opts *opts,
                    pbgpu_frames *dst, uint64_t *nbytes, double *device_ms)
{
    if (ctx == NULL || src == NULL || opts == NULL || dst == NULL || nbytes == NULL || opts->reserved != 0)
        return PBGPU_EINVAL;
    if (!ins_pair_ok(src, dst))
        return PBGPU_EINVAL;
    if (opts->flags & ~PB_PCAP_FLAGS)
        return PBGPU_EINVAL;
    if (!stamps_fit(opts->first_index, n, opts->step_ps, opts->t0_ns))
        return PBGPU_EINVAL;
    uint64_t body = 0, src_end = 0;
    PBCHK(range_bytes(ctx, src, first_frame, n, &body, &src_end));
    pb_pcargs A;
    ins_args(&A, src, dst, first_frame, n, 16u);
    A.flags = opts->flags;
    A.hdr = (opts->flags & PBGPU_PCAP_FILE_HEADER) ? 24u : 0u;
    A.t0_ns = opts->t0_ns;
    A.step_ps = opts->step_ps;
    A.first_index = opts->first_index;
    ins_state r;
    PBCHK(ins_run(
        ctx, src, n, dst, body, src_end, A.hdr, 16u, false, [](ins_state &) { return PBGPU_OK; },
        [&](ins_state &r) {
            A.end16 = r.end16;
            A.per = r.per;
            return pbk_launch_pcap(&A, r.grid, r.st);
        },
        &r));
    *nbytes = r.total;
    if (device_ms)
        *device_ms = r.ms;
    return PBGPU_OK;
}

// ---- encapsulation ----

// Argument checks shared by pbgpu_encap_size and pbgpu_encap, then the header's size and the
// frames' bytes (range_bytes).
static int encap_check(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first, uint64_t n, const pbgpu_encap_opts *opts,
                       uint32_t *P, uint64_t *body, uint64_t *src_end)
{
    if (ctx == NULL || src == NULL || opts == NULL || src->reserved == NULL)
        return PBGPU_EINVAL;
    if (opts->mode != PBGPU_ENCAP_VLAN && opts->mode != PBGPU_ENCAP_VXLAN)
        return PBGPU_EINVAL;
    if (opts->flags != 0 || opts->reserved != 0 || opts->vni >= (1u << 24))
        return PBGPU_EINVAL;
    *P = opts->mode == PBGPU_ENCAP_VLAN ? 4u : 50u;
    const frames_events *fs = (const frames_events *)src->reserved;
    if (src->n_frames && (fs->min_len < 14u || fs->max_len > 65535u - *P))
        return PBGPU_EINVAL;
    return range_bytes(ctx, src, first, n, body, src_end);
}

int pbgpu_encap_size(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                     const pbgpu_encap_opts *opts, uint64_t *frames, uint64_t *bytes)
{
    if (frames == NULL || bytes == NULL)
        return PBGPU_EINVAL;
    uint32_t P = 0;
    uint64_t body = 0, src_end = 0;
    PBCHK(encap_check(ctx, src, first_frame, n, opts, &P, &body, &src_end));
    *frames = n;
    *bytes = body + n * P;
    return PBGPU_OK;
}

int pbgpu_encap(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n, const pbgpu_encap_opts *opts,
                pbgpu_frames *dst, double *device_ms)
{
    if (ctx == NULL || src == NULL || opts == NULL || dst == NULL)
        return PBGPU_EINVAL;
    if (!ins_pair_ok(src, dst))
        return PBGPU_EINVAL;
    uint32_t P = 0;
    uint64_t body = 0, src_end = 0;
    PBCHK(encap_check(ctx, src, first_frame, n, opts, &P, &body, &src_end));
    pb_enargs A;
    ins_args(&A, src, dst, first_frame, n, P);
    A.dst_offsets = dst->offsets;
    A.P = P;
    A.hdw = (P + 6u) / 4u; // P + 3 bytes in dwords
    {
        uint8_t t[PB_EN_TDW * 4];
        memset(t, 0, sizeof t);
        if (opts->mode == PBGPU_ENCAP_VLAN)
        {
            const uint16_t tpid = opts->tpid ? opts->tpid : 0x8100;
            A.split = 12;
            t[0] = (uint8_t)(tpid >> 8), t[1] = (uint8_t)tpid;
            t[2] = (uint8_t)(opts->tci >> 8), t[3] = (uint8_t)opts->tci;
        }
        else
        {
            const uint16_t dport = opts->dst_port ? opts->dst_port : 4789;
            A.split = 0;
            A.flags = PB_EN_VXLAN | (opts->src_port ? 0u : PB_EN_HASH);
            memcpy(t, opts->dst_mac, 6);
            memcpy(t + 6, opts->src_mac, 6);
            t[12] = 0x08;
            t[14] = 0x45, t[15] = opts->tos;
            t[20] = 0x40; // DF
            t[22] = opts->ttl ? opts->ttl : 64, t[23] = 17;
            memcpy(t + 26, opts->src_ip, 4);
            memcpy(t + 30, opts->dst_ip, 4);
            t[34] = (uint8_t)(opts->src_port >> 8), t[35] = (uint8_t)opts->src_port;
            t[36] = (uint8_t)(dport >> 8), t[37] = (uint8_t)dport;
            t[42] = 0x08;
            t[46] = (uint8_t)(opts->vni >> 16), t[47] = (uint8_t)(opts->vni >> 8), t[48] = (uint8_t)opts->vni;
            for (int i = 14; i < 34; i += 2)
                A.csum_base += ((uint32_t)t[i] << 8) | t[i + 1];
            if (src->fixed_len) // the same for every frame: only a hashed source port is left to the device
            {
                const uint32_t tot = src->fixed_len + 36u, ulen = src->fixed_len + 16u;
                uint32_t c = A.csum_base + tot;
                while (c >> 16)
                    c = (c & 0xFFFFu) + (c >> 16);
                c = ~c & 0xFFFFu;
                t[16] = (uint8_t)(tot >> 8), t[17] = (uint8_t)tot;
                t[24] = (uint8_t)(c >> 8), t[25] = (uint8_t)c;
                t[38] = (uint8_t)(ulen >> 8), t[39] = (uint8_t)ulen;
            }
        }
        pack_le32(A.tpl, t, PB_EN_TDW);
    }
    ins_state r;
    PBCHK(ins_run(
        ctx, src, n, dst, body, src_end, 0u, P, true, [](ins_state &) { return PBGPU_OK; },
        [&](ins_state &r) {
            A.end16 = r.end16;
            A.per = r.per;
            return pbk_launch_encap(&A, r.grid, r.st); // variable length: dst->offsets by a launch of its own first
        },
        &r));
    if (device_ms)
        *device_ms = r.ms;
    return PBGPU_OK;
}

// ---- cutting frames into pieces: IPv4 fragmentation and L4 segmentation ----

struct cut_call;

// What differs between the two calls, for the helpers they share
struct cut_kind
{
    uint32_t hdr;     // the fixed L2/L3/L4 header bytes in front of the cut data
    uint32_t worst;   // the longest inserted header
    int ins_word;     // the result word holding the inserted bytes; below 0: 34 (n_out - n)
    uint32_t row_sums; // row sums of the count pass: K, and the inserted bytes where they are counted
    // stage 0: count and scans; stage 1: map and writer (pbk_launch_frag, pbk_launch_seg)
    hipError_t (*launch)(const pb_cutargs *A, int stage, int G, uint32_t grid, hipStream_t st);
    // the kind's own refusals, scratch and arguments of the writer, before dst is touched (may be null)
    int (*prepare)(pbgpu_ctx *ctx, pb_cutargs *A, const cut_call &c, const unsigned long long *r, uint64_t src_end,
                   int *G);
};

// One call's options, checked
struct cut_call
{
    const cut_kind *kd;
    uint32_t cut;   // data bytes of a full piece: C, or mss
    uint32_t fit;   // the longest frame that never splits
    uint32_t flags; // PB_FG_* or PB_SG_*
    uint32_t mtu;   // fragment
};

// What the main call's shared body leaves for the result struct
struct cut_done
{
    unsigned long long r[PB_FG_RES_DW];
    uint64_t n_out, total;
    const frames_events *fe; // dst's
    float ms;
};

// Argument checks shared by all six calls, after the options'; nothing on the device.
static int cut_check(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first, uint64_t n)
{
    if (ctx == NULL || src == NULL || !frames_range_ok(src, first, n))
        return PBGPU_EINVAL;
    const frames_events *fs = (const frames_events *)src->reserved;
    if (src->n_frames && fs->min_len < 14u)
        return PBGPU_EINVAL;
    return PBGPU_OK;
}

static void cut_args(pb_cutargs *A, const pbgpu_frames *src, uint64_t first, uint64_t n, const cut_call &c)
{
    memset(A, 0, sizeof *A);
    A->src = src->data;
    A->offsets = src->fixed_len ? nullptr : src->offsets;
    A->first = first;
    A->n = n;
    A->fixed_len = src->fixed_len;
    A->cut = c.cut;
    A->cdiv = make_div(c.cut);
    A->mtu = c.mtu;
    A->flags = c.flags;
}

// The count and scan stages, queued on the context's stream: A's scratch pointers are set, the
// result words arrive in res[] with the stream's next synchronise.
static int cut_count(pbgpu_ctx *ctx, pb_cutargs *A, const cut_call &c, unsigned long long *res)
{
    const uint64_t nblk = (A->n + PB_FG_WT - 1u) / PB_FG_WT;
    if (nblk > 0xFFFFFFFFull)
        return PBGPU_EINVAL;
    const uint64_t bytes = PB_FG_RES_DW * 8u + nblk * 8u * c.kd->row_sums + A->n * 4u;
    PBCHK(scratch_reserve((void **)&ctx->d_cut_cnt, &ctx->cut_cnt_cap, bytes, bytes));
    A->res = (unsigned long long *)ctx->d_cut_cnt;
    A->bsum = A->res + PB_FG_RES_DW;
    A->xsum = c.kd->row_sums > 1u ? A->bsum + nblk : nullptr;
    A->kcnt = (uint32_t *)(A->bsum + nblk * c.kd->row_sums);
    HIPCHK(c.kd->launch(A, 0, 0, 0, ctx->stream));
    HIPCHK(hipMemcpyAsync(res, A->res, PB_FG_RES_DW * 8u, hipMemcpyDeviceToHost, ctx->stream));
    return PBGPU_OK;
}

// the bytes that n_out = r[0] output records of n source frames have had inserted
static uint64_t cut_inserted(const cut_call &c, const unsigned long long *r, uint64_t n)
{
    return c.kd->ins_word < 0 ? 34u * (r[0] - n) : r[c.kd->ins_word];
}

static int cut_bound(const pbgpu_frames *src, uint64_t n, const cut_call &c, uint64_t *frames, uint64_t *bytes)
{
    if (frames == NULL || bytes == NULL)
        return PBGPU_EINVAL;
    const frames_events *fs = (const frames_events *)src->reserved;
    const uint64_t max_len = fs->max_len;
    uint64_t kmax = 1;
    if (max_len > c.fit)
        kmax = (max_len - c.kd->hdr + c.cut - 1u) / c.cut;
    *frames = n * kmax;
    *bytes = n * (src->fixed_len ? src->fixed_len : max_len) + (uint64_t)c.kd->worst * n * (kmax - 1u);
    return PBGPU_OK;
}

static int cut_size(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first, uint64_t n, const cut_call &c, uint64_t *frames,
                    uint64_t *bytes)
{
    if (frames == NULL || bytes == NULL)
        return PBGPU_EINVAL;
    uint64_t body = 0, src_end = 0;
    PBCHK(range_bytes(ctx, src, first, n, &body, &src_end));
    *frames = n;
    *bytes = body;
    const frames_events *fs = (const frames_events *)src->reserved;
    if (n == 0 || fs->max_len <= c.fit) // nothing can split
        return PBGPU_OK;
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx);
    pb_cutargs A;
    cut_args(&A, src, first, n, c);
    unsigned long long r[PB_FG_RES_DW];
    PBCHK(cut_count(ctx, &A, c, r));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (r[0] < n)
        return PBGPU_EIO;
    *frames = r[0];
    *bytes = body + cut_inserted(c, r, n);
    return PBGPU_OK;
}

// The main call up to, and without, mark_built: the caller fills its result struct from d first.
static int cut_run(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first, uint64_t n, const cut_call &c, pbgpu_frames *dst,
                   cut_done *d)
{
    if (dst == NULL || src == dst || src->data == NULL || dst->data == NULL || buffers_overlap(src, dst))
        return PBGPU_EINVAL;
    uint64_t body = 0, src_end = 0;
    PBCHK(range_bytes(ctx, src, first, n, &body, &src_end));
    if (src_end > src->capacity_bytes)
        return PBGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx);
    hipStream_t st = ctx->stream;
    // a fixed-length source none of whose frames can split: no count, a plain copy
    const bool copy = src->fixed_len && src->fixed_len <= c.fit;
    pb_cutargs A;
    cut_args(&A, src, first, n, c);
    const unsigned long long r0[PB_FG_RES_DW] = {n, 0, 0, 0, src->fixed_len, src->fixed_len, 0, 0};
    unsigned long long *r = d->r;
    memcpy(r, r0, sizeof r0);
    timing_pair tp = {nullptr, nullptr};
    if (n)
    {
        PBCHK(timed_begin(ctx, &tp)); // the timed stretch: count, scans, map, segment's sums and writer
        if (!copy)
        {
            // the count and scans run, and their result is read, before anything of dst is touched
            PBCHK(cut_count(ctx, &A, c, r));
            HIPCHK(hipStreamSynchronize(st));
            if (r[0] < n)
                return PBGPU_EIO;
        }
    }
    const uint64_t n_out = r[0];
    const uint64_t total = body + cut_inserted(c, r, n);
    const uint64_t end16 = (total + 15) & ~15ull;
    if (n_out > dst->capacity_frames || end16 > dst->capacity_bytes)
        return PBGPU_ENOSPC;
    int G = 0;
    if (n && !copy)
    {
        A.n_out = n_out;
        if (c.kd->prepare)
            PBCHK(c.kd->prepare(ctx, &A, c, r, src_end, &G));
        PBCHK(scratch_reserve((void **)&ctx->d_cut_map, &ctx->cut_map_cap, n_out, n_out * sizeof(uint64_t)));
    }
    frames_events *fe = nullptr;
    PBCHK(take_dst(dst, st, n ? (uint32_t)r[4] : 0, n ? (uint32_t)r[5] : 0, &fe));
    d->ms = 0;
    if (n)
    {
        uint32_t grid = 0;
        PBCHK(page_grid((end16 + 4095) >> 12, ctx->opt.rp_per, &A.per, &grid));
        if (copy)
            HIPCHK(pbk_launch_cut_copy(src->data, dst->data, first * src->fixed_len, total, end16, A.per, grid, st));
        else
        {
            A.dst = dst->data;
            A.dst_offsets = dst->offsets;
            A.map = ctx->d_cut_map;
            A.total = total;
            A.end16 = end16;
            HIPCHK(c.kd->launch(&A, 1, G, grid, st));
        }
        PBCHK(timed_stop(ctx, tp));
        PBCHK(timed_ms(ctx, tp, &d->ms));
    }
    dst->first_iter = 0;
    dst->n_frames = n_out;
    dst->fixed_len = (n && copy) ? src->fixed_len : 0;
    dst->total_bytes = total;
    d->n_out = n_out;
    d->total = total;
    d->fe = fe;
    return PBGPU_OK;
}

// ---- IPv4 fragmentation ----

static hipError_t frag_launch(const pb_cutargs *A, int stage, int, uint32_t grid, hipStream_t st)
{
    return pbk_launch_frag(A, stage, grid, st);
}

static const cut_kind FRAG_KIND = {34u, 34u, -1, 1u, frag_launch, nullptr};

static int frag_call(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first, uint64_t n, const pbgpu_frag_opts *opts,
                     cut_call *c)
{
    if (opts == NULL)
        return PBGPU_EINVAL;
    if (opts->mtu < 68u || opts->mtu > 65535u || (opts->flags & ~PBGPU_FRAG_IGNORE_DF) || opts->reserved != 0)
        return PBGPU_EINVAL;
    *c = {&FRAG_KIND, (opts->mtu - 20u) & ~7u, opts->mtu + 14u,
          (opts->flags & PBGPU_FRAG_IGNORE_DF) ? PB_FG_IGNORE_DF : 0u, opts->mtu};
    return cut_check(ctx, src, first, n);
}

int pbgpu_fragment_bound(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                         const pbgpu_frag_opts *opts, uint64_t *frames, uint64_t *bytes)
{
    cut_call c;
    PBCHK(frag_call(ctx, src, first_frame, n, opts, &c));
    return cut_bound(src, n, c, frames, bytes);
}

int pbgpu_fragment_size(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                        const pbgpu_frag_opts *opts, uint64_t *frames, uint64_t *bytes)
{
    cut_call c;
    PBCHK(frag_call(ctx, src, first_frame, n, opts, &c));
    return cut_size(ctx, src, first_frame, n, c, frames, bytes);
}

int pbgpu_fragment(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n, const pbgpu_frag_opts *opts,
                   pbgpu_frames *dst, pbgpu_frag_result *res)
{
    cut_call c;
    cut_done d;
    PBCHK(frag_call(ctx, src, first_frame, n, opts, &c));
    PBCHK(cut_run(ctx, src, first_frame, n, c, dst, &d));
    if (res)
    {
        memset(res, 0, sizeof *res);
        res->n_in = n;
        res->n_out = d.n_out;
        res->n_split = d.r[1];
        res->n_df = d.r[2];
        res->n_other = d.r[3];
        res->out_bytes = d.total;
        res->out_min_len = d.fe->min_len;
        res->out_max_len = d.fe->max_len;
        res->device_ms = d.ms;
    }
    return mark_built(ctx, dst, ctx->stream);
}

// ---- L4 segmentation ----

static int seg_prepare(pbgpu_ctx *ctx, pb_cutargs *A, const cut_call &c, const unsigned long long *r, uint64_t src_end,
                       int *G)
{
    if (src_end >> PB_SG_M_ISH) // a map entry keeps 44 bits of source offset
        return PBGPU_EINVAL;
    const bool sums = !(c.flags & PB_SG_NO_L4);
    if (sums)
        PBCHK(scratch_reserve((void **)&ctx->d_cut_psum, &ctx->cut_psum_cap, A->n_out, A->n_out * sizeof(uint32_t)));
    A->psum = ctx->d_cut_psum;
    A->hdw = 10u + (uint32_t)(r[7] < 15u ? r[7] : 15u);
    // lanes per segment by the slice length, as verify_shape picks pb_vst_kernel's G
    *G = !sums ? 0 : c.cut <= 256u ? 8 : c.cut <= 512u ? 16 : c.cut <= 2048u ? 32 : 64;
    return PBGPU_OK;
}

static const cut_kind SEG_KIND = {42u, 94u, 6, 2u, pbk_launch_seg, seg_prepare};

static int seg_call(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first, uint64_t n, const pbgpu_seg_opts *opts,
                    cut_call *c)
{
    if (opts == NULL)
        return PBGPU_EINVAL;
    if (opts->mss < 8u || opts->mss > 65535u || (opts->flags & ~(PBGPU_SEG_NO_L4_CSUM | PBGPU_SEG_FIXED_ID)) ||
        opts->reserved != 0)
        return PBGPU_EINVAL;
    *c = {&SEG_KIND, opts->mss, opts->mss + 42u,
          ((opts->flags & PBGPU_SEG_NO_L4_CSUM) ? PB_SG_NO_L4 : 0u) |
              ((opts->flags & PBGPU_SEG_FIXED_ID) ? PB_SG_FIXED_ID : 0u),
          0u};
    return cut_check(ctx, src, first, n);
}

int pbgpu_segment_bound(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                        const pbgpu_seg_opts *opts, uint64_t *frames, uint64_t *bytes)
{
    cut_call c;
    PBCHK(seg_call(ctx, src, first_frame, n, opts, &c));
    return cut_bound(src, n, c, frames, bytes);
}

int pbgpu_segment_size(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                       const pbgpu_seg_opts *opts, uint64_t *frames, uint64_t *bytes)
{
    cut_call c;
    PBCHK(seg_call(ctx, src, first_frame, n, opts, &c));
    return cut_size(ctx, src, first_frame, n, c, frames, bytes);
}

int pbgpu_segment(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n, const pbgpu_seg_opts *opts,
                  pbgpu_frames *dst, pbgpu_seg_result *res)
{
    cut_call c;
    cut_done d;
    PBCHK(seg_call(ctx, src, first_frame, n, opts, &c));
    PBCHK(cut_run(ctx, src, first_frame, n, c, dst, &d));
    if (res)
    {
        memset(res, 0, sizeof *res);
        res->n_in = n;
        res->n_out = d.n_out;
        res->n_split_tcp = d.r[1];
        res->n_split_udp = d.r[2];
        res->n_other = d.r[3];
        res->out_bytes = d.total;
        res->out_min_len = d.fe->min_len;
        res->out_max_len = d.fe->max_len;
        res->device_ms = d.ms;
    }
    return mark_built(ctx, dst, ctx->stream);
}

// ---- stamping ----

int pbgpu_stamp(pbgpu_ctx *ctx, pbgpu_frames *f, uint64_t first_frame, uint64_t n, const pbgpu_stamp_opts *opts,
                pbgpu_stamp_result *res)
{
    if (ctx == NULL || f == NULL || opts == NULL || f->data == NULL)
        return PBGPU_EINVAL;
    if ((opts->flags & ~(PBGPU_STAMP_TAIL | PBGPU_STAMP_NO_CSUM)) || opts->offset > 65535u)
        return PBGPU_EINVAL;
    if (!stamps_fit(opts->first_index, n, opts->step_ps, opts->t0_ns))
        return PBGPU_EINVAL;
    uint64_t body = 0, end = 0;
    PBCHK(range_bytes(ctx, f, first_frame, n, &body, &end)); // the range check; variable length: offsets[] in place
    if (end > f->capacity_bytes)
        return PBGPU_EINVAL;
    if (res)
    {
        memset(res, 0, sizeof *res);
        res->n_in = n;
    }
    if (n == 0)
        return PBGPU_OK;
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx);
    hipStream_t st = ctx->stream;
    if (ctx->d_sp_res == nullptr)
        HIPCHK(hipMalloc((void **)&ctx->d_sp_res, PB_SP_RES_DW * sizeof(unsigned long long)));
    PBCHK(take_inplace(f, st, nullptr));
    pb_spargs A;
    memset(&A, 0, sizeof A);
    A.data = f->data;
    A.offsets = f->fixed_len ? nullptr : f->offsets;
    A.first = first_frame;
    A.n = n;
    A.fixed_len = f->fixed_len;
    A.offset = opts->offset;
    A.flags = ((opts->flags & PBGPU_STAMP_TAIL) ? PB_SP_TAIL : 0u) | ((opts->flags & PBGPU_STAMP_NO_CSUM) ? PB_SP_NO_CSUM : 0u);
    A.t0_ns = opts->t0_ns;
    A.step_ps = opts->step_ps;
    A.first_index = opts->first_index;
    A.res = ctx->d_sp_res;
    HIPCHK(hipMemsetAsync(ctx->d_sp_res, 0, PB_SP_RES_DW * sizeof(unsigned long long), st));
    timing_pair tp;
    PBCHK(timed_begin(ctx, &tp));
    HIPCHK(pbk_launch_stamp(&A, st));
    PBCHK(timed_stop(ctx, tp));
    unsigned long long r[PB_SP_RES_DW] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(r, ctx->d_sp_res, sizeof r, hipMemcpyDeviceToHost, st));
    float ms = 0;
    PBCHK(timed_ms(ctx, tp, &ms));
    if (r[0] + r[1] + r[2] != n)
        return PBGPU_EIO;
    if (res)
    {
        res->n_stamped = r[0];
        res->n_short = r[1];
        res->n_other = r[2];
        res->device_ms = ms;
    }
    return mark_built(ctx, f, st); // a later landing follows the stamp
}

// ---- IPv4-to-IPv6 translation ----

// Argument checks shared by pbgpu_xlat46_size and pbgpu_xlat46, then the frames' bytes (range_bytes).
static int xlat_check(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first, uint64_t n, const pbgpu_xlat_opts *opts,
                      uint64_t *body, uint64_t *src_end)
{
    if (ctx == NULL || src == NULL || opts == NULL || src->reserved == NULL)
        return PBGPU_EINVAL;
    if (opts->flow_label >= (1u << 20) || (opts->flags & ~PBGPU_XLAT_HASH_FLOW) || opts->reserved != 0)
        return PBGPU_EINVAL;
    const frames_events *fs = (const frames_events *)src->reserved;
    if (src->n_frames && fs->max_len > 65535u - PB_XL_ADD)
        return PBGPU_EINVAL;
    return range_bytes(ctx, src, first, n, body, src_end);
}

int pbgpu_xlat46_size(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n,
                      const pbgpu_xlat_opts *opts, uint64_t *frames, uint64_t *bytes)
{
    if (frames == NULL || bytes == NULL)
        return PBGPU_EINVAL;
    uint64_t body = 0, src_end = 0;
    PBCHK(xlat_check(ctx, src, first_frame, n, opts, &body, &src_end));
    *frames = n;
    *bytes = body + n * PB_XL_ADD;
    return PBGPU_OK;
}

int pbgpu_xlat46(pbgpu_ctx *ctx, pbgpu_frames *src, uint64_t first_frame, uint64_t n, const pbgpu_xlat_opts *opts,
                 pbgpu_frames *dst, pbgpu_xlat_result *res)
{
    if (ctx == NULL || src == NULL || opts == NULL || dst == NULL)
        return PBGPU_EINVAL;
    if (!ins_pair_ok(src, dst))
        return PBGPU_EINVAL;
    uint64_t body = 0, src_end = 0;
    PBCHK(xlat_check(ctx, src, first_frame, n, opts, &body, &src_end));
    pb_xlargs A;
    ins_args(&A, src, dst, first_frame, n, PB_XL_ADD);
    A.dst_offsets = dst->offsets;
    A.flags = (opts->flags & PBGPU_XLAT_HASH_FLOW) ? PB_XL_HASH : 0u;
    A.flow_label = opts->flow_label;
    uint8_t t[32]; // output bytes 20..51
    memset(t, 0, sizeof t);
    memcpy(t + 2, opts->src_prefix, 12);
    memcpy(t + 18, opts->dst_prefix, 12);
    for (int i = 0; i < 32; i += 2)
        A.ksum += ((uint32_t)t[i] << 8) | t[i + 1];
    while (A.ksum >> 16)
        A.ksum = (A.ksum & 0xFFFFu) + (A.ksum >> 16);
    pack_le32(A.tpl, t, 8);
    // The classify stage: its result is read before anything of dst is touched, and a frame that does
    // not translate refuses the call.  The timed stretch is classify and writer.
    auto classify = [&](ins_state &r) -> int {
        if (n > (uint64_t)0xFFFFFFFFu * (PB_XL_WT * PB_XL_ROWS))
            return PBGPU_EINVAL;
        if (res)
        {
            memset(res, 0, sizeof *res);
            res->n_in = n;
            res->first_other = UINT64_MAX;
        }
        if (n == 0)
            return PBGPU_OK;
        if (ctx->d_xl_res == nullptr)
            HIPCHK(hipMalloc((void **)&ctx->d_xl_res, PB_XL_RES_DW * sizeof(unsigned long long)));
        A.res = ctx->d_xl_res;
        A.end16 = r.end16;
        PBCHK(timed_begin(ctx, &r.tp));
        HIPCHK(pbk_launch_xlat(&A, 0, 0, r.st));
        unsigned long long c[PB_XL_RES_DW];
        HIPCHK(hipMemcpyAsync(c, ctx->d_xl_res, sizeof c, hipMemcpyDeviceToHost, r.st));
        HIPCHK(hipStreamSynchronize(r.st));
        if (c[0] + c[1] + c[2] + c[3] != n)
            return PBGPU_EIO;
        if (res)
        {
            res->n_udp = c[0];
            res->n_tcp = c[1];
            res->n_icmp = c[2];
            res->n_other = c[3];
            res->first_other = c[4];
        }
        if (c[3])
        {
            PBCHK(timed_stop(ctx, r.tp));
            PBCHK(timed_ms(ctx, r.tp, &r.ms));
            if (res)
                res->device_ms = r.ms;
            return PBGPU_EINVAL;
        }
        return PBGPU_OK; // every frame of the range is translatable: at least 42 B
    };
    ins_state r;
    PBCHK(ins_run(
        ctx, src, n, dst, body, src_end, 0u, PB_XL_ADD, true, classify,
        [&](ins_state &r) {
            A.per = r.per;
            return pbk_launch_xlat(&A, 1, r.grid, r.st); // variable length: dst->offsets by a launch of its own first
        },
        &r));
    if (res)
        res->device_ms = r.ms;
    return PBGPU_OK;
}

int pbgpu_host_register(pbgpu_ctx *ctx, void *ptr, size_t bytes)
{
    if (ctx == NULL || ptr == NULL)
        return PBGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipHostRegister(ptr, bytes, hipHostRegisterMapped));
    void *dev = NULL;
    if (hipHostGetDevicePointer(&dev, ptr, 0) == hipSuccess && dev != NULL)
        ctx->regs.push_back({(uint8_t *)ptr, bytes, (uint8_t *)dev});
    (void)hipGetLastError();
    return PBGPU_OK;
}

int pbgpu_host_unregister(pbgpu_ctx *ctx, void *ptr)
{
    if (ctx == NULL || ptr == NULL)
        return PBGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    int rc = pbgpu_land_wait(ctx, 0);
    if (rc != PBGPU_OK)
        return rc;
    for (size_t i = 0; i < ctx->regs.size(); ++i)
        if (ctx->regs[i].host == (uint8_t *)ptr)
        {
            ctx->regs.erase(ctx->regs.begin() + (long)i);
            break;
        }
    HIPCHK(hipHostUnregister(ptr));
    return PBGPU_OK;
}

// device address of [p, p + n) in a registered (mapped) range, or NULL
static uint8_t *mapped(pbgpu_ctx *ctx, uint8_t *p, uint64_t n)
{
    if (ctx->opt.umem_dma)
        return NULL;
    for (const auto &r : ctx->regs)
        if (p >= r.host && p + n <= r.host + r.bytes)
            return r.dev + (p - r.host);
    void *dev = NULL; // registered outside this context
    if (hipHostGetDevicePointer(&dev, p, 0) == hipSuccess && dev != NULL)
        return (uint8_t *)dev;
    (void)hipGetLastError();
    return NULL;
}

// Wait for a landing's event without paying a blocking wait's wake-up latency on short waits,
// and without holding a core for long ones (each TX thread waits this way; the GPU box gives a
// process a 16-CPU quota): poll for up to 50 us, then poll with sched_yield() between queries
// for up to 2 ms, then block in the runtime.
static double now_s()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static hipError_t spin_wait(hipEvent_t ev)
{
    hipError_t e;
    const double t0 = now_s();
    while ((e = hipEventQuery(ev)) == hipErrorNotReady)
    {
        const double dt = now_s() - t0;
        if (dt > 2e-3)
            return hipEventSynchronize(ev);
        if (dt > 50e-6)
            sched_yield();
    }
    return e;
}

int pbgpu_land_wait(pbgpu_ctx *ctx, uint32_t keep)
{
    if (ctx == NULL)
        return PBGPU_EINVAL;
    while (ctx->landings.size() > keep)
    {
        pbgpu_ctx::land_op op = ctx->landings.front();
        // a sender waits on every landing: poll the event rather than block in the runtime
        // (a blocking wait adds its wake-up latency to each landing; PBGPU_LAND_SPIN=0 blocks)
        hipError_t e = hipSuccess;
        if (ctx->opt.land_spin)
            e = spin_wait(op.ev);
        else
            e = hipEventSynchronize(op.ev);
        ctx->landings.pop_front();
        ctx->land_pool.push_back(op.ev);
        if (e != hipSuccess)
            return PBGPU_EIO;
        if (op.lens_out)
        {
            if (op.fixed_len)
                for (uint32_t i = 0; i < op.n; ++i)
                    op.lens_out[i] = (uint16_t)op.fixed_len;
            else
                memcpy(op.lens_out, ctx->h_lens + op.lens_off, (size_t)op.n * 2);
        }
    }
    return PBGPU_OK;
}

// Landing into memory that is not registered with HIP: the queued landings
// first (in order), then a strided DMA (fixed length) or a pinned staging copy.
static int land_unmapped(pbgpu_ctx *ctx, const pbgpu_frames *f, uint8_t *dst, uint32_t slot_stride,
                         uint64_t first_frame, uint32_t n, uint16_t *lens_out)
{
    PB_JOIN(ctx);
    int rc = pbgpu_land_wait(ctx, 0);
    if (rc != PBGPU_OK)
        return rc;
    hipStream_t ls = ctx->land_stream;
    if (f->fixed_len)
    {
        // strided DMA in runs of at most 32768 rows (a 2^18-row copy failed on the runtime)
        for (uint32_t i = 0; i < n; i += 32768)
        {
            const uint32_t rows = n - i < 32768 ? n - i : 32768;
            HIPCHK(hipMemcpy2DAsync(dst + (uint64_t)i * slot_stride, slot_stride,
                                    f->data + (first_frame + i) * f->fixed_len, f->fixed_len, f->fixed_len, rows,
                                    hipMemcpyDeviceToHost, ls));
        }
        HIPCHK(hipStreamSynchronize(ls));
        if (lens_out)
            for (uint32_t i = 0; i < n; ++i)
                lens_out[i] = (uint16_t)f->fixed_len;
        return PBGPU_OK;
    }
    std::vector<uint64_t> off(n + 1);
    HIPCHK(hipMemcpyAsync(off.data(), f->offsets + first_frame, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                          ls));
    HIPCHK(hipStreamSynchronize(ls));
    const uint64_t bytes = off[n] - off[0];
    if (ctx->h_stage_bytes < bytes)
    {
        if (ctx->h_stage)
            (void)hipHostFree(ctx->h_stage);
        ctx->h_stage = NULL;
        ctx->h_stage_bytes = 0;
        HIPCHK(hipHostMalloc((void **)&ctx->h_stage, bytes, 0));
        ctx->h_stage_bytes = bytes;
    }
    HIPCHK(hipMemcpyAsync(ctx->h_stage, f->data + off[0], bytes, hipMemcpyDeviceToHost, ls));
    HIPCHK(hipStreamSynchronize(ls));
    for (uint32_t i = 0; i < n; ++i)
    {
        const uint64_t len = off[i + 1] - off[i]; // <= slot_stride: the caller checked the buffer's longest frame
        memcpy(dst + (uint64_t)i * slot_stride, ctx->h_stage + (off[i] - off[0]), len);
        if (lens_out)
            lens_out[i] = (uint16_t)len;
    }
    return PBGPU_OK;
}

// send_packet()'s memcpy into UMEM slot idx * FRAME_SIZE, af_xdp.c:200-214.
// Registered (mapped) UMEM: a scatter kernel on the landing stream stores each
// frame into its slot over the host link, queued behind the build of these
// frames only; the caller waits with pbgpu_land_wait (several landings may be
// in flight: their launch and completion latencies overlap).  Unregistered
// memory: a synchronous strided DMA (fixed length) or pinned staging copy.
int pbgpu_copy_to_umem_async(pbgpu_ctx *ctx, const pbgpu_frames *f, void *umem, uint32_t slot_stride,
                             uint32_t first_slot, uint64_t first_frame, uint32_t n, uint16_t *lens_out)
{
    if (ctx == NULL || f == NULL || umem == NULL || slot_stride == 0 || first_frame + n > f->n_frames)
        return PBGPU_EINVAL;
    if (n == 0)
        return PBGPU_OK;
    // a frame longer than a slot would overrun the next slot (or, in the last slot,
    // the UMEM allocation): refused before anything is written, from the fixed length or
    // the longest frame recorded for the buffer by its build, upload or repack, never from
    // the sequence slot, which may hold another sequence by now (the reference does not
    // check, af_xdp.c:214)
    const frames_events *fu = (const frames_events *)f->reserved;
    if (f->fixed_len ? f->fixed_len > slot_stride : (fu == NULL || fu->max_len > slot_stride))
        return PBGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx);
    if (!f->fixed_len)
    {
        const int mrc = materialize_offsets(ctx, f);
        if (mrc != PBGPU_OK)
            return mrc;
    }
    hipStream_t ls = ctx->land_stream;
    ctx->land_events = true;
    frames_events *fe = (frames_events *)f->reserved;
    if (fe && fe->built)
        HIPCHK(hipStreamWaitEvent(ls, fe->built, 0));
    else
        HIPCHK(hipStreamSynchronize(ctx->stream));
    uint8_t *dst = (uint8_t *)umem + (uint64_t)first_slot * slot_stride;
    uint8_t *dev_dst = mapped(ctx, dst, (uint64_t)n * slot_stride);
    if (dev_dst == NULL)
        return land_unmapped(ctx, f, dst, slot_stride, first_frame, n, lens_out);
    pbgpu_ctx::land_op op = {nullptr, lens_out, n, 0, f->fixed_len};
    if (f->fixed_len && f->fixed_len >= ctx->opt.land_dma_min)
    {
        // PBGPU_LAND_DMA_MIN: the copy engine, a strided DMA on the landing stream, in runs of
        // <= 32768 rows (1500 B, 2^18 frames: 56.1 vs 52.2 GB/s for the scatter kernel landing
        // alone, 43.1 vs 49.2 in bench.py's build + land; at 64 B the engine moves 218 Mpps against
        // the kernel's 540, profiles/r06/d2h/)
        for (uint32_t i = 0; i < n; i += 32768)
        {
            const uint32_t rows = n - i < 32768 ? n - i : 32768;
            HIPCHK(hipMemcpy2DAsync(dst + (uint64_t)i * slot_stride, slot_stride,
                                    f->data + (first_frame + i) * f->fixed_len, f->fixed_len, f->fixed_len, rows,
                                    hipMemcpyDeviceToHost, ls));
        }
    }
    else if (f->fixed_len)
    {
        // a tight slot (no longer than the frame rounded up to 64 B, e.g. --umemslot 64 for 60- or
        // 64-B frames) is written whole: contiguous slots then reach the host as contiguous writes
        // (64 B: 783 Mpps into back-to-back slots against 535-541 for 64-B writes into 128-B to
        // 4-KiB slots, profiles/r06/d2h/d2h_slots.jsonl); otherwise only the frame's bytes
        const uint32_t r64 = (f->fixed_len + 63u) & ~63u;
        const uint32_t wlen = slot_stride <= r64 ? slot_stride : f->fixed_len;
        HIPCHK(pbk_launch_scatter_fixed(f->data + first_frame * f->fixed_len, f->fixed_len, wlen, n,
                                        f->capacity_bytes - first_frame * f->fixed_len, dev_dst, slot_stride, ls));
    }
    else
    {
        // lengths: a contiguous range of the context's ring (device + pinned host), FIFO
        // with the queued landings; never a stream-ordered allocation or a pageable copy
        if (ctx->lens_cap < n)
        {
            int rc = pbgpu_land_wait(ctx, 0);
            if (rc != PBGPU_OK)
                return rc;
            HIPCHK(hipStreamSynchronize(ls));
            if (ctx->d_lens)
                (void)hipFree(ctx->d_lens);
            if (ctx->h_lens)
                (void)hipHostFree(ctx->h_lens);
            ctx->d_lens = NULL;
            ctx->h_lens = NULL;
            ctx->lens_cap = 0;
            const uint32_t cap = n > (1u << 16) ? n : (1u << 16);
            HIPCHK(hipMalloc((void **)&ctx->d_lens, (size_t)cap * 2));
            HIPCHK(hipHostMalloc((void **)&ctx->h_lens, (size_t)cap * 2, 0));
            ctx->lens_cap = cap;
            ctx->lens_head = 0;
        }
        uint32_t off = ctx->lens_head + n <= ctx->lens_cap ? ctx->lens_head : 0;
        // wait for the queued landings whose ranges the new one would overwrite
        for (;;)
        {
            bool clash = false;
            for (const auto &q : ctx->landings)
                if (!q.fixed_len && q.lens_off < off + n && off < q.lens_off + q.n)
                    clash = true;
            if (!clash)
                break;
            int rc = pbgpu_land_wait(ctx, (uint32_t)ctx->landings.size() - 1);
            if (rc != PBGPU_OK)
                return rc;
        }
        HIPCHK(pbk_launch_scatter(f->data, f->offsets, first_frame, n, dev_dst, slot_stride, ctx->d_lens + off, ls));
        HIPCHK(hipMemcpyAsync(ctx->h_lens + off, ctx->d_lens + off, (size_t)n * 2, hipMemcpyDeviceToHost, ls));
        op.lens_off = off;
        ctx->lens_head = off + n;
    }
    if (!ctx->land_pool.empty())
    {
        op.ev = ctx->land_pool.back();
        ctx->land_pool.pop_back();
    }
    else
        HIPCHK(hipEventCreateWithFlags(&op.ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(op.ev, ls));
    ctx->landings.push_back(op);
    // the next pbgpu_build into this buffer waits for the landing (pbgpu.h)
    frames_events *fw = frames_ev(const_cast<pbgpu_frames *>(f));
    if (fw == NULL)
        return PBGPU_ENOMEM;
    if (fw->landed == nullptr)
        HIPCHK(hipEventCreateWithFlags(&fw->landed, hipEventDisableTiming));
    HIPCHK(hipEventRecord(fw->landed, ls));
    fw->land_pending = true;
    return PBGPU_OK;
}

int pbgpu_copy_to_umem(pbgpu_ctx *ctx, const pbgpu_frames *f, void *umem, uint32_t slot_stride, uint32_t first_slot,
                       uint64_t first_frame, uint32_t n, uint16_t *lens_out)
{
    int rc = pbgpu_copy_to_umem_async(ctx, f, umem, slot_stride, first_slot, first_frame, n, lens_out);
    if (rc == PBGPU_OK)
        rc = pbgpu_land_wait(ctx, 0);
    return rc;
}

// A slot's device counters: the shards' sums; fixed-length kernels add only the bytes they
// stored (one atomic per workgroup: each is a memory-side transaction, 0.4-1% of a small-frame
// launch's traffic as two), so their frames are bytes / length.
// sum: slot i's shard sums {frames, bytes} (read_counter_sums)
static void slot_counts(const pbgpu_ctx *ctx, const unsigned long long *sum, int i, uint64_t *p, uint64_t *b)
{
    uint64_t pp = sum[0], bb = sum[1];
    const seq_slot &S = ctx->seqs[i];
    if (S.loaded && S.K.fixed_len)
        pp = bb / S.K.fixed_len;
    *p = pp + ctx->ctr_base[i][0];
    *b = bb + ctx->ctr_base[i][1];
}

// Slots [first, first + n_seq)'s shard sums into ctx->h_ctr_sum[2 (i - first) ..], by a kernel
// writing the mapped host buffer (on ctx->stream, after everything issued there), then a stream
// synchronisation.  A pageable hipMemcpy of the shards instead (8 KiB per slot) cost 8-16 ms on
// its first use for three slots, an idle gap before bench.py's timed configs[4] steps that cost
// their first 25 launches up to 30% (profiles/r05/ab/gap.log, profiles/r05/prof/cfg/trace_c5_mix*)
static int read_counter_sums(pbgpu_ctx *ctx, int first, int n_seq)
{
    HIPCHK(pbk_launch_ctr_read(ctx->d_counters + PB_CTR_WORDS * (size_t)first, (uint32_t)n_seq,
                               ctx->d_ctr_sum, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBGPU_OK;
}

int pbgpu_counters(pbgpu_ctx *ctx, uint64_t *pckts, uint64_t *bytes, int n_seq)
{
    if (ctx == NULL || n_seq < 0 || n_seq > PB_MAX_SEQUENCES)
        return PBGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx);
    if (n_seq == 0)
        return PBGPU_OK;
    // the launches' pending per-workgroup records first, then the shards' sums
    for (int i = 0; i < n_seq; ++i)
    {
        const int frc = ctr_fold(ctx, i, ctx->stream);
        if (frc != PBGPU_OK)
            return frc;
    }
    const int rrc = read_counter_sums(ctx, 0, n_seq);
    if (rrc != PBGPU_OK)
        return rrc;
    for (int i = 0; i < n_seq; ++i)
    {
        uint64_t p = 0, b = 0;
        slot_counts(ctx, ctx->h_ctr_sum + 2 * i, i, &p, &b);
        if (pckts)
            pckts[i] = p;
        if (bytes)
            bytes[i] = b;
    }
    return PBGPU_OK;
}

int pbgpu_set_timing(pbgpu_ctx *ctx, int mode)
{
    if (ctx == NULL || (mode != PBGPU_TIMING_LAUNCH && mode != PBGPU_TIMING_SPAN))
        return PBGPU_EINVAL;
    double ms; // close what the old mode measured
    uint32_t n;
    const int rc = pbgpu_kernel_time(ctx, &ms, &n);
    if (rc)
        return rc;
    ctx->timing_mode = mode;
    return PBGPU_OK;
}

int pbgpu_kernel_time(pbgpu_ctx *ctx, double *ms_total, uint32_t *n_launches)
{
    if (ctx == NULL)
        return PBGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx); // the span ends after every sequence stream's launches
    double tot = 0;
    uint32_t n = 0;
    if (ctx->span_n)
    {
        HIPCHK(hipEventRecord(ctx->span.b, ctx->stream));
        HIPCHK(hipEventSynchronize(ctx->span.b));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ctx->span.a, ctx->span.b));
        tot += ms;
        n += ctx->span_n;
        ctx->span_n = 0;
    }
    for (auto &p : ctx->pending)
    {
        HIPCHK(hipEventSynchronize(p.b));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, p.a, p.b));
        tot += ms;
        ++n;
        ctx->pool.push_back(p);
    }
    ctx->pending.clear();
    if (ms_total)
        *ms_total = tot;
    if (n_launches)
        *n_launches = n;
    return PBGPU_OK;
}

int pbgpu_kernel_times(pbgpu_ctx *ctx, double *ms_each, uint32_t cap, uint32_t *n_launches)
{
    if (ctx == NULL || (cap && ms_each == NULL))
        return PBGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx);
    uint32_t n = 0;
    for (auto &p : ctx->pending)
    {
        HIPCHK(hipEventSynchronize(p.b));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, p.a, p.b));
        if (n < cap)
            ms_each[n] = ms;
        ++n;
        ctx->pool.push_back(p);
    }
    ctx->pending.clear();
    if (n_launches)
        *n_launches = n;
    return PBGPU_OK;
}

static int fill_probe_buf(pbgpu_ctx *ctx, void *buf, uint64_t bytes, uint32_t reps, double *ms_per_shape,
                          int *best_shape);

int pbgpu_fill_probe_ex(pbgpu_ctx *ctx, uint64_t bytes, uint32_t reps, double *ms_per_shape, int *best_shape)
{
    if (ctx == NULL || bytes < 16 || reps == 0)
        return PBGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx);
    void *buf = NULL;
    HIPCHK(hipMalloc(&buf, bytes));
    const int rc = fill_probe_buf(ctx, buf, bytes, reps, ms_per_shape, best_shape);
    (void)hipFree(buf);
    return rc;
}

int pbgpu_fill_probe_at(pbgpu_ctx *ctx, void *dst, uint64_t bytes, uint32_t reps, double *ms_per_shape)
{
    if (ctx == NULL || dst == NULL || bytes < 16 || reps == 0)
        return PBGPU_EINVAL;
    HIPCHK(hipSetDevice(ctx->device));
    PB_JOIN(ctx);
    return fill_probe_buf(ctx, dst, bytes, reps, ms_per_shape, NULL);
}

static int fill_probe_buf(pbgpu_ctx *ctx, void *buf, uint64_t bytes, uint32_t reps, double *ms_per_shape,
                          int *best_shape)
{
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    double best = 1e30;
    int bi = 0;
    for (int mode = 0; mode < PBGPU_FILL_SHAPES; ++mode) // pbk_launch_fill's shapes; the fastest is the peak
    {
        double mode_best = 1e30;
        for (int trial = 0; trial < 2; ++trial)
        {
            HIPCHK(pbk_launch_fill(buf, bytes, mode, ctx->stream)); // warm-up
            HIPCHK(hipEventRecord(a, ctx->stream));
            for (uint32_t r = 0; r < reps; ++r)
                HIPCHK(pbk_launch_fill(buf, bytes, mode, ctx->stream));
            HIPCHK(hipEventRecord(b, ctx->stream));
            HIPCHK(hipEventSynchronize(b));
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, a, b));
            mode_best = ms / reps < mode_best ? ms / reps : mode_best;
        }
        if (ms_per_shape)
            ms_per_shape[mode] = mode_best;
        if (mode_best < best)
            best = mode_best, bi = mode;
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    if (best_shape)
        *best_shape = bi;
    return PBGPU_OK;
}

int pbgpu_fill_probe(pbgpu_ctx *ctx, uint64_t bytes, uint32_t reps, double *ms_per_launch)
{
    double ms[PBGPU_FILL_SHAPES];
    int bi = 0;
    const int rc = pbgpu_fill_probe_ex(ctx, bytes, reps, ms, &bi);
    if (rc == PBGPU_OK && ms_per_launch)
        *ms_per_launch = ms[bi];
    return rc;
}

const char *pbgpu_fill_shape_name(int shape)
{
    return pbk_fill_shape_name(shape);
}

int pbgpu_kernel_name(pbgpu_ctx *ctx, uint16_t seq_idx, char *buf, size_t n)
{
    if (ctx == NULL || seq_idx >= PB_MAX_SEQUENCES || buf == NULL || n == 0)
        return PBGPU_EINVAL;
    const seq_slot &S = ctx->seqs[seq_idx];
    if (!S.loaded)
        return PBGPU_ENOENT;
    pb_plan_name(S.plan, S.K, buf, n);
    return PBGPU_OK;
}

// Test hook: what pbgpu_load_sequence would choose for this sequence under the present PBGPU_*
// environment, as one line (pb_plan_describe); no context and no device
int pbgpu_plan_describe(uint16_t seq_idx, const pb_sequence_t *seq, const pb_rules_t *rules, uint64_t seed_base,
                        char *buf, size_t n)
{
    if (seq == NULL || seq_idx >= PB_MAX_SEQUENCES || buf == NULL || n == 0)
        return PBGPU_EINVAL;
    const pb_opts O = read_opts();
    pb_compiled C;
    const int rc = pb_compile(seq_idx, seq, NULL, NULL, rules, seed_base, &C);
    if (rc != PBGPU_OK)
        return rc;
    const pb_plan P = pb_make_plan(C, O);
    pb_plan_describe(C, P, O, pbk_batch_kind(&C.K), buf, n);
    return PBGPU_OK;
}

size_t pbgpu_abi_size(int which)
{
    switch (which)
    {
    case 0: return sizeof(pb_sequence_t);
    case 1: return sizeof(pb_payload_opt_t);
    case 2: return sizeof(pbgpu_frames);
    case 3: return offsetof(pb_sequence_t, ip.ranges);
    case 4: return offsetof(pb_sequence_t, pls);
    case 5: return offsetof(pb_sequence_t, pl_cnt);
    case 6: return offsetof(pbgpu_frames, total_bytes);
    case 7: return sizeof(pbgpu_verify_result);
    case 8: return sizeof(pbgpu_pcap_opts);
    case 9: return sizeof(pbgpu_encap_opts);
    case 10: return sizeof(pbgpu_frag_opts);
    case 11: return sizeof(pbgpu_frag_result);
    case 18: return sizeof(pbgpu_seg_opts);
    case 19: return sizeof(pbgpu_seg_result);
    case 12: return sizeof(pbgpu_stamp_opts);
    case 13: return sizeof(pbgpu_stamp_result);
    case 14: return sizeof(pbgpu_xlat_opts);
    case 15: return sizeof(pbgpu_xlat_result);
    case 16: return sizeof(pbgpu_wire_opts);
    case 17: return sizeof(pbgpu_wire_result);
    default: return 0;
    }
}

} // extern "C"
