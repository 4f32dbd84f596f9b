/*
 * stamp_host.c — the host method pbgpu_stamp replaces, for scripts/stamp_bench.py: the definition in
 * include/pbgpu.h applied to a packed buffer in host memory by `nthreads` threads, each a contiguous
 * share of the frames.  Byte by byte in the definition's own (big-endian) terms; shares no code with
 * the kernel.  Built by the benchmark itself: gcc -O2 -shared -fPIC -pthread.
 */
#include <pthread.h>
#include <stdint.h>
#include <string.h>

typedef struct job
{
    uint8_t *data;
    const uint64_t *offsets; /* NULL: fixed length */
    uint32_t fixed_len, offset, flags;
    uint64_t j0, j1, t0_ns, step_ps, first_index;
    uint64_t counts[3]; /* stamped, short, other */
} job_t;

static int stamp_one(uint8_t *F, uint32_t L, uint64_t idx, uint64_t T, uint32_t offset, uint32_t flags)
{
    if (L < 34 || F[12] != 0x08 || F[13] != 0x00 || F[14] != 0x45 || (((F[20] << 8) | F[21]) & 0x3FFF))
        return 2;
    const uint8_t proto = F[23];
    if (proto != 1 && proto != 6 && proto != 17)
        return 2;
    uint32_t H = 8, Q = proto == 17 ? 40 : 36;
    if (proto == 6)
    {
        if (L < 47)
            return 1;
        H = 4u * (F[46] >> 4);
        Q = 50;
        if (H < 20)
            return 2;
    }
    const int64_t P0 = 34 + H, S = (flags & 1u) ? (int64_t)L - 16 - offset : P0 + offset;
    if (S < P0 || S + 16 > L)
        return 1;
    uint8_t nw[16];
    for (int i = 0; i < 8; ++i)
    {
        nw[i] = (uint8_t)(idx >> (56 - 8 * i));
        nw[8 + i] = (uint8_t)(T >> (56 - 8 * i));
    }
    if (!(flags & 2u))
    {
        uint32_t s = ~(((uint32_t)F[Q] << 8) | F[Q + 1]) & 0xFFFFu;
        for (int64_t w = S & ~(int64_t)1; w < S + 16; w += 2) /* the words that intersect [S, S + 16) */
        {
            const uint32_t ohi = F[w], olo = w + 1 < L ? F[w + 1] : 0;
            const uint32_t nhi = w >= S ? nw[w - S] : ohi, nlo = w + 1 < S + 16 ? nw[w + 1 - S] : olo;
            s += (~((ohi << 8) | olo) & 0xFFFFu) + ((nhi << 8) | nlo);
        }
        while (s >> 16)
            s = (s & 0xFFFFu) + (s >> 16);
        s = ~s & 0xFFFFu;
        F[Q] = (uint8_t)(s >> 8);
        F[Q + 1] = (uint8_t)s;
    }
    memcpy(F + S, nw, 16);
    return 0;
}

static void *worker(void *p)
{
    job_t *J = (job_t *)p;
    for (uint64_t j = J->j0; j < J->j1; ++j)
    {
        const uint64_t o = J->offsets ? J->offsets[j] : j * J->fixed_len;
        const uint32_t L = J->offsets ? (uint32_t)(J->offsets[j + 1] - o) : J->fixed_len;
        const uint64_t idx = J->first_index + j;
        J->counts[stamp_one(J->data + o, L, idx, J->t0_ns + idx * J->step_ps / 1000u, J->offset, J->flags)]++;
    }
    return NULL;
}

/* Frames [0, n) of data; offsets has n + 1 entries relative to data, or is NULL with fixed_len. */
int stamp_host(uint8_t *data, const uint64_t *offsets, uint32_t fixed_len, uint64_t n, uint64_t t0_ns,
               uint64_t step_ps, uint64_t first_index, uint32_t offset, uint32_t flags, int nthreads, uint64_t *counts)
{
    if (nthreads < 1 || nthreads > 64)
        return -1;
    pthread_t th[64];
    job_t jobs[64];
    for (int t = 0; t < nthreads; ++t)
    {
        job_t J = {data, offsets, fixed_len, offset, flags, n * t / nthreads, n * (t + 1) / nthreads,
                   t0_ns, step_ps, first_index, {0, 0, 0}};
        jobs[t] = J;
        if (pthread_create(&th[t], NULL, worker, &jobs[t]) != 0)
            return -1;
    }
    counts[0] = counts[1] = counts[2] = 0;
    for (int t = 0; t < nthreads; ++t)
    {
        pthread_join(th[t], NULL);
        for (int k = 0; k < 3; ++k)
            counts[k] += jobs[t].counts[k];
    }
    return 0;
}
