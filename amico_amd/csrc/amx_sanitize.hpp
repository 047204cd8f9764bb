// amx_sanitize.hpp -- what the kernels that count NaN / Inf elements share (amx_sanitize.hip, amx_ingest.hip): the block reduction of
// the per-lane counts, the ctx's two counters (one taken per call, zeroed on the call's stream, copied to pinned memory behind the
// kernel), the grid of a streaming pass and the test for a plan whose image is a permutation of a contiguous block.
#pragma once
#include "amx_host.hpp"

namespace amx {

// block sum of per-lane counts -> one atomicAdd (none when the block found nothing)
__device__ __forceinline__ void san_block_add(unsigned int mine, unsigned long long *counter)
{
    __shared__ unsigned int part[4];
    unsigned int w = mine;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) w += __shfl_down(w, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long tot = (unsigned long long)part[0] + part[1] + part[2] + part[3];
        if (tot) atomicAdd(counter, tot);
    }
}

// the counter and the event of this call; the launch function zeroes the counter on the call's stream
inline int san_begin(amx_ctx *ctx, hipStream_t s, unsigned long long **counter)
{
    if (!ctx->san_count) {
        HIPCHK(ctx, hipMalloc((void **)&ctx->san_count, 2 * sizeof(unsigned long long)));
        HIPCHK(ctx, hipHostMalloc((void **)&ctx->san_host, 2 * sizeof(unsigned long long)));
        ctx->san_host[0] = ctx->san_host[1] = 0;
        for (int k = 0; k < 2; k++) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->san_ev[k], hipEventDisableTiming));
    }
    const int slot = (int)(ctx->san_seq & 1u);
    *counter = ctx->san_count + slot;
    HIPCHK(ctx, hipMemsetAsync(*counter, 0, sizeof(unsigned long long), s));
    return AMX_OK;
}

inline int san_end(amx_ctx *ctx, hipStream_t s, const char *kernel)
{
    HIPCHK(ctx, hipGetLastError());
    // the count goes home behind the kernel, into pinned memory: reading it is a wait for the event and a load, not a blocking copy
    const unsigned slot = ctx->san_seq & 1u;
    HIPCHK(ctx, hipMemcpyAsync(ctx->san_host + slot, ctx->san_count + slot, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipEventRecord(ctx->san_ev[slot], s));      // amx_sanitize_last waits for this, not for the caller's stream
    ctx->san_seq++;
    amx_note(ctx, kernel);
    return AMX_OK;
}

inline unsigned san_grid(const amx_ctx *ctx, long long items)
{
    long long grid = (items + 255) / 256;
    const long long cap = (long long)ctx->n_cu * 8;
    if (grid > cap) grid = cap;
    return (unsigned)(grid < 1 ? 1 : grid);
}

// the four (extent, stride) pairs of a plan's image sorted by stride, axes of extent 1 dropped; dense: together they tile a contiguous block
inline bool san_axes(const amx_prep *p, long long d[4], long long st[4])
{
    long long dd[4] = {p->d[0], p->d[1], p->d[2], (long long)p->nS}, ss[4] = {p->s[0], p->s[1], p->s[2], p->sv};
    int n = 0;
    for (int k = 0; k < 4; k++) {
        if (dd[k] == 1) continue;
        int j = n++;
        for (; j > 0 && st[j - 1] > ss[k]; j--) { st[j] = st[j - 1]; d[j] = d[j - 1]; }
        st[j] = ss[k]; d[j] = dd[k];
    }
    bool dense = true;
    long long expect = 1;
    for (int k = 0; k < n; k++) { if (st[k] != expect) dense = false; expect *= d[k]; }
    for (int k = n; k < 4; k++) { d[k] = 1; st[k] = 0; }
    return dense;
}

}  // namespace amx
