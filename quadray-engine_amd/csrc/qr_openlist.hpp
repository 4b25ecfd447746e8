/*
 * The open list of an adaptive path-traced ray state (include/qrhip.h qr_pt_adapt_open_list_async): the indices of the rays the
 * stop rule would still let take a sample, in ascending order, and their number -- built on chip, so that qr_pt_list_kernel
 * (qr_kernel.hpp) fills its waves with open rays only.  Three small launches on one stream and nothing else:
 *   qr_open_count_kernel    one count per block of QR_PT_OPEN_BLOCK rays: per wave the rule's ballot and its population count,
 *                           the block's waves combined through LDS
 *   qr_open_scan_kernel     ONE workgroup turns the counts into exclusive offsets in place, QR_PT_OPEN_CHUNK at a time with a
 *                           carried total, and stores the total: the list's length
 *   qr_open_scatter_kernel  the rule again; a lane's position is the block's offset + the offsets of the waves before its own
 *                           (LDS) + its rank among the wave's open lanes (mbcnt of the ballot below it)
 * The list is a pure function of the state: no atomic, so no order left to the hardware; and no workgroup waits for another -- the
 * stream orders the launches -- so there is nothing that can spin.  The state is only read.  Every store is a vector store.
 */
#pragma once

static_assert(QR_PT_OPEN_BLOCK % 64 == 0 && QR_PT_OPEN_BLOCK >= 64 && QR_PT_OPEN_BLOCK <= 1024, "whole waves, one workgroup");
static_assert(QR_PT_OPEN_CHUNK % 64 == 0 && QR_PT_OPEN_CHUNK >= 64 && QR_PT_OPEN_CHUNK <= 1024, "whole waves, one workgroup");

/* the stop rule of qr_pt_adapt_rays_async (pt_adapt_rule, qr_kernel.hpp) on column i of the state in memory (planes 4..7) */
__device__ __forceinline__ bool qr_open_rule(const u32 *__restrict__ state, size_t n, size_t i, u32 min_samples, u32 max_samples,
                                             float tol2)
{
    const u32 m = state[4 * n + i];
    const float m2r = u2f(state[5 * n + i]), m2g = u2f(state[6 * n + i]), m2b = u2f(state[7 * n + i]);
    return pt_adapt_rule(m, m2r, m2g, m2b, min_samples, max_samples, tol2);
}

__global__ __launch_bounds__(QR_PT_OPEN_BLOCK)
void qr_open_count_kernel(const u32 *__restrict__ state, u32 n, u32 min_samples, u32 max_samples, float tol2, u32 *__restrict__ counts)
{
    __shared__ u32 lds_wave[QR_PT_OPEN_BLOCK / 64];
    const u32 tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const size_t i = (size_t)blockIdx.x * QR_PT_OPEN_BLOCK + tid;
    const bool op = i < n && qr_open_rule(state, n, i, min_samples, max_samples, tol2);
    const unsigned long long b = __ballot(op);
    if (lane == 0u) lds_wave[wave] = (u32)__popcll(b);
    __syncthreads();
    if (tid == 0u)
    {
        u32 t = 0u;
#pragma unroll
        for (int w = 0; w < QR_PT_OPEN_BLOCK / 64; w++) t += lds_wave[w];
        counts[blockIdx.x] = t;
    }
}

/* counts[0 .. nb) -> their exclusive prefix sums, in place; *total = their sum.  One workgroup of QR_PT_OPEN_CHUNK threads */
__global__ __launch_bounds__(QR_PT_OPEN_CHUNK)
void qr_open_scan_kernel(u32 *__restrict__ counts, u32 nb, u32 *__restrict__ total)
{
    __shared__ u32 lds_wave[QR_PT_OPEN_CHUNK / 64];
    const u32 tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    u32 carry = 0u;                                         /* the same in every thread */
    for (u32 base = 0u; base < nb; base += QR_PT_OPEN_CHUNK)
    {
        const u32 j = base + tid;
        const u32 v = j < nb ? counts[j] : 0u;
        u32 incl = v;                                       /* inclusive scan inside the wave */
#pragma unroll
        for (int d = 1; d < 64; d <<= 1)
        {
            const u32 up = (u32)__shfl_up((int)incl, d);
            if (lane >= (u32)d) incl += up;
        }
        if (lane == 63u) lds_wave[wave] = incl;
        __syncthreads();
        u32 before = 0u, all = 0u;
#pragma unroll
        for (u32 w = 0; w < QR_PT_OPEN_CHUNK / 64; w++)
        {
            const u32 t = lds_wave[w];
            if (w < wave) before += t;
            all += t;
        }
        if (j < nb) counts[j] = carry + before + (incl - v);
        carry += all;
        __syncthreads();                                    /* lds_wave is written again in the next pass */
    }
    if (tid == 0u) *total = carry;
}

__global__ __launch_bounds__(QR_PT_OPEN_BLOCK)
void qr_open_scatter_kernel(const u32 *__restrict__ state, u32 n, u32 min_samples, u32 max_samples, float tol2,
                            const u32 *__restrict__ offsets, u32 *__restrict__ index)
{
    __shared__ u32 lds_wave[QR_PT_OPEN_BLOCK / 64];
    const u32 tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const size_t i = (size_t)blockIdx.x * QR_PT_OPEN_BLOCK + tid;
    const bool op = i < n && qr_open_rule(state, n, i, min_samples, max_samples, tol2);
    const unsigned long long b = __ballot(op);
    if (lane == 0u) lds_wave[wave] = (u32)__popcll(b);
    __syncthreads();
    u32 pos = offsets[blockIdx.x];
#pragma unroll
    for (u32 w = 0; w < QR_PT_OPEN_BLOCK / 64; w++) if (w < wave) pos += lds_wave[w];
    pos += __builtin_amdgcn_mbcnt_hi((u32)(b >> 32), __builtin_amdgcn_mbcnt_lo((u32)b, 0u));
    /* pos < n whenever the state is the one the counts were taken from; a state changed in between must not write past the list */
    if (op && pos < n) index[pos] = (u32)i;
}
