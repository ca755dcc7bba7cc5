// opnet_stream_x4_kernels.hip - gfx950 boundary kernels of a stream step that runs as ONE persistent launch of the 4-clip form
// (opnet_stream_step_x4_f32): opnet_xcd4_forward<false, true> between a prologue and a write-back, as opnet_stream_kernels.hip
// puts the launch chain's step kernel between its two.
//
// Where a stream's state is around the persistent launch of T = k frames (opnet_xcd4_kernels.hip; stream b of the call is clip
// b: row block rb = b / 32, group gg = rb * 8 + (b & 31) / 4 - XCD (b & 31) / 4 -, column j = b & 3):
//   in  : h1 / h2 of "step -1" = slot 0 of the exchange rings h1x / h2x, [group][slot][unit quad][4 clips] float4 - the slot phase 0
//         gathers (h1: s & 3, h2: (s + 2) & 3 at s = 2), where opnet_xcd4_init puts zeros; c1 / c2 = the cs1 / cs2 staging buffers,
//         [group][unit][4 clips] float, which the forward loads into LDS in place of its zero fill;
//   out : h1 of step T-1 = h1x slot T & 3 (published at (s + 1) & 3 in phase s = T-1; that slot was last re-armed in phase T-3, and
//         phases >= T run no LSTM1 cell); h2 of step T-1 = slot T of the h2 history (what opnet_xcd4_out_head reads); c1 / c2 = cs1 /
//         cs2 again, stored by the cell waves behind the phase loop.
// The prologue's stores reach the persistent launch, and that launch's plain (XCD-local when the placement check passed) stores
// reach the write-back, across a kernel boundary each - the same hand-off opnet_xcd4_init and opnet_xcd4_out_head rely on.
// All of it is fp32 copies: a stream's frames see the arithmetic of the whole-clip 4-clip forward whatever the chunking.
#pragma once

struct StreamX4Args {
    Xcd4Args x;              // the persistent launch's arguments for B = n clips, T = k frames
    const float *boxes;      // [n][k][90]
    const int32_t *slots;    // [n] pool rows, distinct, in [0, capacity)
    float *state;            // [capacity][2*H1 + 2*H2] = [h1 | c1 | h2 | c2]
    float *y;                // [n][k][4]
    float *logits;           // [n][15][k]
    long capacity;
};

#define SX4_ROW (2 * XCD_H1 + 2 * XCD_H2)      // floats in a pool row
#define SX4_GATHER 16                            // state workgroups per row block in the prologue

__device__ __forceinline__ const float *stream_x4_row(const StreamX4Args &s, int b)
{
    if (b >= s.x.B) return nullptr;
    const long slot = s.slots[b];
    // a slot outside the pool is a caller bug the host checks catch; here it must not turn into a wild access
    if (slot < 0 || slot >= s.capacity) return nullptr;
    return s.state + slot * (long)SX4_ROW;
}

// A ring word with the sentinel's bits would never count as published: every consumer would spin to the limit and the launch
// would give up.  It is a NaN either way, so a state word (h or c) with those bits enters the launch as the canonical one.
__device__ __forceinline__ unsigned stream_x4_word(float v)
{
    const unsigned u = __float_as_uint(v);
    return u == X4_SENT ? 0x7fc00000u : u;
}

// grid (k + SX4_GATHER, RB) x 256.  Workgroups x < k pack frame x of row block y (opnet_pack_input).  The others do, for the 8
// groups of row block y, what opnet_xcd4_init does for all - status words, ring slots 1..3 unpublished - except that ring slot 0
// holds each named stream's h1 / h2 and cs1 / cs2 its c1 / c2 (stream_x4_word); columns beyond n and ids outside the pool get zeros.
__global__ void __launch_bounds__(256) opnet_stream_x4_prologue(const StreamX4Args s)
{
    const Xcd4Args &a = s.x;
    const int rb = blockIdx.y;
    if ((int)blockIdx.x < a.T) {
        OpnetIO io = {};
        io.B = a.B; io.T = a.T; io.RB = a.RB;
        io.boxes = s.boxes;
        io.xp = (float4 *)(a.ws + a.xp_off);      // io.state_f4 = 0: nothing to zero
        pack_input_body(&io, blockIdx.x, rb, a.RB);
        return;
    }
    const int tid = (blockIdx.x - a.T) * 256 + threadIdx.x, nth = SX4_GATHER * 256;
    if (rb == 0) {
        if (tid < 8) a.status[tid] = 0u;
        for (int i = tid; i < 256; i += nth) a.status[8 + i] = 0xffffffffu;
    }
    const xcd_u32x4 z = {0u, 0u, 0u, 0u}, sent = {X4_SENT, X4_SENT, X4_SENT, X4_SENT};
    constexpr int Q1 = XCD_H1 / 4, Q2 = XCD_H2 / 4;
    // rings: item = (group g of the row block, slot, unit quad q, clip j)
    xcd_u32x4 *h1x = (xcd_u32x4 *)(a.ws + a.h1x_off) + (size_t)rb * 8 * X4_SLOTS * (Q1 * 4);
    xcd_u32x4 *h2x = (xcd_u32x4 *)(a.ws + a.h2x_off) + (size_t)rb * 8 * X4_SLOTS * (Q2 * 4);
    for (int i = tid; i < 8 * X4_SLOTS * (Q1 * 4 + Q2 * 4); i += nth) {
        const bool l1 = i < 8 * X4_SLOTS * Q1 * 4;
        const int e = l1 ? i : i - 8 * X4_SLOTS * Q1 * 4, Q = l1 ? Q1 : Q2;
        const int j = e & 3, q = (e >> 2) % Q, slot = ((e >> 2) / Q) & (X4_SLOTS - 1), g = (e >> 2) / (Q * X4_SLOTS);
        xcd_u32x4 v = sent;
        if (slot == 0) {
            v = z;
            const float *row = stream_x4_row(s, rb * 32 + g * 4 + j);
            if (row) {
                const float4 h = *(const float4 *)(row + (l1 ? 0 : 2 * XCD_H1) + 4 * q);
                v.x = stream_x4_word(h.x); v.y = stream_x4_word(h.y); v.z = stream_x4_word(h.z); v.w = stream_x4_word(h.w);
            }
        }
        (l1 ? h1x : h2x)[e] = v;
    }
    // cell states: item = (group g, unit quad q, clip j) -> four floats of [group][unit][4 clips]
    float *cs1 = (float *)(a.ws + a.cs1_off) + (size_t)rb * 8 * XCD_H1 * 4;
    float *cs2 = (float *)(a.ws + a.cs2_off) + (size_t)rb * 8 * XCD_H2 * 4;
    for (int i = tid; i < 8 * (Q1 + Q2) * 4; i += nth) {
        const bool l1 = i < 8 * Q1 * 4;
        const int e = l1 ? i : i - 8 * Q1 * 4, Q = l1 ? Q1 : Q2, H = l1 ? XCD_H1 : XCD_H2;
        const int j = e & 3, q = (e >> 2) % Q, g = (e >> 2) / Q;
        float4 cv = make_float4(0.f, 0.f, 0.f, 0.f);
        const float *row = stream_x4_row(s, rb * 32 + g * 4 + j);
        if (row) cv = *(const float4 *)(row + (l1 ? XCD_H1 : 2 * XCD_H1 + XCD_H2) + 4 * q);
        // c never enters a ring itself, but h = o * tanh(c') does, and a NaN operand hands its payload on: the same canonical NaN
        float *dst = (l1 ? cs1 : cs2) + ((size_t)g * H + 4 * q) * 4 + j;
        dst[0] = __uint_as_float(stream_x4_word(cv.x));
        dst[4] = __uint_as_float(stream_x4_word(cv.y));
        dst[8] = __uint_as_float(stream_x4_word(cv.z));
        dst[12] = __uint_as_float(stream_x4_word(cv.w));
    }
}

// 1-D grid-stride, behind opnet_xcd4_out_head.  A launch that completed (status[0] == 0): every named stream's pool row gets its
// state after frame k-1, and y / logits go from the staging buffers to the caller's tensors (opnet_copy_out).  A launch that gave
// up: the pool rows keep the state from before the call - so the caller can run the same call again - and y / logits are NaN.
// Rows the call does not name are never touched.
__global__ void __launch_bounds__(256) opnet_stream_x4_writeback(const StreamX4Args s)
{
    const Xcd4Args &a = s.x;
    const int k = a.T;
    const bool ok = a.status[0] == 0u;
    constexpr int Q1 = XCD_H1 / 4, Q2 = XCD_H2 / 4, Q = Q1 + Q2;
    const long stride = (long)gridDim.x * blockDim.x;
    const long i0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long nst = ok ? (long)a.RB * Q * 32 : 0;
    const float4 *h1x = (const float4 *)(a.ws + a.h1x_off), *h2h = (const float4 *)(a.ws + a.h2_off);
    const float *cs1 = (const float *)(a.ws + a.cs1_off), *cs2 = (const float *)(a.ws + a.cs2_off);
    for (long i = i0; i < nst; i += stride) {
        const int clip = i & 31;
        const long rq = i >> 5;
        const int q = rq % Q, rb = rq / Q;
        float *row = (float *)stream_x4_row(s, rb * 32 + clip);
        if (!row) continue;
        const int gg = rb * 8 + (clip >> 2), j = clip & 3;
        if (q < Q1) {
            const float *c = cs1 + ((size_t)gg * XCD_H1 + 4 * q) * 4 + j;
            *(float4 *)(row + 4 * q) = h1x[((size_t)gg * X4_SLOTS + (k & 3)) * (Q1 * 4) + q * 4 + j];
            *(float4 *)(row + XCD_H1 + 4 * q) = make_float4(c[0], c[4], c[8], c[12]);
        } else {
            const int u4 = q - Q1;
            const float *c = cs2 + ((size_t)gg * XCD_H2 + 4 * u4) * 4 + j;
            *(float4 *)(row + 2 * XCD_H1 + 4 * u4) = h2h[(((size_t)k * a.RB + rb) * Q2 + u4) * 32 + clip];
            *(float4 *)(row + 2 * XCD_H1 + XCD_H2 + 4 * u4) = make_float4(c[0], c[4], c[8], c[12]);
        }
    }
    const long ny = (long)a.B * k;                   // float4 units
    const long nl = (long)a.B * OPNET_SLOTS_ * k;    // floats
    const float4 *ys = (const float4 *)(a.ws + a.ys_off);
    const float *ls = (const float *)(a.ws + a.lg_off);
    const float4 nan4 = make_float4(NAN, NAN, NAN, NAN);
    for (long i = i0; i < ny; i += stride) ((float4 *)s.y)[i] = ok ? ys[i] : nan4;
    for (long i = i0; i < nl; i += stride) s.logits[i] = ok ? ls[i] : NAN;
}
