// seq_stream_x_kernels.hip - gfx950 boundary kernels of a stacked-LSTM stream step that runs as ONE persistent launch of the
// 4-clip form (opseq_stream_step_x_f32): seqx_forward<.., false, true> between a prologue and a write-back, as
// seq_stream_kernels.hip puts the launch chain's step kernel between its two.
//
// Where a stream's state is around the persistent launch of T = k frames (seq_xcd_kernels.hip; stream b of the call is clip b:
// group G = b / 4, column j = b & 3):
//   in  : h_l of "step -1" = slot 0 of layer l's exchange / history buffer hl[l], [group][T + 1 slots][unit quad q][4 clips] float4
//         (float4 = units 4 q .. 4 q + 3 of clip j at [q][j]) - the slot step 0 gathers, where seqx_init puts zeros; c_l = the
//         staging buffer cs[l], [group][unit][4 clips] float, which the forward loads into LDS in place of its zero fill;
//   out : h_l of step T-1 = slot T of hl[l] (for the top layer: what seqx_out_head reads); c_l = cs[l] again, stored by the cell
//         wave behind the phase loop.
// The prologue's stores reach the persistent launch, and that launch's plain (XCD-local when the placement check passed) stores
// reach the write-back, across a kernel boundary each - the same hand-off seqx_init and seqx_out_head rely on.
// All of it is fp32 copies: a stream's frames see the arithmetic of the whole-clip 4-clip forward whatever the chunking.
#pragma once

struct SeqStreamXArgs {
    SeqXArgs a;              // the persistent launch's arguments for B = n clips, T = k frames
    const int32_t *slots;    // [n] pool rows, distinct, in [0, capacity)
    float *state;            // [capacity][2 * L * 512] = [h_0 | c_0 | h_1 | c_1]
    long capacity;
};

#define SSX_Q (SX_H / 4)       // unit quads of a layer

__device__ __forceinline__ float *seq_stream_x_row(const SeqStreamXArgs &s, int b)
{
    if (b >= s.a.B) return nullptr;
    const long slot = s.slots[b];
    // a slot outside the pool is a caller bug the host checks catch; here it must not turn into a wild access
    if (slot < 0 || slot >= s.capacity) return nullptr;
    return s.state + slot * (long)(2 * s.a.L * SX_H);
}

// An exchange word with the sentinel's bits would never count as published: every consumer would spin to the limit and the
// launch would give up.  It is a NaN either way, so a state word (h or c) with those bits enters the launch as the canonical one.
__device__ __forceinline__ unsigned seq_stream_x_word(float v)
{
    const unsigned u = __float_as_uint(v);
    return u == 0xffffffffu ? 0x7fc00000u : u;
}

// 1-D grid-stride.  What seqx_init does - status words, XCC sentinels, slots 1..T of every exchange buffer unpublished - except
// that slot 0 of hl[l] (and of its written-through copy hc[l], which nobody reads) holds each named stream's h_l and cs[l] its
// c_l (seq_stream_x_word); columns beyond n and ids outside the pool get zeros.
__global__ void __launch_bounds__(256) seq_stream_x_prologue(const SeqStreamXArgs s)
{
    const SeqXArgs &a = s.a;
    const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, n = (long)gridDim.x * blockDim.x;
    if (tid < 8) a.status[tid] = 0u;
    for (long i = tid; i < 256; i += n) a.status[8 + i] = 0xffffffffu;
    const xcd_u32x4 sent = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    const long per = (long)(a.T + 1) * (SSX_Q * 4), tot = (long)a.NGT * per;       // float4 per group, per buffer
    for (int l = 0; l < a.L; ++l) {
        xcd_u32x4 *hl = (xcd_u32x4 *)(a.ws + a.hl_off[l]);
        xcd_u32x4 *hc = l + 1 < a.L ? (xcd_u32x4 *)(a.ws + a.hc_off[l]) : nullptr;
        for (long i = tid; i < tot; i += n) {
            const long e = i % per;
            xcd_u32x4 v = sent;
            if (e < SSX_Q * 4) {              // slot 0: item (group, unit quad q, clip j)
                v = (xcd_u32x4){0u, 0u, 0u, 0u};
                const int j = e & 3, q = e >> 2;
                const float *row = seq_stream_x_row(s, (int)(i / per) * 4 + j);
                if (row) {
                    const float4 h = *(const float4 *)(row + l * 2 * SX_H + 4 * q);
                    v.x = seq_stream_x_word(h.x); v.y = seq_stream_x_word(h.y);
                    v.z = seq_stream_x_word(h.z); v.w = seq_stream_x_word(h.w);
                }
            }
            hl[i] = v;
            if (hc) hc[i] = v;
        }
        // cell states: item (group, unit quad q, clip j) -> four floats of [group][unit][4 clips]
        float *cs = (float *)(a.ws + a.cs_off[l]);
        for (long i = tid; i < (long)a.NGT * SSX_Q * 4; i += n) {
            const int j = i & 3, q = (i >> 2) % SSX_Q, g = (int)((i >> 2) / SSX_Q);
            float4 cv = make_float4(0.f, 0.f, 0.f, 0.f);
            const float *row = seq_stream_x_row(s, g * 4 + j);
            if (row) cv = *(const float4 *)(row + l * 2 * SX_H + SX_H + 4 * q);
            // c never enters an exchange buffer itself, but h = o * tanh(c') does, and a NaN operand hands its payload on: the
            // same canonical NaN
            float *dst = cs + ((size_t)g * SX_H + 4 * q) * 4 + j;
            dst[0] = __uint_as_float(seq_stream_x_word(cv.x));
            dst[4] = __uint_as_float(seq_stream_x_word(cv.y));
            dst[8] = __uint_as_float(seq_stream_x_word(cv.z));
            dst[12] = __uint_as_float(seq_stream_x_word(cv.w));
        }
    }
}

// 1-D grid-stride, behind seqx_out_head (which has written y, NaN if the launch gave up).  A launch that completed
// (status[0] == 0): every named stream's pool row gets its state after frame k-1.  A launch that gave up: the pool rows keep the
// state from before the call, so the caller can run the same call again.  Rows the call does not name are never touched.
__global__ void __launch_bounds__(256) seq_stream_x_writeback(const SeqStreamXArgs s)
{
    const SeqXArgs &a = s.a;
    if (a.status[0] != 0u) return;
    const long stride = (long)gridDim.x * blockDim.x;
    const long items = (long)a.NGT * a.L * SSX_Q * 4;        // (group, layer, unit quad, clip)
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < items; i += stride) {
        const int j = i & 3, q = (i >> 2) % SSX_Q;
        const int gl = (int)((i >> 2) / SSX_Q), l = gl % a.L, g = gl / a.L;
        float *row = seq_stream_x_row(s, g * 4 + j);
        if (!row) continue;
        const float4 *hl = (const float4 *)(a.ws + a.hl_off[l]);
        const float *c = (const float *)(a.ws + a.cs_off[l]) + ((size_t)g * SX_H + 4 * q) * 4 + j;
        *(float4 *)(row + l * 2 * SX_H + 4 * q) = hl[((size_t)g * (a.T + 1) + a.T) * (SSX_Q * 4) + q * 4 + j];
        *(float4 *)(row + l * 2 * SX_H + SX_H + 4 * q) = make_float4(c[0], c[4], c[8], c[12]);
    }
}
