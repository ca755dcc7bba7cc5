// opnet_state_train_kernels.hip - gfx950 boundary kernels of a training step that starts from a carried LSTM state
// (opnet_train_forward_state_f32 / opnet_train_backward_state_f32).
//
// State and state gradients cross the ABI as rows [B][2*H1 + 2*H2] = [h1 | c1 | h2 | c2] in torch's unit order - the row
// layout of the stream pool (opnet_stream_kernels.hip), so a pool slice is passed as it lies.  Inside, the state of a training
// step lives in the histories of the launch chain: slot 0 of h1all / c1all / h2all / c2all is what step 0 reads
// (slot_prev(a, 0) / cslot_prev(a, 0) with a.train set), slot T what step T-1 wrote.
//   forward : rows -> slot 0 behind opnet_pack_input's zeroing, slot T -> rows behind the chain (opnet_train_state_copy);
//             plain fp32 copies, so the frames see the arithmetic of the whole-clip chain;
//   backward: the gradient arriving on the final state -> where the reverse recurrence's first step looks for what comes
//             from t + 1 (opnet_pack_dstate_seed; BwdArgs::seeded widens the `t < T - 1` tests of the cell backwards), and
//             the gradient of the initial state out of what the recurrence left behind (opnet_bwd_dstate).
// OPNetLstmMlp (a.mlp) has no LSTM2 state: the h2 / c2 columns of the rows are neither read nor written.
#pragma once

// Work item = (row block, unit quad q, clip): q < H1/4 is LSTM1, the rest LSTM2.  OUT = false: rows -> slot (clips beyond
// B keep the zero they hold); OUT = true: slot -> rows.
template <bool OUT>
__global__ void __launch_bounds__(256) opnet_train_state_copy(const StepArgs a, float *__restrict__ rows, const long slot)
{
    const int Q1 = a.H1 >> 2, Q = a.mlp ? Q1 : Q1 + (a.H2 >> 2);
    const long rowlen = 2L * (a.H1 + a.H2);
    const long n = (long)a.RB * Q * 32;
    for (long j = blockIdx.x * 256L + threadIdx.x; j < n; j += gridDim.x * 256L) {
        const int clip = j & 31;
        const long rq = j >> 5;
        const int q = rq % Q;
        const int rb = rq / Q;
        const long b = (long)rb * 32 + clip;
        if (b >= a.B) continue;
        const bool l1 = q < Q1;
        const int H = l1 ? a.H1 : a.H2;
        const int u4 = l1 ? q : q - Q1;
        float4 *hb = (l1 ? a.h1buf : a.h2buf) + ((slot * a.RB + rb) * (H >> 2) + u4) * 32 + clip;
        float *cc = (l1 ? a.c1 : a.c2) + ((slot * a.RB + rb) * H + 4 * u4) * 32 + clip;
        float *row = rows + b * rowlen + (l1 ? 0 : 2 * a.H1);
        if (OUT) {
            *(float4 *)(row + 4 * u4) = *hb;
            *(float4 *)(row + H + 4 * u4) = make_float4(cc[0], cc[32], cc[64], cc[96]);
        } else {
            *hb = *(const float4 *)(row + 4 * u4);
            const float4 c = *(const float4 *)(row + H + 4 * u4);
            cc[0] = c.x;
            cc[32] = c.y;
            cc[64] = c.z;
            cc[96] = c.w;
        }
    }
}

// d new_state rows -> the reverse recurrence's entry at t = T-1: dh as split-K partial 0 of dhpart (partials 1..3 zero, so
// the split pair's ((p0 + p1) + p2) + p3 is the seed itself; the fused form reads partial 0 alone), dc in the cell-gradient
// carry.  Runs behind opnet_pack_dy, which zeroed the carries.  Clips beyond B get zeros.
__global__ void __launch_bounds__(256) opnet_pack_dstate_seed(const BwdArgs a, const float *__restrict__ seed)
{
    const int HH = a.mlp ? a.H1 : a.H1 + a.H2;
    const long rowlen = 2L * (a.H1 + a.H2);
    const long n = (long)a.RB * HH * 32;
    for (long j = blockIdx.x * 256L + threadIdx.x; j < n; j += gridDim.x * 256L) {
        const int clip = j & 31;
        const long ru = j >> 5;
        const int uu = ru % HH;
        const int rb = ru / HH;
        const long b = (long)rb * 32 + clip;
        const bool l1 = uu < a.H1;
        const int H = l1 ? a.H1 : a.H2;
        const int u = l1 ? uu : uu - a.H1;
        float dh = 0.f, dc = 0.f;
        if (b < a.B) {
            const float *row = seed + b * rowlen + (l1 ? 0 : 2 * a.H1);
            dh = row[u];
            dc = row[H + u];
        }
        const long e = ((long)rb * H + u) * 32 + clip;
        const long ps = (long)a.RB * H * 32;
        float *part = l1 ? a.dhpart1 : a.dhpart2;
        part[e] = dh;
        part[ps + e] = 0.f;
        part[2 * ps + e] = 0.f;
        part[3 * ps + e] = 0.f;
        (l1 ? a.dc1 : a.dc2)[e] = dc;
    }
}

// d state_in rows, behind the reverse recurrence of any form:
//     dh_init = W_hh^T da_0   - the product pass "t = -1" that no cell follows: fused_product over the gate gradients of t = 0;
//     dc_init = dc_0 * f_0    - what the cell backward of t = 0 left in the carry.
// grid.x = 2 * (H2/16 + H1/16) workgroups (LSTM2 tiles first; tile x clip half as opnet_bwd_fused), grid.y <= RB.
__global__ void __launch_bounds__(FUSED_THREADS) opnet_bwd_dstate(const BwdArgs a, float *__restrict__ dstate)
{
    __shared__ __attribute__((aligned(16))) float part[FUSED_NW * 4 * 64];
    const int n2 = 2 * (a.H2 >> 4);
    const int bx = blockIdx.x, tid = threadIdx.x;
    const bool l1 = bx >= n2;
    if (!l1 && a.mlp) return;
    const int H = l1 ? a.H1 : a.H2;
    const int b1 = l1 ? bx - n2 : bx;
    const int tile = b1 >> 1, hf = b1 & 1;
    const float4 *A = (l1 ? a.w1bt : a.w2bt) + (long)tile * (H >> 2) * 64;
    const float4 *da = l1 ? a.g1 : a.g2;
    const float *dc = l1 ? a.dc1 : a.dc2;
    const long rowlen = 2L * (a.H1 + a.H2);
    const int u = tile * 16 + ((tid & 255) >> 4), clip = hf * 16 + (tid & 15);
    for (int rb = blockIdx.y; rb < a.RB; rb += gridDim.y) {
        const float rec = fused_product(A, da + (long)rb * H * 32, H >> 2, hf, part);
        const long b = (long)rb * 32 + clip;
        if (tid < 256 && b < a.B) {
            float *row = dstate + b * rowlen + (l1 ? 0 : 2 * a.H1);
            row[u] = rec;
            row[H + u] = dc[((long)rb * H + u) * 32 + clip];
        }
        if (rb + (int)gridDim.y < a.RB) __syncthreads();
    }
}
