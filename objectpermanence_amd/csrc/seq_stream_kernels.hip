// seq_stream_kernels.hip - gfx950 kernels of the stateful stacked-LSTM streams (opseq_stream_step_f32: BaselineLstm,
// NonLinearLstm).
//
// A call advances n streams by k frames each.  Between calls a stream's recurrent state lives in a row of a caller-owned
// pool, float state[capacity][2*L*H] = [h_0 | c_0 | h_1 | c_1 ...] in torch's unit order (nn.LSTM's h_n / c_n, layer by
// layer).  The frames run through the launch chain's own step kernel (seq_kernels.hip lstm_stack_step, k + 2L - 1 launches
// over an inference workspace of n clips x k frames); the kernels here replace its boundary kernels:
//   prologue     : x -> xp (as rows_to_packed; only when layer 0 reads its input directly), and each named pool row -> the
//                  buffers where step t = 0 reads its previous state (h: hbuf parity slot 1, c: slot 0) - in place of the
//                  chain's zeroing;
//   write-back   : hbuf slot (k-1)&1 and c of every layer -> the pool rows, and ystage -> y (as copy_y_out);
//   skinny input : NonLinearLstm's hoisted layer-0 input product xg = x . W_ih0^T for calls with few rows, straight into
//                  the step kernel's xg layout (see seq_stream_input_skinny).
// Ragged calls (opseq_stream_step_ragged_f32) run lstm_stack_step_ragged, where stream b's column freezes from frame len[b]
// on, so the state copy is the same; the write-back then writes +0.0 to y at frames t >= len[b] (SeqStreamArgs len; null
// for uniform calls).
// Gather and write-back are plain fp32 copies and the skinny product does the tiled GEMM's arithmetic per element, so a
// clip's frames see exactly the arithmetic of the whole-clip chain whatever the chunking.
#pragma once

struct SeqStreamArgs {
    StackArgs a;             // the step kernel's arguments for B = n clips, T = k frames (inference layout)
    const float *x;          // [n][k][KX] layer 0's input
    const int32_t *slots;    // [n] pool rows, distinct, in [0, capacity)
    float *state;            // [capacity][2*L*H]
    float *y;                // [n][k][4]
    float4 *xp;              // the packed layer-0 input of the workspace (a.xp, writable); unused when hoisted
    int KX, KQ;              // layer 0's input width, and its k-quads in xp (0: hoisted, nothing to pack)
    long capacity;
    const int32_t *len;      // [n] frames per stream (ragged calls), or null: k each
};

__device__ __forceinline__ float *seq_stream_row(const SeqStreamArgs &s, int b)
{
    const long slot = s.slots[b];
    // a slot outside the pool is a caller bug the host checks catch; here it must not turn into a wild access
    if (slot < 0 || slot >= s.capacity) return nullptr;
    return s.state + slot * (2L * s.a.L * s.a.layer[0].H);
}

// grid (P + G, RB) x 256, P = k when layer 0's input is packed (KQ > 0), else 0: workgroups x < P pack frame x of row
// block y (the rows_to_packed layout [t][rb][KQ][32] float4, K zero-padded); the G beyond gather that row block's state.
// Work item j of the gather = (layer l, unit quad u4, clip j & 31).
__global__ void __launch_bounds__(256) seq_stream_prologue(const SeqStreamArgs s)
{
    const StackArgs &a = s.a;
    const int rb = blockIdx.y;
    const int P = s.KQ > 0 ? a.T : 0;
    if ((int)blockIdx.x < P) {
        const int t = blockIdx.x;
        for (int j = threadIdx.x; j < s.KQ * 32; j += 256) {
            const int kq = j % s.KQ, clip = j / s.KQ;       // consecutive threads walk k within one row: coalesced reads
            const int b = rb * 32 + clip;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (b < a.B) {
                const float *src = s.x + ((long)b * a.T + t) * s.KX + kq * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (kq * 4 + e < s.KX) v[e] = src[e];
            }
            s.xp[(((long)t * a.RB + rb) * s.KQ + kq) * 32 + clip] = make_float4(v[0], v[1], v[2], v[3]);
        }
        return;
    }
    const int H = a.layer[0].H, Q = H >> 2;
    const int G = gridDim.x - P;
    for (int j = (blockIdx.x - P) * 256 + threadIdx.x; j < a.L * Q * 32; j += G * 256) {
        const int clip = j & 31, q = j >> 5;
        const int l = q / Q, u4 = q - l * Q;
        const int b = rb * 32 + clip;
        float4 h = make_float4(0.f, 0.f, 0.f, 0.f), c = h;
        if (b < a.B) {
            const float *row = seq_stream_row(s, b);
            if (row) {
                row += 2L * l * H;
                h = *(const float4 *)(row + 4 * u4);
                c = *(const float4 *)(row + H + 4 * u4);
            }
        }
        const StackLayer &ly = a.layer[l];
        ly.hbuf[((1L * a.RB + rb) * Q + u4) * 32 + clip] = h;         // parity slot (t + 1) & 1 of step t = 0
        float *cc = ly.c + (((long)rb * H + 4 * u4) * 32) + clip;      // slot 0: read and written in place
        cc[0] = c.x;
        cc[32] = c.y;
        cc[64] = c.z;
        cc[96] = c.w;
    }
}

// 1-D grid-stride: the final state of every stream (every layer after step k-1) -> its pool row, then ystage -> y (+0.0 at
// the frames frame_kept drops, opnet_stream_kernels.hip)
__global__ void __launch_bounds__(256) seq_stream_writeback(const SeqStreamArgs s)
{
    const StackArgs &a = s.a;
    const int k = a.T;
    const int H = a.layer[0].H, Q = H >> 2;
    const long so = (k - 1) & 1;
    const long stride = (long)gridDim.x * blockDim.x;
    const long i0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long nst = (long)a.RB * a.L * Q * 32;
    for (long j = i0; j < nst; j += stride) {
        const int clip = j & 31;
        const long rq = j >> 5;
        const int q = rq % (a.L * Q);
        const int rb = rq / (a.L * Q);
        const int b = rb * 32 + clip;
        if (b >= a.B) continue;
        float *row = seq_stream_row(s, b);
        if (!row) continue;
        const int l = q / Q, u4 = q - l * Q;
        const StackLayer &ly = a.layer[l];
        const float4 h = ly.hbuf[((so * a.RB + rb) * Q + u4) * 32 + clip];
        const float *cc = ly.c + (((long)rb * H + 4 * u4) * 32) + clip;
        row += 2L * l * H;
        *(float4 *)(row + 4 * u4) = h;
        *(float4 *)(row + H + 4 * u4) = make_float4(cc[0], cc[32], cc[64], cc[96]);
    }
    const long ny = (long)a.B * k;                   // float4 units: ystage rows b < B are y's [B][k] prefix
    for (long i = i0; i < ny; i += stride) {
        const float4 v = a.ystage[i];
        ((float4 *)s.y)[i] = frame_kept(s.len, i, k, k) ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// The hoisted layer-0 input product of a call with few rows: xg [k][RB][H][32] float4 = x . W_ih0^T, for NonLinearLstm's
// one-frame calls (M = n*k rows of K = KX, N = 4H columns).  The tiled GEMM (conv2d_nhwc_glds) fills 128-row tiles and runs
// 16 chains a wave; with M = 32 that is mostly padding on 16 workgroups.  Here one wave owns ONE 16 x 16 output fragment:
//   rows    = 16 clips of one (frame t, row block rb, half) in the xg order [t][rb][clip] - clips past n are written as
//             zeros (what stack_xg_repack writes there), a fragment of such clips only without computing it;
//   columns = 16 rows of the packed W_ih0 (wih0g: row 4 unit + gate) = units 4j .. 4j+3, so a lane's 4 results are one
//             unit's gate float4 of xg.
// Per element this is conv2d_nhwc_glds's arithmetic: ONE accumulator, K walked in order 16 at a time as four
// v_mfma_f32_16x16x4_f32 (component c of the lane's k-quad, weights as the first operand, pixels as the second), no K
// split - the f32 MFMA is bitwise an fmaf chain, so the bits are the tiled kernel's whatever the fragment's neighbours.
// Parallelism is M x N only: (M/16) x (4H/16) chains of KX/4 dependent MFMAs.  At 32 cycles issue and 40 dependent
// latency per SIMD a second accumulator in the same wave would lengthen every chain (2 x 32 > 40), so a wave keeps one;
// the waves of a workgroup share a column fragment (its W rows through one L1), and the loads run D steps ahead.
template <int D>
__global__ void __launch_bounds__(256) seq_stream_input_skinny(const float *__restrict__ x, const float *__restrict__ wih,
                                                               float4 *__restrict__ xg, int n, int k, int RB, int KX, int H)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int i = lane & 15, kk = lane >> 4;
    const long frag = (long)blockIdx.x * (blockDim.x >> 6) + wave;     // row fragment: (t, rb, half)
    if (frag >= (long)k * RB * 2) return;
    const int half = frag & 1;
    const int rb = (frag >> 1) % RB;
    const int t = (frag >> 1) / RB;
    const int j = blockIdx.y;                                           // column fragment: units 4j .. 4j + 3
    const int clip = half * 16 + i;
    const int b = rb * 32 + clip;
    float4 *dst = xg + (((long)t * RB + rb) * H + 4 * j + kk) * 32 + clip;
    if (rb * 32 + half * 16 >= n) {                                     // (wave-uniform) padding clips only
        *dst = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    // clips past n read the last stream's row (their results are replaced by zeros below; a D column is its own chain): no
    // predicated loads, so every load of the ring stays in flight
    const float *xrow = x + ((long)(b < n ? b : n - 1) * k + t) * KX + 4 * kk;
    const float *wrow = wih + (long)(16 * j + i) * KX + 4 * kk;
    const int nhex = KX >> 4;
    float4 xr[D], wr[D];
#pragma unroll
    for (int u = 0; u < D; ++u) {
        const int q = u < nhex ? u : nhex - 1;
        xr[u] = *(const float4 *)(xrow + 16 * q);
        wr[u] = *(const float4 *)(wrow + 16 * q);
    }
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    // whole rounds of D steps without a branch (a branch per step makes the compiler drain every load of the ring at it);
    // ring slot u holds step q0 + u
    int q0 = 0;
    for (; q0 + D <= nhex; q0 += D) {
#pragma unroll
        for (int u = 0; u < D; ++u) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[u].x, xr[u].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[u].y, xr[u].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[u].z, xr[u].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[u].w, xr[u].w, acc, 0, 0, 0);
            // refill the slot it just consumed (into the same registers: no copy that would wait for the load)
            const int qn = q0 + u + D < nhex ? q0 + u + D : nhex - 1;   // (past the end: a redundant in-bounds load)
            xr[u] = *(const float4 *)(xrow + 16 * qn);
            wr[u] = *(const float4 *)(wrow + 16 * qn);
            __builtin_amdgcn_sched_barrier(0);      // keep the refill here: clustered at the round's end, each round would
        }                                           // wait for a whole memory latency
    }
#pragma unroll
    for (int u = 0; u < D; ++u) {                                       // the last nhex % D steps
        if (q0 + u < nhex) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[u].x, xr[u].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[u].y, xr[u].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[u].z, xr[u].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[u].w, xr[u].w, acc, 0, 0, 0);
        }
    }
    // D fragment lane = (pixel column i, rows 4 kk + r = gate r of unit 4j + kk); clips past n get zeros
    *dst = b < n ? make_float4(acc[0], acc[1], acc[2], acc[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
}
