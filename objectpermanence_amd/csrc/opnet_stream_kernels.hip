// opnet_stream_kernels.hip - gfx950 boundary kernels of the stateful OPNet streams (opnet_stream_step_f32).
//
// A call advances n streams by k frames each.  Between calls a stream's recurrent state lives in a row of a
// caller-owned pool, float state[capacity][2*H1 + 2*H2] = [h1 | c1 | h2 | c2] in torch's unit order (what nn.LSTM
// returns as h_n / c_n).  The frames themselves run through the launch chain's own step kernel (opnet_kernels.hip,
// k + 3 launches of opnet_step / opnet_step_wide over an inference workspace of n clips x k frames); the two kernels
// here replace its boundary kernels:
//   prologue   : boxes -> xp (pack_input_body), and each named pool row -> the rings where step t = 0 reads its
//                previous state (h: slot_prev(a, 0), c: cslot_prev(a, 0)) - in place of the chain's zeroing;
//   write-back : the rings after step k-1 (slot_out / cslot_out) -> the pool rows, and the staging buffers -> the
//                caller's y / logits, as opnet_copy_out.
// Ragged calls (opnet_stream_step_ragged_f32) run the step kernel's ragged form, where stream b's column freezes from frame
// len[b] on, so the state copy is the same; the write-back then writes +0.0 to y / logits at frames t >= len[b] (StreamArgs
// len; null for uniform calls).
// Gather and write-back are plain fp32 copies, so a clip's frames see exactly the arithmetic of the whole-clip chain
// whatever the chunking.  OPNetLstmMlp (a.mlp) has no LSTM2 state: its h2 / c2 columns are neither read nor written.
#pragma once

struct StreamArgs {
    StepArgs a;              // the step kernel's arguments for B = n clips, T = k frames (inference layout)
    const float *boxes;      // [n][k][90]
    const int32_t *slots;    // [n] pool rows, distinct, in [0, capacity)
    float *state;            // [capacity][2*H1 + 2*H2]
    float *y;                // [n][k][4]
    float *logits;           // [n][15][k]
    float4 *xp;              // the packed LSTM1 input of the workspace (a.xp, writable)
    long capacity;
    const int32_t *len;      // [n] frames per stream (ragged calls), or null: k each
};

__device__ __forceinline__ const float *stream_row(const StreamArgs &s, int b)
{
    const long slot = s.slots[b];
    // a slot outside the pool is a caller bug the host checks catch; here it must not turn into a wild access
    if (slot < 0 || slot >= s.capacity) return nullptr;
    return s.state + slot * (2L * (s.a.H1 + s.a.H2));
}

// grid (k + G, RB) x 256: workgroups x < k pack frame x of row block y; the G beyond gather that row block's state.
// Work item j of the gather = (unit quad q, clip j & 31); q < H1/4 is LSTM1, the rest LSTM2.
__global__ void __launch_bounds__(256) opnet_stream_prologue(const StreamArgs s)
{
    const StepArgs &a = s.a;
    const int rb = blockIdx.y;
    if ((int)blockIdx.x < a.T) {
        OpnetIO io = {};
        io.B = a.B; io.T = a.T; io.RB = a.RB;
        io.boxes = s.boxes;
        io.xp = s.xp;           // io.state_f4 = 0: nothing to zero, the gather below sets the state
        pack_input_body(&io, blockIdx.x, rb, gridDim.y);
        return;
    }
    const int Q1 = a.H1 >> 2, Q = Q1 + (a.H2 >> 2);
    const int G = gridDim.x - a.T;
    for (int j = (blockIdx.x - a.T) * 256 + threadIdx.x; j < Q * 32; j += G * 256) {
        const int clip = j & 31, q = j >> 5;
        const int b = rb * 32 + clip;
        const bool l1 = q < Q1;
        const int H = l1 ? a.H1 : a.H2;
        const int u4 = l1 ? q : q - Q1;
        float4 h = make_float4(0.f, 0.f, 0.f, 0.f), c = h;
        if (b < a.B && (l1 || !a.mlp)) {
            const float *row = stream_row(s, b);
            if (row) {
                row += l1 ? 0 : 2 * a.H1;
                h = *(const float4 *)(row + 4 * u4);
                c = *(const float4 *)(row + H + 4 * u4);
            }
        }
        float4 *hb = l1 ? a.h1buf : a.h2buf;
        float *cb = l1 ? a.c1 : a.c2;
        hb[((slot_prev(a, 0) * a.RB + rb) * (H >> 2) + u4) * 32 + clip] = h;
        float *cc = cb + ((cslot_prev(a, 0) * a.RB + rb) * H + 4 * u4) * 32 + clip;
        cc[0] = c.x;
        cc[32] = c.y;
        cc[64] = c.z;
        cc[96] = c.w;
    }
}

// element i of a [n][.. per ..] output, at frame i % k of stream i / per, keeps its value: always in a uniform call (len
// null), for the first len[b] frames of a ragged one (clamped to [0, k]: the kernels cannot trust a device array the host
// never saw); otherwise it is written as +0.0
__device__ __forceinline__ bool frame_kept(const int32_t *len, long i, long per, int k)
{
    return !len || (int)(i % k) < min(max(len[i / per], 0), k);
}

// 1-D grid-stride: the final state of every stream (after LSTM1 / LSTM2 step k-1) -> its pool row, then y and logits
// (+0.0 at the frames frame_kept drops)
__global__ void __launch_bounds__(256) opnet_stream_writeback(const StreamArgs s)
{
    const StepArgs &a = s.a;
    const int k = a.T;
    const int Q1 = a.H1 >> 2, Q = a.mlp ? Q1 : Q1 + (a.H2 >> 2);
    const long stride = (long)gridDim.x * blockDim.x;
    const long i0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long nst = (long)a.RB * Q * 32;
    for (long j = i0; j < nst; j += stride) {
        const int clip = j & 31;
        const long rq = j >> 5;
        const int q = rq % Q;
        const int rb = rq / Q;
        const int b = rb * 32 + clip;
        if (b >= a.B) continue;
        float *row = (float *)stream_row(s, b);
        if (!row) continue;
        const bool l1 = q < Q1;
        const int H = l1 ? a.H1 : a.H2;
        const int u4 = l1 ? q : q - Q1;
        const float4 *hb = l1 ? a.h1buf : a.h2buf;
        const float *cb = l1 ? a.c1 : a.c2;
        const float4 h = hb[((slot_out(a, k - 1) * a.RB + rb) * (H >> 2) + u4) * 32 + clip];
        const float *cc = cb + ((cslot_out(a, k - 1) * a.RB + rb) * H + 4 * u4) * 32 + clip;
        row += l1 ? 0 : 2 * a.H1;
        *(float4 *)(row + 4 * u4) = h;
        *(float4 *)(row + H + 4 * u4) = make_float4(cc[0], cc[32], cc[64], cc[96]);
    }
    const long ny = (long)a.B * k;                   // float4 units
    const long nl = (long)a.B * OPNET_SLOTS_ * k;    // floats
    for (long i = i0; i < ny; i += stride) {
        const float4 v = a.ystage[i];
        ((float4 *)s.y)[i] = frame_kept(s.len, i, k, k) ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (long i = i0; i < nl; i += stride) s.logits[i] = frame_kept(s.len, i, (long)OPNET_SLOTS_ * k, k) ? a.lgstage[i] : 0.f;
}
