// seq_stream_abi.hip - host side of the stateful stacked-LSTM streams (C ABI: opseq_stream_*; kernels in
// seq_stream_kernels.hip).  Included by opnet_abi.hip (one translation unit: it uses that file's fail / HIP_TRY / env_int /
// aligned16 / ew_blocks and the launch chain's check_stack / stack_args_inference / stack_hoisted_input_tiled /
// stack_step_form / stack_step_kernel).
#pragma once

// The skinny input product computes every 16-clip fragment of every frame that holds a live stream: k * ceil(n / 16) * 16
// rows, each fragment re-reading its 16 W_ih0 rows.  Calls of at most SEQ_STREAM_SKINNY_MAX_ROWS such rows take it; larger
// ones the tiled GEMM, which gives the same bits.  Measured on the MI355X (tools/stream_bench.py --model non_linear_lstm,
// DESIGN.md 12b): the product alone 223 against 289 us at 512 such rows, 443 against 293 us at 1 024.
// OPSEQ_STREAM_SKINNY_MAX_ROWS overrides it at call time; 0 = always the tiled GEMM.
#define SEQ_STREAM_SKINNY_MAX_ROWS 512
#define SEQ_STREAM_SKINNY_DEPTH 16       // K steps of 16 whose operands a wave keeps in flight

static long seq_stream_skinny_rows(int n, int k) { return (long)k * ((n + 15) / 16) * 16; }

// the hoisted layer-0 input product into xg [k][RB][H][32] float4: skinny (one wave per 16 x 16 fragment of xg, row fragments
// in its [t][rb][clip] order, the waves of a workgroup along rows over one column fragment) or the tiled GEMM + repack (its G
// in the workspace w)
static void seq_stream_input_product(const float *x, const float *packed, float4 *xg, char *w, int n, int k, int L, int KX,
                                     int H, bool skinny, hipStream_t st)
{
    if (skinny) {
        const StackPackedLayout P = stack_packed_layout(L, KX, H);
        const int RB = (n + 31) / 32;
        const long frags = (long)k * RB * 2;
        const int nw = frags < 4 ? (int)frags : 4;
        seq_stream_input_skinny<SEQ_STREAM_SKINNY_DEPTH><<<dim3((unsigned)((frags + nw - 1) / nw), H / 4), nw * 64, 0, st>>>(
            x, packed + P.wih0g, xg, n, k, RB, KX, H);
        return;
    }
    stack_hoisted_input_tiled(x, packed, w, xg, n, k, L, KX, H, st);
}

// the ragged form (lstm_stack_step_ragged) of the step kernel stack_step_kernel picks for this many row blocks
typedef void (*stack_step_ragged_fn)(const StackArgs, const int, const int32_t *);
static stack_step_ragged_fn stack_step_kernel_ragged(int RB)
{
    static const stack_step_ragged_fn k[] = {lstm_stack_step_ragged<8>, lstm_stack_step_ragged<4>, lstm_stack_step_ragged<4, 8>};
    return k[stack_step_form(RB)];
}

static bool seq_stream_takes_skinny(int n, int k)
{
    return seq_stream_skinny_rows(n, k) <= env_int("OPSEQ_STREAM_SKINNY_MAX_ROWS", SEQ_STREAM_SKINNY_MAX_ROWS);
}

static int check_seq_stream(int n, int k, int L, int KX, int H)
{
    if (int rc = check_stack(n, k, L, KX, H)) return rc;
    if ((n + 31) / 32 > 65535) return fail(OPNET_ESHAPE, "n=%d streams exceed one call's 65535 row blocks", n);
    return OPNET_OK;
}

extern "C" size_t opseq_stream_state_floats(int L, int H)
{
    if (check_stack(1, 1, L, 1, H)) return 0;
    return 2 * (size_t)L * H;
}

// the chain's inference workspace for n clips x k frames: the skinny product writes xg directly and leaves the chain's G
// buffer unused, but a call may still take the tiled GEMM (OPSEQ_STREAM_SKINNY_MAX_ROWS), so the size stays the chain's
extern "C" size_t opseq_stream_workspace_bytes(int n, int k, int L, int KX, int H)
{
    if (check_seq_stream(n, k, L, KX, H)) return 0;
    return stack_workspace_layout(n, k, L, KX, H).total;
}

// [hoisted input product] -> prologue -> k + 2L - 1 step launches -> write-back, dependent launches on `stream`, no host
// synchronisation.  lengths (device [n], or null for the uniform call) selects the ragged step kernel and is the
// write-back's len.
static int opseq_stream_step(const float *x, const int32_t *slots, const int32_t *lengths, float *state, const float *packed,
                             float *y, void *workspace, size_t workspace_bytes, int n, int k, int capacity, int L, int KX,
                             int H, void *stream)
{
    if (int rc = check_seq_stream(n, k, L, KX, H)) return rc;
    if (capacity <= 0) return fail(OPNET_ESHAPE, "capacity=%d must be positive", capacity);
    if (!x || !slots || !state || !packed || !y || !workspace) return fail(OPNET_EINVAL, "null pointer");
    const bool hoist = stack_hoists_input(KX, H);
    if (!aligned16(state) || !aligned16(packed) || !aligned16(y) || !aligned16(workspace) || (((uintptr_t)slots) & 3u) ||
        (((uintptr_t)lengths) & 3u) || (((uintptr_t)x) & (hoist ? 15u : 3u)))
        return fail(OPNET_EINVAL, "state/packed/y/workspace must be 16-byte aligned, slots/lengths 4-byte and x %d-byte",
                    hoist ? 16 : 4);
    const StackWorkspaceLayout W = stack_workspace_layout(n, k, L, KX, H);
    if (workspace_bytes < W.total) return fail(OPNET_EWORKSPACE, "workspace %zu B < %zu B", workspace_bytes, W.total);

    char *w = (char *)workspace;
    SeqStreamArgs s;
    memset(&s, 0, sizeof(s));
    const dim3 grid = stack_args_inference(&s.a, w, packed, n, k, L, KX, H);
    s.x = x;
    s.slots = slots;
    s.state = state;
    s.y = y;
    s.xp = (float4 *)(w + W.xp);
    s.KX = KX;
    s.KQ = hoist ? 0 : stack_packed_layout(L, KX, H).nhx[0] * 4;
    s.capacity = capacity;
    s.len = lengths;
    const StackArgs &a = s.a;
    hipStream_t st = (hipStream_t)stream;

    if (hoist)
        seq_stream_input_product(x, packed, (float4 *)(w + W.xg), w, n, k, L, KX, H, seq_stream_takes_skinny(n, k), st);
    // gather workgroups per row block: one work item per (layer, unit quad, clip), up to 256 a thread
    seq_stream_prologue<<<dim3((hoist ? 0 : k) + ew_blocks(L * (H / 4) * 32, 64), a.RB), 256, 0, st>>>(s);
    if (lengths) {
        const stack_step_ragged_fn stepk = stack_step_kernel_ragged(a.RB);
        for (int t = 0; t < k + 2 * L - 1; ++t) stepk<<<grid, stack_step_threads(a.RB), 0, st>>>(a, t, lengths);
    } else {
        const stack_step_fn stepk = stack_step_kernel(a.RB);
        for (int t = 0; t < k + 2 * L - 1; ++t) stepk<<<grid, stack_step_threads(a.RB), 0, st>>>(a, t);
    }
    const long outputs = (long)n * k, states = (long)a.RB * 32 * L * (H / 4);
    seq_stream_writeback<<<ew_blocks(outputs > states ? outputs : states, 1024), 256, 0, st>>>(s);
    HIP_TRY(hipGetLastError());
    return OPNET_OK;
}

extern "C" int opseq_stream_step_f32(const float *x, const int32_t *slots, float *state, const float *packed, float *y,
                                     void *workspace, size_t workspace_bytes, int n, int k, int capacity, int L, int KX,
                                     int H, void *stream)
{
    return opseq_stream_step(x, slots, nullptr, state, packed, y, workspace, workspace_bytes, n, k, capacity, L, KX, H,
                             stream);
}

// stream i advances by lengths[i] of the k frames (device int32 [n], clamped to [0, k] by the kernels)
extern "C" int opseq_stream_step_ragged_f32(const float *x, const int32_t *slots, const int32_t *lengths, float *state,
                                            const float *packed, float *y, void *workspace, size_t workspace_bytes, int n,
                                            int k, int capacity, int L, int KX, int H, void *stream)
{
    if (!lengths) return fail(OPNET_EINVAL, "null pointer: lengths");
    return opseq_stream_step(x, slots, lengths, state, packed, y, workspace, workspace_bytes, n, k, capacity, L, KX, H,
                             stream);
}

// the hoisted layer-0 input product of a stream call alone, into the caller's xg: route 0 = as opseq_stream_step_f32 routes
// it, 1 = the skinny kernel, 2 = the tiled GEMM + repack (workspace: opseq_stream_workspace_bytes)
extern "C" int opseq_stream_input_product_f32(const float *x, const float *packed, float *xg, void *workspace,
                                              size_t workspace_bytes, int n, int k, int L, int KX, int H, int route, void *stream)
{
    if (int rc = check_seq_stream(n, k, L, KX, H)) return rc;
    if (!stack_hoists_input(KX, H))
        return fail(OPNET_EINVAL, "layer 0's input is not hoisted (KX=%d H=%d: needs KX %% 16 == 0 and KX >= 2H)", KX, H);
    if (route < 0 || route > 2) return fail(OPNET_EINVAL, "route must be 0, 1 or 2 (got %d)", route);
    if (!x || !packed || !xg || !workspace) return fail(OPNET_EINVAL, "null pointer");
    if (!aligned16(x) || !aligned16(packed) || !aligned16(xg) || !aligned16(workspace))
        return fail(OPNET_EINVAL, "x/packed/xg/workspace must be 16-byte aligned");
    const size_t need = stack_workspace_layout(n, k, L, KX, H).total;
    if (workspace_bytes < need) return fail(OPNET_EWORKSPACE, "workspace %zu B < %zu B", workspace_bytes, need);
    const bool skinny = route == 0 ? seq_stream_takes_skinny(n, k) : route == 1;
    seq_stream_input_product(x, packed, (float4 *)xg, (char *)workspace, n, k, L, KX, H, skinny, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return OPNET_OK;
}

// ------------------------------------------------------------------------------------------------
// the same uniform step as ONE persistent launch of the 4-clip form (kernels: seq_stream_x_kernels.hip, seq_xcd_kernels.hip)
// ------------------------------------------------------------------------------------------------
// opseq_xcd_forward_f32's workspace (seqx_ws_layout, unchanged) with the cell-state staging buffers behind it
struct SeqXStreamLayout { SeqXWs W; size_t cs[2], total; };      // bytes
static SeqXStreamLayout seqx_stream_layout(int n, int k, int L, int KX, int H)
{
    SeqXStreamLayout S;
    S.W = seqx_ws_layout(n, k, L, KX, H);
    const size_t NGT = (n + 3) / 4;
    size_t o = S.W.total;
    for (int l = 0; l < 2; ++l) {
        S.cs[l] = o; if (l < L) o += NGT * SX_H * 4 * sizeof(float);
    }
    S.total = align_up(o, 4096);
    return S;
}
static int check_seqx_stream(int n, int k, int L, int KX, int H)
{
    if (int rc = check_seqx(n, k, L, KX, H)) return rc;
    if (L == 2 && seqx_nxq0(KX, H) != 0)
        return fail(OPNET_ESHAPE, "a persistent stream step is built for BaselineLstm (L=1, KX<=80) and NonLinearLstm (L=2, hoisted "
                                  "input); got L=%d KX=%d H=%d (transformer_lstm is not streamed)", L, KX, H);
    if (seqx_stream_layout(n, k, L, KX, H).total >= ((size_t)1 << 31))
        return fail(OPNET_ESHAPE, "n=%d x k=%d: the workspace exceeds the 2 GiB one buffer descriptor addresses", n, k);
    return OPNET_OK;
}

extern "C" int opseq_stream_x_max_streams(int L) { return opseq_xcd_max_batch(L); }

extern "C" size_t opseq_stream_x_workspace_bytes(int n, int k, int L, int KX, int H)
{
    if (check_seqx_stream(n, k, L, KX, H)) return 0;
    return seqx_stream_layout(n, k, L, KX, H).total;
}

extern "C" size_t opseq_stream_x_status_offset(int n, int k, int L, int KX, int H)
{
    if (check_seqx_stream(n, k, L, KX, H)) return (size_t)-1;
    return seqx_stream_layout(n, k, L, KX, H).W.status;
}

// [input pack | hoisted GEMM] -> prologue -> the persistent launch -> out_head -> write-back: five dependent launches on
// `stream` whatever k, no host synchronisation
extern "C" int opseq_stream_step_x_f32(const float *x, const int32_t *slots, float *state, const float *xpacked,
                                       const float *w_head, float *y, void *workspace, size_t workspace_bytes, int n, int k,
                                       int capacity, int L, int KX, int H, void *stream)
{
    if (int rc = check_seqx_stream(n, k, L, KX, H)) return rc;
    if (capacity <= 0) return fail(OPNET_ESHAPE, "capacity=%d must be positive", capacity);
    if (!x || !slots || !state || !xpacked || !w_head || !y || !workspace) return fail(OPNET_EINVAL, "null pointer");
    const int nxq0 = seqx_nxq0(KX, H);
    if (!aligned16(state) || !aligned16(xpacked) || !aligned16(w_head) || !aligned16(y) || !aligned16(workspace) ||
        (((uintptr_t)slots) & 3u) || (((uintptr_t)x) & (nxq0 == 0 ? 15u : 3u)))
        return fail(OPNET_EINVAL, "state/xpacked/w_head/y/workspace must be 16-byte aligned, slots 4-byte and x %d-byte",
                    nxq0 == 0 ? 16 : 4);
    const SeqXStreamLayout S = seqx_stream_layout(n, k, L, KX, H);
    if (workspace_bytes < S.total) return fail(OPNET_EWORKSPACE, "workspace %zu B < %zu B", workspace_bytes, S.total);
    int dev = 0;
    if (int rc = persistent_device(&dev)) return rc;
    const SeqXHostPacked PK = seqx_host_packed(L, KX, H);
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)workspace;
    const int RB = (n + 31) / 32;
    SeqStreamXArgs s;
    memset(&s, 0, sizeof(s));
    SeqXArgs &a = s.a;
    a.B = n; a.T = k; a.L = L; a.NGT = (n + 3) / 4; a.RB = RB; a.KXQ = nxq0;
    a.pk = xpacked + PK.regs;
    a.whead = w_head;
    a.ws = w;
    a.xp_off = (unsigned)S.W.xp; a.g_off = (unsigned)S.W.gemm;
    for (int l = 0; l < 2; ++l) {
        a.hl_off[l] = (unsigned)S.W.hl[l]; a.hc_off[l] = (unsigned)S.W.hc[l]; a.cs_off[l] = (unsigned)S.cs[l];
    }
    a.status = (unsigned *)(w + S.W.status);
    a.ystage = (float4 *)y;
    a.force_safe = env_int("OPNET_XCD_SAFE", 0);
    s.slots = slots;
    s.state = state;
    s.capacity = capacity;
    if (nxq0 == 0)      // G [n*k][4H] = x [n*k][KX] . W_ih0^T; the cell reads it where it lies
        launch_conv_tiled(row_gemm_args(x, xpacked + PK.wih0g, nullptr, nullptr, (float *)(w + S.W.gemm), (long)n * k, 4 * H, KX, 0),
                          (long)n * k, st);
    else
        rows_to_packed<<<1024, 256, 0, st>>>(x, (float4 *)(w + S.W.xp), n, k, RB, KX, 4 * nxq0, nullptr, 0);
    seq_stream_x_prologue<<<512, 256, 0, st>>>(s);
    if (int rc = persistent_launch(dev, st, PROF_SEQX, [&] {
            if (L == 1) seqx_forward<20, 1, false, true><<<XCD_COUNT * XCD_CUS, 256, 0, st>>>(a);
            else seqx_forward<0, 2, false, true><<<XCD_COUNT * XCD_CUS, 256, 0, st>>>(a);
        }))
        return rc;
    seqx_out_head<<<dim3(k, a.NGT), 64, 0, st>>>(a);
    seq_stream_x_writeback<<<ew_blocks((long)a.NGT * L * SSX_Q * 4, 1024), 256, 0, st>>>(s);
    HIP_TRY(hipGetLastError());
    return OPNET_OK;
}
