// opnet_stream_abi.hip - host side of the stateful OPNet streams (C ABI: opnet_stream_*; kernels in opnet_stream_kernels.hip).
// Included by opnet_abi.hip (one translation unit: it uses that file's fail / HIP_TRY / check_dims / aligned16 / ew_blocks and
// the launch chain's step_form / step_kernel / step_grid / step_threads).
#pragma once

extern "C" size_t opnet_stream_state_floats(int H1, int H2)
{
    if (check_dims(1, 1, H1, H2)) return 0;
    return 2 * (size_t)H1 + 2 * (size_t)H2;
}

// the chain's inference workspace for n clips x k frames (its OpnetIO head stays unused: the boundary kernels take their
// arguments by value)
extern "C" size_t opnet_stream_workspace_bytes(int n, int k, int H1, int H2)
{
    if (check_dims(n, k, H1, H2)) return 0;
    if ((n + 31) / 32 > 65535) { fail(OPNET_ESHAPE, "n=%d streams exceed one call's 65535 row blocks", n); return 0; }
    return workspace_layout(n, k, H1, H2).total;
}

// the ragged form (opnet_step_ragged / opnet_step_wide_ragged) of the step kernel step_kernel picks for this shape
typedef void (*opnet_step_ragged_fn)(const StepArgs, const int, const int32_t *);
static opnet_step_ragged_fn step_kernel_ragged(const StepArgs &a)
{
    static const opnet_step_ragged_fn k[] = {opnet_step_ragged<8>, opnet_step_ragged<4>, opnet_step_ragged<4, 8>,
                                             opnet_step_wide_ragged<8>, opnet_step_wide_ragged<4>};
    return k[step_form(a)];
}

// prologue -> k + 3 step launches -> write-back: k + 5 dependent launches on `stream`, no host synchronisation.  lengths
// (device [n], or null for the uniform call) selects the ragged step kernel and is the write-back's len.
static int opnet_stream_step(const float *boxes, const int32_t *slots, const int32_t *lengths, float *state,
                             const float *packed, float *y, float *logits, void *workspace, size_t workspace_bytes, int n,
                             int k, int capacity, int H1, int H2, int mlp, void *stream)
{
    if (int rc = check_dims(n, k, H1, H2)) return rc;
    if (capacity <= 0) return fail(OPNET_ESHAPE, "capacity=%d must be positive", capacity);
    if ((n + 31) / 32 > 65535) return fail(OPNET_ESHAPE, "n=%d streams exceed one call's 65535 row blocks", n);
    if (mlp != 0 && mlp != 1) return fail(OPNET_EINVAL, "mlp must be 0 or 1 (got %d)", mlp);
    if (!boxes || !slots || !state || !packed || !y || !logits || !workspace) return fail(OPNET_EINVAL, "null pointer");
    if (!aligned16(state) || !aligned16(packed) || !aligned16(y) || !aligned16(workspace) || (((uintptr_t)boxes) & 7u) ||
        (((uintptr_t)slots) & 3u) || (((uintptr_t)logits) & 3u) || (((uintptr_t)lengths) & 3u))
        return fail(OPNET_EINVAL, "state/packed/y/workspace must be 16-byte, boxes 8-byte and slots/lengths/logits 4-byte "
                                  "aligned");
    const WorkspaceLayout W = workspace_layout(n, k, H1, H2);
    if (workspace_bytes < W.total) return fail(OPNET_EWORKSPACE, "workspace %zu B < %zu B", workspace_bytes, W.total);

    StreamArgs s;
    memset(&s, 0, sizeof(s));
    step_args_inference(&s.a, (char *)workspace, packed, n, k, H1, H2);
    s.a.mlp = mlp;
    s.boxes = boxes;
    s.slots = slots;
    s.state = state;
    s.y = y;
    s.logits = logits;
    s.xp = (float4 *)((char *)workspace + W.xp);
    s.capacity = capacity;
    s.len = lengths;
    const StepArgs &a = s.a;
    hipStream_t st = (hipStream_t)stream;

    // gather workgroups per row block: one work item per (unit quad, clip), up to 256 a thread
    opnet_stream_prologue<<<dim3(k + ew_blocks((H1 + H2) / 4 * 32, 64), a.RB), 256, 0, st>>>(s);
    // the chain's step kernel for this shape; the kernarg-preload form (opnet_step_pl) is left out: it carves its buffers
    // from the chain's own workspace, and computes the same body as opnet_step<4, 8>
    const dim3 grid = step_grid(a);
    if (lengths) {
        const opnet_step_ragged_fn stepk = step_kernel_ragged(a);
        for (int t = 0; t < k + 3; ++t) stepk<<<grid, step_threads(a), 0, st>>>(a, t, lengths);
    } else {
        const opnet_step_fn stepk = step_kernel(a);
        for (int t = 0; t < k + 3; ++t) stepk<<<grid, step_threads(a), 0, st>>>(a, t);
    }
    const long outputs = (long)a.B * OPNET_SLOTS * k, states = (long)a.RB * 32 * (H1 + H2) / 4;
    opnet_stream_writeback<<<ew_blocks(outputs > states ? outputs : states, 1024), 256, 0, st>>>(s);
    HIP_TRY(hipGetLastError());
    return OPNET_OK;
}

extern "C" int opnet_stream_step_f32(const float *boxes, const int32_t *slots, float *state, const float *packed, float *y,
                                     float *logits, void *workspace, size_t workspace_bytes, int n, int k, int capacity, int H1,
                                     int H2, int mlp, void *stream)
{
    return opnet_stream_step(boxes, slots, nullptr, state, packed, y, logits, workspace, workspace_bytes, n, k, capacity, H1,
                             H2, mlp, stream);
}

// stream i advances by lengths[i] of the k frames (device int32 [n], clamped to [0, k] by the kernels)
extern "C" int opnet_stream_step_ragged_f32(const float *boxes, const int32_t *slots, const int32_t *lengths, float *state,
                                            const float *packed, float *y, float *logits, void *workspace,
                                            size_t workspace_bytes, int n, int k, int capacity, int H1, int H2, int mlp,
                                            void *stream)
{
    if (!lengths) return fail(OPNET_EINVAL, "null pointer: lengths");
    return opnet_stream_step(boxes, slots, lengths, state, packed, y, logits, workspace, workspace_bytes, n, k, capacity, H1,
                             H2, mlp, stream);
}

// ------------------------------------------------------------------------------------------------
// the same step as ONE persistent launch of the 4-clip form (kernels: opnet_stream_x4_kernels.hip, opnet_xcd4_kernels.hip)
// ------------------------------------------------------------------------------------------------
// opnet_xcd4_forward_f32's workspace (x4_infer_layout, unchanged) with the cell-state staging buffers behind it
struct X4StreamLayout { X4InferLayout L; size_t cs1, cs2, total; };      // bytes
static X4StreamLayout x4_stream_layout(int n, int k)
{
    X4StreamLayout S;
    S.L = x4_infer_layout(n, k);
    const size_t NG = (size_t)((n + 31) / 32) * 8;
    size_t o = S.L.total;
    S.cs1 = o; o += NG * XCD_H1 * 4 * sizeof(float);
    S.cs2 = o; o += NG * XCD_H2 * 4 * sizeof(float);
    S.total = align_up(o, 256);
    return S;
}
static int check_x4_stream(int n, int k, int H1, int H2)
{
    if (int rc = check_x4_infer(n, k, H1, H2)) return rc;
    if (x4_stream_layout(n, k).total >= ((size_t)1 << 31))
        return fail(OPNET_ESHAPE, "n=%d x k=%d: the workspace exceeds the 2 GiB one buffer descriptor addresses", n, k);
    return OPNET_OK;
}

extern "C" int opnet_stream_x4_max_streams(void) { return opnet_xcd4_max_batch(); }

extern "C" size_t opnet_stream_x4_workspace_bytes(int n, int k, int H1, int H2)
{
    if (check_x4_stream(n, k, H1, H2)) return 0;
    return x4_stream_layout(n, k).total;
}

extern "C" size_t opnet_stream_x4_status_offset(int n, int k, int H1, int H2)
{
    if (check_x4_stream(n, k, H1, H2)) return (size_t)-1;
    return x4_stream_layout(n, k).L.status;
}

// prologue -> the persistent launch -> out_head -> write-back: four dependent launches on `stream`, no host synchronisation
extern "C" int opnet_stream_step_x4_f32(const float *boxes, const int32_t *slots, float *state, const float *x4packed, float *y,
                                        float *logits, void *workspace, size_t workspace_bytes, int n, int k, int capacity,
                                        int H1, int H2, void *stream)
{
    if (int rc = check_x4_stream(n, k, H1, H2)) return rc;
    if (capacity <= 0) return fail(OPNET_ESHAPE, "capacity=%d must be positive", capacity);
    if (!boxes || !slots || !state || !x4packed || !y || !logits || !workspace) return fail(OPNET_EINVAL, "null pointer");
    if (!aligned16(state) || !aligned16(x4packed) || !aligned16(y) || !aligned16(workspace) || (((uintptr_t)boxes) & 7u) ||
        (((uintptr_t)slots) & 3u) || (((uintptr_t)logits) & 3u))
        return fail(OPNET_EINVAL, "state/x4packed/y/workspace must be 16-byte, boxes 8-byte and slots/logits 4-byte aligned");
    const X4StreamLayout S = x4_stream_layout(n, k);
    if (workspace_bytes < S.total) return fail(OPNET_EWORKSPACE, "workspace %zu B < %zu B", workspace_bytes, S.total);
    int dev = 0;
    if (int rc = persistent_device(&dev)) return rc;
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)workspace;
    const X4InferPacked PK = x4_infer_packed_layout();
    const int RB = (n + 31) / 32;
    StreamX4Args s;
    memset(&s, 0, sizeof(s));
    Xcd4Args &x = s.x;
    x.B = n; x.T = k; x.RB = RB;
    x.pk = x4packed + PK.x4fwd;
    x.woutp = x4packed + PK.woutp;
    x.ws = w;
    x.xp_off = (unsigned)S.L.xp;
    x.h2_off = (unsigned)S.L.h2all;
    x.lg_off = (unsigned)S.L.lgstage; x.ys_off = (unsigned)S.L.ystage;
    x.h1x_off = (unsigned)S.L.h1x; x.h2x_off = (unsigned)S.L.h2x;
    x.cs1_off = (unsigned)S.cs1; x.cs2_off = (unsigned)S.cs2;
    x.status = (unsigned *)(w + S.L.status);
    x.force_safe = env_int("OPNET_XCD_SAFE", 0);
    x.debug = 0;
    g_x4_last_status = x.status;
    s.boxes = boxes;
    s.slots = slots;
    s.state = state;
    s.y = y;
    s.logits = logits;
    s.capacity = capacity;
    opnet_stream_x4_prologue<<<dim3(k + SX4_GATHER, RB), 256, 0, st>>>(s);
    if (int rc = persistent_launch(dev, st, -1, [&] { opnet_xcd4_forward<false, true><<<XCD_COUNT * XCD_CUS, 256, 0, st>>>(x); }))
        return rc;
    opnet_xcd4_out_head<<<dim3(k, RB), 256, 0, st>>>(x, nullptr, nullptr);
    const long outputs = (long)n * OPNET_SLOTS * k, states = (long)RB * 32 * (XCD_H1 + XCD_H2) / 4;
    opnet_stream_x4_writeback<<<ew_blocks(outputs > states ? outputs : states, 1024), 256, 0, st>>>(s);
    HIP_TRY(hipGetLastError());
    return OPNET_OK;
}
