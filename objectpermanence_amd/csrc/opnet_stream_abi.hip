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
