// online_encode_abi.hip - host side of the per-frame input encoder (C ABI: opnet_online_encode_f32; kernels in
// online_encode_kernels.hip).  Included by opnet_abi.hip (one translation unit: it uses that file's fail / HIP_TRY /
// aligned16).
#pragma once

// learn -> encode: 2 launches on `stream`, no host synchronisation.  lengths: device [n] frames per stream, or null for k
static int online_encode(const float *det_boxes, const float *det_scores, const int64_t *det_labels, const int32_t *n_det,
                         const int32_t *lengths, int md, const int32_t *slots, int32_t *tables, int capacity,
                         const uint8_t *cone_mask, int num_classes, int n, int k, int n_tracks, float score_thresh, float *out,
                         void *stream)
{
    if (!det_boxes || !det_scores || !det_labels || !n_det || !slots || !tables || !cone_mask || !out)
        return fail(OPNET_EINVAL, "null pointer");
    if (!aligned16(det_boxes) || !aligned16(tables) || (((uintptr_t)det_labels) & 7u) || (((uintptr_t)det_scores) & 3u) ||
        (((uintptr_t)n_det) & 3u) || (((uintptr_t)slots) & 3u) || (((uintptr_t)out) & 3u) ||
        (((uintptr_t)lengths) & 3u))
        return fail(OPNET_EINVAL, "det_boxes/tables must be 16-byte, det_labels 8-byte and det_scores/n_det/lengths/slots/out "
                                  "4-byte aligned");
    if (n_tracks != 5 && n_tracks != 6) return fail(OPNET_ESHAPE, "n_tracks=%d must be 5 or 6", n_tracks);
    if (n <= 0 || k <= 0 || md <= 0 || capacity <= 0 || num_classes <= 0)
        return fail(OPNET_ESHAPE, "n=%d k=%d md=%d capacity=%d num_classes=%d must be positive", n, k, md, capacity,
                    num_classes);
    if ((long)n * k * md > (1L << 40)) return fail(OPNET_ESHAPE, "n*k*md=%ld rows is too many", (long)n * k * md);

    OnlineArgs a;
    a.boxes = det_boxes;
    a.scores = det_scores;
    a.labels = (const long long *)det_labels;
    a.n_det = n_det;
    a.len = lengths;
    a.slots = slots;
    a.tables = tables;
    a.cone = cone_mask;
    a.out = out;
    a.md = md;
    a.capacity = capacity;
    a.num_classes = num_classes;
    a.n = n;
    a.k = k;
    a.n_tracks = n_tracks;
    a.thresh = score_thresh;
    const long items = (long)n * k;
    if ((items + 3) / 4 > 0x7fffffffL) return fail(OPNET_ESHAPE, "n*k=%ld frames exceed one launch", items);
    hipStream_t st = (hipStream_t)stream;
    // fixed rows leave the learn kernel at once; the encode kernel reads what it wrote (stream order)
    opnet_online_learn<<<n, 256, 0, st>>>(a);
    opnet_online_encode<<<(unsigned)((items + 3) / 4), 256, 0, st>>>(a);
    HIP_TRY(hipGetLastError());
    return OPNET_OK;
}

extern "C" int opnet_online_encode_f32(const float *det_boxes, const float *det_scores, const int64_t *det_labels,
                                       const int32_t *n_det, int md, const int32_t *slots, int32_t *tables, int capacity,
                                       const uint8_t *cone_mask, int num_classes, int n, int k, int n_tracks,
                                       float score_thresh, float *out, void *stream)
{
    return online_encode(det_boxes, det_scores, det_labels, n_det, nullptr, md, slots, tables, capacity, cone_mask, num_classes,
                         n, k, n_tracks, score_thresh, out, stream);
}

// stream i's frames j >= lengths[i] (device int32 [n], clamped to [0, k]) are padding: n_det = 0
extern "C" int opnet_online_encode_ragged_f32(const float *det_boxes, const float *det_scores, const int64_t *det_labels,
                                              const int32_t *n_det, const int32_t *lengths, int md, const int32_t *slots,
                                              int32_t *tables, int capacity, const uint8_t *cone_mask, int num_classes, int n,
                                              int k, int n_tracks, float score_thresh, float *out, void *stream)
{
    if (!lengths) return fail(OPNET_EINVAL, "null pointer: lengths");
    return online_encode(det_boxes, det_scores, det_labels, n_det, lengths, md, slots, tables, capacity, cone_mask, num_classes,
                         n, k, n_tracks, score_thresh, out, stream);
}
