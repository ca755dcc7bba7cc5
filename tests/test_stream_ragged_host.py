"""CPU-side checks of the ragged stream steps (include/opnet_hip.h opnet_stream_step_ragged_f32, opseq_stream_step_ragged_f32,
opnet_online_encode_ragged_f32; streaming.check_lengths; detector_streams.encode_detections_numpy with lengths): the new
entry points exist and refuse bad arguments before anything is launched, and the encoder's statement treats frames past a
stream's length as frames without detections."""
import numpy as np
import pytest

from test_detector_streams_host import VARIANTS, pad_clip
from oracle import synth

EINVAL, ESHAPE, EWORKSPACE = -1, -2, -3
P = 1 << 20          # a fake 16-byte aligned device address: every refusal below happens before a launch


def _lib():
    from objectpermanence_amd import _lib, build
    build.build()
    return _lib.load()


def test_ragged_symbols_are_declared_and_exported():
    from objectpermanence_amd import _lib as L
    lib = _lib()
    for name in ("opnet_stream_step_ragged_f32", "opseq_stream_step_ragged_f32", "opnet_online_encode_ragged_f32"):
        assert name in L.EXPORTS
        assert getattr(lib, name).argtypes is not None
    assert lib.opnet_hip_abi_version() == 9


def test_opnet_ragged_step_refusals():
    lib = _lib()
    # the workspace is the uniform call's for n x K
    assert lib.opnet_stream_workspace_bytes(70, 3, 256, 512) == lib.opnet_workspace_bytes(70, 3, 256, 512)
    f = lib.opnet_stream_step_ragged_f32
    # boxes, slots, lengths, state, packed, y, logits, workspace, bytes, n, k, capacity, H1, H2, mlp, stream
    assert f(P, P, None, P, P, P, P, P, 1 << 30, 1, 1, 4, 256, 512, 0, None) == EINVAL
    assert b"lengths" in lib.opnet_last_error()
    assert f(P, P, P, P, P, P, P, P, 1 << 30, 1, 0, 4, 256, 512, 0, None) == ESHAPE
    assert f(P, P, P, P, P, P, P, P, 1 << 30, 0, 1, 4, 256, 512, 0, None) == ESHAPE
    assert f(P, P, P, P, P, P, P, P, 1 << 30, 1, 1, 4, 250, 512, 0, None) == ESHAPE
    assert f(P, P, P, P, P, P, P, P, 1 << 30, 1, 1, 0, 256, 512, 0, None) == ESHAPE
    assert f(P, P, P + 2, P, P, P, P, P, 1 << 30, 1, 1, 4, 256, 512, 0, None) == EINVAL
    assert b"aligned" in lib.opnet_last_error()
    assert f(P, P, P, P + 4, P, P, P, P, 1 << 30, 1, 1, 4, 256, 512, 0, None) == EINVAL
    assert f(P, P, P, P, P, P, P, P, 64, 1, 1, 4, 256, 512, 0, None) == EWORKSPACE
    assert b"workspace" in lib.opnet_last_error()


def test_opseq_ragged_step_refusals():
    lib = _lib()
    assert lib.opseq_stream_workspace_bytes(70, 3, 2, 3840, 512) == lib.opseq_lstm_stack_workspace_bytes(70, 3, 2, 3840, 512)
    f = lib.opseq_stream_step_ragged_f32
    # x, slots, lengths, state, packed, y, workspace, bytes, n, k, capacity, L, KX, H, stream
    assert f(P, P, None, P, P, P, P, 1 << 30, 1, 1, 4, 1, 75, 512, None) == EINVAL
    assert b"lengths" in lib.opnet_last_error()
    assert f(P, P, P, P, P, P, P, 1 << 30, 1, 0, 4, 1, 75, 512, None) == ESHAPE
    assert f(P, P, P, P, P, P, P, 1 << 30, 1, 1, 4, 4, 75, 512, None) == ESHAPE
    assert f(P, P, P, P, P, P, P, 1 << 30, 1, 1, 0, 1, 75, 512, None) == ESHAPE
    assert f(P, P, P + 1, P, P, P, P, 1 << 30, 1, 1, 4, 1, 75, 512, None) == EINVAL
    assert b"aligned" in lib.opnet_last_error()
    assert f(P + 4, P, P, P, P, P, P, 1 << 30, 1, 1, 4, 2, 3840, 512, None) == EINVAL      # hoisted x must be 16-byte
    assert f(P, P, P, P, P, P, P, 64, 1, 1, 4, 1, 75, 512, None) == EWORKSPACE


def test_online_encode_ragged_refusals():
    lib = _lib()
    f = lib.opnet_online_encode_ragged_f32
    # boxes, scores, labels, n_det, lengths, md, slots, tables, capacity, cone, num_classes, n, k, n_tracks, thresh, out, st
    assert f(P, P, P, P, None, 8, P, P, 4, P, 200, 1, 1, 6, 0.8, P, None) == EINVAL
    assert b"lengths" in lib.opnet_last_error()
    assert f(P, P, P, P, P + 2, 8, P, P, 4, P, 200, 1, 1, 6, 0.8, P, None) == EINVAL
    assert b"aligned" in lib.opnet_last_error()
    assert f(P, P, P, P, P, 8, P, P, 4, P, 200, 1, 1, 7, 0.8, P, None) == ESHAPE
    assert f(P, P, P, P, P, 8, P, P, 4, P, 200, 1, 0, 6, 0.8, P, None) == ESHAPE
    assert f(P, P, P, P, P, 0, P, P, 4, P, 200, 1, 1, 6, 0.8, P, None) == ESHAPE


def test_host_lengths_are_checked():
    from objectpermanence_amd.streaming import check_lengths
    assert check_lengths([0, 3, 1], 3, 3).dtype == np.int32
    assert check_lengths(np.array([2, 2], np.uint8), 2, 2).tolist() == [2, 2]
    with pytest.raises(ValueError, match=r"\[n=3\]"):
        check_lengths([1, 2], 3, 3)
    with pytest.raises(ValueError, match=r"\[n=2\]"):
        check_lengths([[1, 2]], 2, 3)
    with pytest.raises(TypeError, match="integers"):
        check_lengths([1.0, 2.0], 2, 3)
    with pytest.raises(ValueError, match="0, k=3"):
        check_lengths([1, 4], 2, 3)
    with pytest.raises(ValueError, match="0, k=3"):
        check_lengths([-1, 2], 2, 3)


# ---- the encoder's statement with lengths --------------------------------------------------------------------------------
def _streams(n, T, seed):
    """n streams of T frames of padded detections (common md) -> numpy (boxes, scores, labels, n_det) [n, T, ...]"""
    raws = [synth.make_raw_video(seed + i, VARIANTS[i % 5]) for i in range(n)]
    raws = [(bb[:T], lab[:T]) for bb, lab, _ in raws]
    md = max(len(l) for _, lab in raws for l in lab) + 4
    parts = [pad_clip(bb, lab, np.random.default_rng(seed + 50 + i), md=md) for i, (bb, lab) in enumerate(raws)]
    return tuple(np.stack([p[q] for p in parts]) for q in range(4))


def _fresh_tables(capacity, fixed=None):
    from objectpermanence_amd.detector_streams import table_row
    t = np.tile(table_row(None), (capacity, 1))
    for slot, classes in (fixed or {}).items():
        t[slot] = table_row(classes)
    return t


@pytest.mark.parametrize("n_tracks", [5, 6])
def test_encode_with_lengths_equals_the_unpadded_streams(n_tracks):
    from objectpermanence_amd.detector_streams import encode_detections_numpy
    from objectpermanence_amd.datasets import _cone_table
    n, K = 5, 9
    lengths = np.array([0, 1, K, 4, K], np.int32)
    det = _streams(n, K, seed=3)
    boxes, scores, labels, n_det = det
    # the padding frames hold classes no valid frame has, above the threshold: they must not reach any table
    boxes, scores, labels, n_det = (a.copy() for a in det)
    for i, L in enumerate(lengths):
        labels[i, L:, :2] = 100000 + i
        scores[i, L:, :2] = 0.99
        n_det[i, L:] = np.maximum(n_det[i, L:], 2)
        boxes[i, L:, :2] = 7.5
    slots = [3, 0, 6, 1, 4]
    cone = _cone_table()
    fixed = {6: [140, 100000, 100001, 100002, 100003, 100004, 1, 2, 3]}      # a fixed row that ranks the padding classes
    tables = _fresh_tables(8, fixed)
    x = encode_detections_numpy(boxes, scores, labels, n_det, slots, tables, cone, n_tracks, lengths=lengths)
    assert x.shape == (n, K, 15, n_tracks)
    want_tables = _fresh_tables(8, fixed)
    for i, L in enumerate(lengths):
        assert not x[i, L:].any(), "padding frames encode as zeros"
        if L == 0:
            continue
        one = encode_detections_numpy(*(a[i:i + 1, :L] for a in (boxes, scores, labels, n_det)), [slots[i]], want_tables,
                                      cone, n_tracks)
        assert np.array_equal(x[i, :L].view(np.uint32), one[0].view(np.uint32))
    assert np.array_equal(tables, want_tables)
    for i in range(n):
        if slots[i] != 6:
            assert not np.isin(tables[slots[i], :15], 100000 + np.arange(n)).any()
    # lengths = K everywhere, and None, are the uniform statement
    t1, t2 = _fresh_tables(8, fixed), _fresh_tables(8, fixed)
    a = encode_detections_numpy(*det, slots, t1, cone, n_tracks, lengths=[K] * n)
    b = encode_detections_numpy(*det, slots, t2, cone, n_tracks)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(t1, t2)


def test_learn_tables_with_lengths_ignores_padding():
    from objectpermanence_amd.detector_streams import learn_tables_numpy
    n, K = 3, 6
    boxes, scores, labels, n_det = _streams(n, K, seed=11)
    labels = labels.copy()
    scores = scores.copy()
    labels[:, 2:, 0] = 100099
    scores[:, 2:, 0] = 1.0
    n_det = np.maximum(n_det, 1)
    tables = _fresh_tables(4)
    learn_tables_numpy(tables, [0, 1, 2], scores, labels, n_det, lengths=[2, 0, 1])
    want = _fresh_tables(4)
    learn_tables_numpy(want, [0], scores[:1, :2], labels[:1, :2], n_det[:1, :2])
    learn_tables_numpy(want, [2], scores[2:, :1], labels[2:, :1], n_det[2:, :1])
    assert np.array_equal(tables, want)
    assert not (tables == 100099).any()
