"""GPU tests of ragged DetectorStreams calls (detector_streams.py, opnet_online_encode_ragged_f32): the device encoder with
lengths is bit-exact with its numpy statement, padding frames with new classes never reach a learned slot order,
step_detections with lengths gives the pool's ragged bits without a host sync, and step with per-stream frame lists runs
the detector on the real frames only.  `pytest -m gpu` on the MI355X box."""
import numpy as np
import pytest
import torch

from oracle import detector_oracle as do
from oracle import synth

from test_detector_streams_host import VARIANTS, pad_clip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OPNET_CFG = {"object_to_track_pred_dim": 15, "object_to_track_hidden_dim": 256, "videos_hidden_dim": 512}
CFG = {"opnet": OPNET_CFG, "non_linear_lstm": {"boxes_features_dim": 256, "videos_hidden_dim": 512}}
PARAMS = {"opnet": synth.opnet_synth_params, "non_linear_lstm": synth.non_linear_lstm_synth_params}
_MODELS = {}


def _model(name):
    if name not in _MODELS:
        from objectpermanence_amd import ModelsFactory
        m = ModelsFactory.get_model(name, CFG[name])
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in PARAMS[name](CFG[name]).items()})
        _MODELS[name] = m.eval().to(DEV)
    return _MODELS[name]


def _cone():
    from objectpermanence_amd.datasets import _cone_table
    return _cone_table()


def _clips(n, T, seed=0):
    raws = [synth.make_raw_video(seed + i, VARIANTS[i % 5]) for i in range(n)]
    raws = [(bb[:T], lab[:T]) for bb, lab, _ in raws]
    md = max(len(l) for _, lab in raws for l in lab) + 4
    parts = [pad_clip(bb, lab, np.random.default_rng(seed + 100 + i), md=md) for i, (bb, lab) in enumerate(raws)]
    return tuple(np.stack([p[q] for p in parts]) for q in range(4))


def _dev(det):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in det)


def _same_bits(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), what


def _with_new_classes_in_padding(det, lengths):
    boxes, scores, labels, n_det = (a.copy() for a in det)
    for i, L in enumerate(lengths):
        labels[i, L:, :2] = 100000 + i
        scores[i, L:, :2] = 0.99
        boxes[i, L:, :2] = np.float32(11.0)
        n_det[i, L:] = np.maximum(n_det[i, L:], 2)
    return boxes, scores, labels, n_det


@pytest.mark.parametrize("name", ["opnet", "non_linear_lstm"])
def test_step_detections_with_lengths(name):
    from objectpermanence_amd import DetectorStreams
    from objectpermanence_amd.detector_streams import encode_detections_numpy
    n, K = 6, 8
    lengths = np.array([0, 1, K, 5, K, 3], np.int32)
    det = _with_new_classes_in_padding(_clips(n, K, seed=2), lengths)
    m = _model(name)
    ds = DetectorStreams(m, capacity=8)
    ids = ds.open(n)
    tables_np = ds.tables.cpu().numpy()
    classes_before = ds.get_slot_classes(ids).cpu().numpy()
    r = ds.step_detections(ids, *_dev(det), lengths=lengths)
    torch.cuda.synchronize()
    x_ref = encode_detections_numpy(*det, ids, tables_np, _cone(), ds.n_tracks, lengths=lengths)
    _same_bits(r.x.cpu().numpy(), x_ref, "x")
    assert np.array_equal(ds.tables.cpu().numpy(), tables_np)
    # the padding frames' classes (100000 + i) never reached the learned slot orders
    got = ds.get_slot_classes(ids).cpu().numpy()
    assert not np.isin(got, 100000 + np.arange(n)).any()
    assert np.array_equal(got[lengths == 0], classes_before[lengths == 0])
    # the pool's ragged call on the same input rows
    pool = type(ds.pool)(m, 8)
    pids = pool.open(n)
    out = pool.step(pids, torch.from_numpy(x_ref).to(DEV), lengths)
    y, lg = out if isinstance(out, tuple) else (out, None)
    _same_bits(r.y.cpu().numpy(), y.cpu().numpy(), "y")
    if lg is not None:
        _same_bits(r.logits.cpu().numpy(), lg.cpu().numpy(), "logits")
    _same_bits(ds.pool.state[ids].cpu().numpy(), pool.state[pids].cpu().numpy(), "state")
    px = r.boxes_px.cpu().numpy()
    for i, L in enumerate(lengths):
        assert not px[i, L:].any()
    assert np.array_equal(r.lengths.cpu().numpy(), lengths)


def test_step_detections_device_lengths_do_not_sync():
    from objectpermanence_amd import DetectorStreams
    n, K = 5, 6
    lengths = np.array([2, 0, 6, 1, 4], np.int32)
    det = _dev(_clips(n, K, seed=5))
    m = _model("opnet")
    A, B = DetectorStreams(m, capacity=8), DetectorStreams(m, capacity=8)
    ia, ib = A.open(n), B.open(n)
    ra = A.step_detections(ia, *det, lengths=lengths)
    ld = torch.from_numpy(lengths).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rb = B.step_detections(ib, *det, lengths=ld)
        xb = B.encode(ib, *det, lengths=ld)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    _same_bits(ra.y.cpu().numpy(), rb.y.cpu().numpy(), "y")
    _same_bits(ra.x.cpu().numpy(), rb.x.cpu().numpy(), "x")
    assert xb.shape == ra.x.shape


def test_step_with_per_stream_frame_lists():
    from objectpermanence_amd import DetectorStreams
    from objectpermanence_amd.detector import CaterObjectDetector
    from objectpermanence_amd.detector_streams import encode_detections_numpy
    det = CaterObjectDetector(None, min_size=128, max_size=200)
    det.load_state_dict({**do.synth_backbone_params(), **do.synth_head_params()}, DEV)
    rng = np.random.default_rng(6)
    ks = [2, 0, 3, 1]
    frames = [rng.integers(0, 256, size=(k, 60, 80, 3), dtype=np.uint8) for k in ks]
    m = _model("opnet")
    ds = DetectorStreams(m, detector=det, capacity=8)
    ids = ds.open(len(ks))
    tables_np = ds.tables.cpu().numpy()
    seen = []
    real = CaterObjectDetector._enqueue_padded

    def counting(self, fr, device):
        seen.append(len(fr))
        return real(self, fr, device)
    CaterObjectDetector._enqueue_padded = counting
    try:
        r = ds.step(ids, frames)
    finally:
        CaterObjectDetector._enqueue_padded = real
    torch.cuda.synchronize()
    assert sum(seen) == sum(ks)
    K = max(ks)
    d = tuple(a.cpu().numpy() for a in r.detections)
    assert d[0].shape[:2] == (len(ks), K)
    for i, k in enumerate(ks):
        assert not d[3][i, k:].any()
    _same_bits(r.x.cpu().numpy(), encode_detections_numpy(*d, ids, tables_np, _cone(), 6, lengths=ks), "x")
    assert r.lengths.cpu().numpy().tolist() == ks
    # per-stream calls on the same detections give the same bits
    ref = DetectorStreams(m, capacity=8)
    rid = ref.open(len(ks))
    for i, k in enumerate(ks):
        if k == 0:
            continue
        ri = ref.step_detections([rid[i]], *(torch.from_numpy(np.ascontiguousarray(a[i:i + 1, :k])).to(DEV) for a in d))
        torch.cuda.synchronize()
        _same_bits(r.y[i, :k].cpu().numpy(), ri.y[0].cpu().numpy(), f"y stream {i}")
        _same_bits(r.logits[i, :, :k].cpu().numpy(), ri.logits[0].cpu().numpy(), f"logits stream {i}")
        _same_bits(r.x[i, :k].cpu().numpy(), ri.x[0].cpu().numpy(), f"x stream {i}")
    _same_bits(ds.pool.state[ids].cpu().numpy(), ref.pool.state[rid].cpu().numpy(), "state")
    with pytest.raises(ValueError):
        ds.step(ids[:2], [np.zeros((1, 60, 80, 3), np.uint8), np.zeros((1, 50, 80, 3), np.uint8)])
