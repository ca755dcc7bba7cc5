"""GPU tests of DetectorStreams (objectpermanence_amd/detector_streams.py, csrc/online_encode_kernels.hip): the device
encoder is bit-exact with its numpy statement (tables included), step_detections gives the bits of the pools and of the
launch-chain forward for the four streamable reasoners, step runs frames through the detector without a host read-back,
nothing in step_detections / encode synchronises the host, and bad input is refused.  `pytest -m gpu` on the MI355X box."""
import numpy as np
import pytest
import torch

from oracle import detector_oracle as do
from oracle import synth

from test_detector_streams_host import VARIANTS, _with_union_first_frame, pad_clip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OPNET_CFG = {"object_to_track_pred_dim": 15, "object_to_track_hidden_dim": 256, "videos_hidden_dim": 512}
CFG = {"opnet": OPNET_CFG, "opnet_lstm_mlp": OPNET_CFG, "baseline_lstm": {"videos_hidden_dim": 512},
       "non_linear_lstm": {"boxes_features_dim": 256, "videos_hidden_dim": 512}}
PARAMS = {"opnet": synth.opnet_synth_params, "opnet_lstm_mlp": synth.opnet_lstm_mlp_synth_params,
          "baseline_lstm": synth.baseline_lstm_synth_params, "non_linear_lstm": synth.non_linear_lstm_synth_params}
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
    """n streams of padded detections (the five variants in turn), common md -> numpy (boxes, scores, labels, n_det)
    [n, T, ...] and the raw (bb, lab) lists"""
    raws = [synth.make_raw_video(seed + i, VARIANTS[i % 5]) for i in range(n)]
    raws = [(bb[:T], lab[:T]) for bb, lab, _ in raws]
    md = max(len(l) for _, lab in raws for l in lab) + 4
    parts = [pad_clip(bb, lab, np.random.default_rng(seed + 100 + i), md=md) for i, (bb, lab) in enumerate(raws)]
    return tuple(np.stack([p[q] for p in parts]) for q in range(4)), raws


def _dev(det):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in det)


def _schedules(T):
    return {"1-7-rest": [1, 7, T - 8], "k7": [7] * (T // 7) + ([T % 7] if T % 7 else []), "whole": [T]}


def _encode_both(ds, ids, det, chunks, tables_np):
    """the device encoder and the statement over the same chunks -> (x device, x statement) numpy [n, T, 15, nt]"""
    from objectpermanence_amd.detector_streams import encode_detections_numpy
    xs, xr, t = [], [], 0
    for k in chunks:
        sl = tuple(a[:, t:t + k] for a in det)
        xs.append(ds.encode(ids, *_dev(sl)))
        xr.append(encode_detections_numpy(*sl, ids, tables_np, _cone(), ds.n_tracks))
        t += k
    torch.cuda.synchronize()
    return torch.cat(xs, dim=1).cpu().numpy(), np.concatenate(xr, axis=1)


def _same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    assert np.array_equal(a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint8),
                          b.view(np.uint32 if b.dtype.itemsize == 4 else np.uint8)), f"max |diff| {np.abs(a - b).max():.3e}"


# ---- 1. the kernel against the statement ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["opnet", "baseline_lstm"])           # 6 and 5 tracks
@pytest.mark.parametrize("mode", ["fixed", "learned"])
@pytest.mark.parametrize("n,T", [(1, 60), (5, 300), (33, 40)])
def test_kernel_equals_statement(name, mode, n, T):
    from objectpermanence_amd import DetectorStreams
    from objectpermanence_amd.datasets import slot_order
    det, raws = _clips(n, T, seed=3 * n)
    for sched, chunks in _schedules(T).items():
        ds = DetectorStreams(_model(name), capacity=80)
        filler = ds.open(7)                                  # rows the calls do not name
        ids = ds.open(n, classes=None if mode == "learned" else [slot_order(lab) for _, lab in raws])
        ds.close(filler[::2])
        before = ds.tables.cpu().numpy()
        tables_np = before.copy()
        x, x_ref = _encode_both(ds, ids, det, chunks, tables_np)
        _same_bits(x, x_ref)
        after = ds.tables.cpu().numpy()
        assert np.array_equal(after, tables_np), sched
        others = np.setdiff1d(np.arange(80), ids)
        assert np.array_equal(after[others], before[others])
        if mode == "fixed":
            assert np.array_equal(after, before)


@pytest.mark.parametrize("md", [100, 150])
def test_kernel_fuzz(md):
    from objectpermanence_amd import DetectorStreams
    rng = np.random.default_rng(md)
    n, T = 9, 24
    boxes = rng.uniform(-1.0, 330.0, size=(n, T, md, 4)).astype(np.float32)
    scores = rng.uniform(0.5, 1.0, size=(n, T, md)).astype(np.float32)
    scores[rng.random((n, T, md)) < 0.05] = np.float32(0.8)
    labels = rng.integers(1, 193, size=(n, T, md)).astype(np.int64)
    labels[rng.random((n, T, md)) < 0.1] = 140
    n_det = rng.integers(0, md + 1, size=(n, T)).astype(np.int32)
    n_det[:, ::5] = 0
    for name in ("opnet", "non_linear_lstm"):
        for mode in ("fixed", "learned"):
            ds = DetectorStreams(_model(name), capacity=32)
            pool_ids = np.setdiff1d(np.arange(1, 193), [140])
            classes = None if mode == "learned" else [list(rng.permutation(pool_ids)[:int(rng.integers(0, 20))])
                                                      + ([140] if i % 2 else []) for i in range(n)]
            ids = ds.open(n, classes=classes)
            tables_np = ds.tables.cpu().numpy()
            x, x_ref = _encode_both(ds, ids, (boxes, scores, labels, n_det), [1, 5, T - 6], tables_np)
            _same_bits(x, x_ref)
            assert np.array_equal(ds.tables.cpu().numpy(), tables_np)
            if mode == "learned":
                assert (tables_np[ids, :15] != -1).all()     # 192 classes seen: every learned row is full


def test_reopened_id_starts_fresh():
    from objectpermanence_amd import DetectorStreams
    from objectpermanence_amd.detector_streams import table_row
    ds = DetectorStreams(_model("opnet"), capacity=4)
    det, _ = _clips(2, 20)
    ids = ds.open(2)
    r = ds.step_detections(ids, *_dev(det))
    torch.cuda.synchronize()
    assert (ds.get_slot_classes(ids).cpu().numpy()[:, 1] != -1).all()
    ds.close([ids[1]])
    again = ds.open(1, classes=[[3, 140]])
    assert again == [ids[1]]
    assert ds.get_slot_classes(again).cpu().numpy().tolist() == [table_row([3, 140])[:15].tolist()]
    assert all(float(s.abs().sum()) == 0.0 for s in ds.get_state(again))
    ds.close(again)
    assert ds.open(1) == [ids[1]]
    assert ds.get_slot_classes([ids[1]]).cpu().numpy().tolist() == [table_row(None)[:15].tolist()]
    assert r.boxes_px.shape == (2, 20, 4)


# ---- 2. step_detections for the four streamable models ----------------------------------------------------------------
def _chain(m, x):
    """the whole-clip launch-chain forward -> numpy (y, logits | None)"""
    xb = torch.from_numpy(x).to(DEV)
    with torch.no_grad():
        if hasattr(m, "_runner"):
            m._runner.use_xcd = "0"
            try:
                out = m(xb)
            finally:
                m._runner.use_xcd = "auto"
        elif hasattr(m, "use_xcd"):
            m.use_xcd = "0"
            try:
                out = m(xb)
            finally:
                m.use_xcd = "auto"
        else:
            out = m(xb)
    torch.cuda.synchronize()
    y, lg = out if isinstance(out, tuple) else (out, None)
    return y.cpu().numpy(), None if lg is None else lg.cpu().numpy()


def _pool(m, capacity=16):
    from objectpermanence_amd import LstmStackStreams, OPNetStreams
    from objectpermanence_amd.learned_models import OPNet, OPNetLstmMlp
    return OPNetStreams(m, capacity) if isinstance(m, (OPNet, OPNetLstmMlp)) else LstmStackStreams(m, capacity)


@pytest.mark.parametrize("name", ["opnet", "opnet_lstm_mlp", "baseline_lstm", "non_linear_lstm"])
@pytest.mark.parametrize("mode", ["fixed", "learned"])
def test_step_detections_equals_pool_and_chain(name, mode):
    from objectpermanence_amd import DetectorStreams
    from objectpermanence_amd.datasets import slot_order
    from objectpermanence_amd.detector_streams import encode_detections_numpy
    from objectpermanence_amd.metrics import postprocess_and_iou
    m = _model(name)
    T, n = 300, 5
    det, raws = _clips(n, T, seed=50)
    if mode == "learned":      # the condition under which learned orders equal the offline ones
        rng = np.random.default_rng(9)
        raws = [_with_union_first_frame(bb, lab, rng) for bb, lab in raws]
        md = max(len(l) for _, lab in raws for l in lab) + 4
        parts = [pad_clip(bb, lab, np.random.default_rng(i), md=md) for i, (bb, lab) in enumerate(raws)]
        det = tuple(np.stack([p[q] for p in parts]) for q in range(4))
    results = {}
    for sched, chunks in _schedules(T).items():
        ds = DetectorStreams(m, capacity=16)
        ds.open(3)
        ids = ds.open(n, classes=None if mode == "learned" else [slot_order(lab) for _, lab in raws])
        tables_np = ds.tables.cpu().numpy()
        pool = _pool(m)
        pids = pool.open(n)
        ys, lgs, pxs, ys_ref, lgs_ref, t = [], [], [], [], [], 0
        for k in chunks:
            sl = tuple(a[:, t:t + k] for a in det)
            r = ds.step_detections(ids, *_dev(sl))
            x_ref = encode_detections_numpy(*sl, ids, tables_np, _cone(), ds.n_tracks)
            out = pool.step(pids, torch.from_numpy(x_ref).to(DEV))
            y_ref, lg_ref = out if isinstance(out, tuple) else (out, None)
            _same_bits(r.x.cpu().numpy(), x_ref)
            ys.append(r.y); pxs.append(r.boxes_px); ys_ref.append(y_ref)
            if r.logits is not None:
                lgs.append(r.logits); lgs_ref.append(lg_ref)
            else:
                assert lg_ref is None
            t += k
        torch.cuda.synchronize()
        y = torch.cat(ys, 1).cpu().numpy()
        _same_bits(y, torch.cat(ys_ref, 1).cpu().numpy())
        px = torch.cat(pxs, 1)
        assert torch.equal(px, postprocess_and_iou(torch.from_numpy(y).to(DEV))[0])
        lg = torch.cat(lgs, 2).cpu().numpy() if lgs else None
        if lg is not None:
            _same_bits(lg, torch.cat(lgs_ref, 2).cpu().numpy())
        results[sched] = (y, lg)
    from objectpermanence_amd.datasets import encode_boxes
    x_clip = np.stack([encode_boxes(bb, lab, 6 if name.startswith("opnet") else 5).astype(np.float32) for bb, lab in raws])
    y_c, lg_c = _chain(m, x_clip)
    for sched, (y, lg) in results.items():
        _same_bits(y, y_c)
        if lg is not None:
            _same_bits(lg, lg_c)


def test_transformer_lstm_is_refused():
    from objectpermanence_amd import DetectorStreams, ModelsFactory
    m = ModelsFactory.get_model("transformer_lstm", {"boxes_features_dim": 16, "num_attention_heads": 2,
                                                     "num_attention_layers": 1, "lstm_hidden_dim": 32,
                                                     "num_lstm_layers": 2}).eval().to(DEV)
    with pytest.raises(TypeError, match="not streamed"):
        DetectorStreams(m)


# ---- 3. frames through the synthetic detector -------------------------------------------------------------------------
MIN_SIZE, MAX_SIZE = 128, 200


def _match_fraction(got_b, got_l, want_b, want_l, tol=1.0):
    hits = 0
    for b, l in zip(want_b, want_l):
        cand = got_b[got_l == l]
        hits += bool(len(cand) and np.abs(cand - b).max(axis=1).min() < tol)
    return hits / max(1, len(want_l))


def test_step_frames_through_the_detector(monkeypatch):
    from objectpermanence_amd import DetectorStreams
    from objectpermanence_amd.detector import CaterObjectDetector
    from objectpermanence_amd.detector_streams import encode_detections_numpy
    det = CaterObjectDetector(None, min_size=MIN_SIZE, max_size=MAX_SIZE)
    det.load_state_dict({**do.synth_backbone_params(), **do.synth_head_params()}, DEV)
    rng = np.random.default_rng(4)
    n, T = 3, 12
    frames = rng.integers(0, 256, size=(n, T, 60, 80, 3), dtype=np.uint8)
    m = _model("opnet")
    ds = DetectorStreams(m, detector=det, capacity=8)
    ids = ds.open(n)
    tables_np = ds.tables.cpu().numpy()
    pool = _pool(m)
    pids = pool.open(n)

    def refuse(*a, **k):
        raise AssertionError("a host read-back of the detections")
    monkeypatch.setattr(CaterObjectDetector, "_finish", refuse)
    monkeypatch.setattr(CaterObjectDetector, "remove_low_probability_object", staticmethod(refuse))
    dets, t = [], 0
    for k in (1, 4, 7):
        r = ds.step(ids, frames[:, t:t + k])
        torch.cuda.synchronize()
        d = tuple(a.cpu().numpy() for a in r.detections)
        assert d[0].shape[:2] == (n, k) and d[3].shape == (n, k)
        x_ref = encode_detections_numpy(*d, ids, tables_np, _cone(), 6)
        _same_bits(r.x.cpu().numpy(), x_ref)
        y_ref, lg_ref = pool.step(pids, torch.from_numpy(x_ref).to(DEV))
        _same_bits(r.y.cpu().numpy(), y_ref.cpu().numpy())
        _same_bits(r.logits.cpu().numpy(), lg_ref.cpu().numpy())
        dets.append(d)
        t += k
    assert np.array_equal(ds.tables.cpu().numpy(), tables_np)
    # more frames than one pass holds: one stream's frames in passes of MAX_FRAMES_PER_PASS
    long = rng.integers(0, 256, size=(1, det.MAX_FRAMES_PER_PASS + 2, 60, 80, 3), dtype=np.uint8)
    r = ds.step([ids[1]], long)
    torch.cuda.synchronize()
    d = tuple(a.cpu().numpy() for a in r.detections)
    _same_bits(r.x.cpu().numpy(), encode_detections_numpy(*d, [ids[1]], tables_np, _cone(), 6))
    monkeypatch.undo()
    # the detections used agree with detect_batch + remove_low_probability_object (the existing perception bar)
    got_b = np.concatenate([d[0] for d in dets], axis=1)
    got_s = np.concatenate([d[1] for d in dets], axis=1)
    got_l = np.concatenate([d[2] for d in dets], axis=1)
    got_n = np.concatenate([d[3] for d in dets], axis=1)
    fr, total = [], 0
    for i in range(n):
        outs = det.detect_batch(list(frames[i]), torch.device(DEV))
        for j, o in enumerate(outs):
            kept = CaterObjectDetector.remove_low_probability_object(o, 0.8)
            kf = int((got_s[i, j, :got_n[i, j]] >= np.float32(0.8)).sum())
            wb, wl = kept["boxes"].cpu().numpy(), kept["labels"].cpu().numpy()
            total += len(wl)
            fr.append(_match_fraction(got_b[i, j, :kf], got_l[i, j, :kf], wb, wl) * len(wl))
    assert total > 0
    assert sum(fr) / total >= 0.9


# ---- 4. no host sync ------------------------------------------------------------------------------------------------
def test_step_detections_and_encode_do_not_sync():
    from objectpermanence_amd import DetectorStreams
    det, _ = _clips(4, 10, seed=7)
    for name in ("opnet", "non_linear_lstm"):
        ds = DetectorStreams(_model(name), capacity=8)
        ids = ds.open(4)
        dd = _dev(det)
        ds.step_detections(ids, *dd)        # first call: weight image and workspaces
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            r = ds.step_detections(ids, *dd)
            x = ds.encode(ids, *dd)
            with pytest.raises(RuntimeError):
                r.y.sum().item()            # the mode is live on this build
        finally:
            torch.cuda.set_sync_debug_mode(0)
        torch.cuda.synchronize()
        assert x.shape == (4, 10, 15, ds.n_tracks) and r.boxes_px.dtype == torch.int32


# ---- 5. refusals and side streams -----------------------------------------------------------------------------------
def test_refusals():
    from objectpermanence_amd import DetectorStreams, _lib
    m = _model("opnet")
    with pytest.raises(ValueError):
        DetectorStreams(m, n_tracks=5)
    ds = DetectorStreams(m, capacity=4)
    ids = ds.open(2)
    det = _dev(_clips(2, 6)[0])
    b, s, l, nd = det
    with pytest.raises(ValueError):
        ds.encode(ids, b[:, :, :, :3], s, l, nd)
    with pytest.raises(ValueError):
        ds.encode(ids, b, s[:, :3], l, nd)
    with pytest.raises(ValueError):
        ds.encode(ids, b, s, l, nd[:1])
    with pytest.raises(TypeError):
        ds.encode(ids, b.double(), s, l, nd)
    with pytest.raises(TypeError):
        ds.encode(ids, b, s, l.int(), nd)
    with pytest.raises(RuntimeError):
        ds.encode(ids, b.cpu(), s, l, nd)
    with pytest.raises(ValueError):
        ds.encode([ids[0]], b, s, l, nd)
    ds.close([ids[1]])
    with pytest.raises(KeyError):
        ds.step_detections(ids, b, s, l, nd)
    with pytest.raises(IndexError):
        ds.encode([ids[0], 9], b, s, l, nd)
    with pytest.raises(ValueError):
        ds.open(2, classes=[[1, 2]])
    with pytest.raises(RuntimeError):
        ds.step([ids[0]], np.zeros((1, 1, 60, 80, 3), np.uint8))          # no detector
    # the C ABI on real device buffers
    lib = _lib.load()
    out = torch.empty((2, 6, 15, 6), device=DEV)
    slots = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    cone = ds.cone_mask
    md = int(b.shape[2])

    def call(bp=b.data_ptr(), tp=ds.tables.data_ptr(), lp=l.data_ptr(), op=out.data_ptr(), nt=6):
        return lib.opnet_online_encode_f32(bp, s.data_ptr(), lp, nd.data_ptr(), md, slots.data_ptr(), tp, 4, cone.data_ptr(),
                                           193, 2, 6, nt, 0.8, op, torch.cuda.current_stream().cuda_stream)
    assert call(bp=None) == -1 and call(tp=None) == -1 and call(op=None) == -1
    assert call(bp=b.data_ptr() + 4) == -1 and call(tp=ds.tables.data_ptr() + 8) == -1 and call(lp=l.data_ptr() + 4) == -1
    assert call(nt=7) == -2
    assert b"n_tracks" in lib.opnet_last_error()


def test_side_stream_gives_the_same_bits():
    from objectpermanence_amd import DetectorStreams
    m = _model("opnet")
    det = _dev(_clips(3, 16, seed=2)[0])
    out = []
    for side in (False, True):
        ds = DetectorStreams(m, capacity=4)
        ids = ds.open(3)
        st = torch.cuda.Stream() if side else torch.cuda.current_stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            r1 = ds.step_detections(ids, *(a[:, :5] for a in det))
            r2 = ds.step_detections(ids, *(a[:, 5:] for a in det))
            x = ds.encode(ids, *(a[:, :2] for a in det))
        torch.cuda.synchronize()
        out.append([t.cpu().numpy() for t in (r1.y, r1.logits, r2.y, r2.logits, r2.boxes_px, x, ds.tables)])
    for a, b in zip(*out):
        assert np.array_equal(a, b)
