"""GPU test of DetectorStreams on the persistent engine (objectpermanence_amd/detector_streams.py engine="persistent"): a
300-frame backlog of detections goes through step_detections as ONE persistent launch, the stream then ticks frame by frame
on the launch chain; the encoded rows equal the numpy encoder's bit for bit and the outputs stay within the fp64 oracle's
bounds across the hand-over; and a replay of the pool's log derives the pixel boxes again from the rewritten y.
`pytest -m gpu` on the MI355X box."""
import numpy as np
import pytest
import torch

from oracle import opnet_oracle as oo
from oracle import synth

from test_detector_streams_gpu import _clips, _cone, _dev, _same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CFG = {"object_to_track_pred_dim": 15, "object_to_track_hidden_dim": 256, "videos_hidden_dim": 512}
TOL_Y = 2e-5          # the project's bounds over 300 steps (tests/test_opnet_stream_gpu.py)
TOL_LOGITS = 1e-4
BACKLOG, TICKS = 300, 6


def test_backlog_on_the_persistent_engine_then_chain_ticks():
    from objectpermanence_amd import DetectorStreams, ModelsFactory
    from objectpermanence_amd.datasets import slot_order
    from objectpermanence_amd.detector_streams import encode_detections_numpy
    from objectpermanence_amd.metrics import postprocess_and_iou
    params = synth.opnet_synth_params(CFG)
    m = ModelsFactory.get_model("opnet", CFG)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    m.eval().to(DEV)
    n = 5
    det, raws = _clips(n, BACKLOG, seed=50)
    live, _ = _clips(n, TICKS, seed=80)                 # what the cameras see next: other detections, same padded width or not
    ds = DetectorStreams(m, capacity=16)                # the pool's default stays the chain; the backlog call names its engine
    ds.open(3)
    ids = ds.open(n, classes=[slot_order(lab) for _, lab in raws])
    tables_np = ds.tables.cpu().numpy()
    with pytest.raises(ValueError, match="ragged"):     # refused before anything is encoded
        ds.step_detections(ids, *_dev(det), lengths=[BACKLOG] * n, engine="persistent")
    assert np.array_equal(ds.tables.cpu().numpy(), tables_np)
    results = [ds.step_detections(ids, *_dev(det), engine="persistent")]
    xs = [encode_detections_numpy(*det, ids, tables_np, _cone(), 6)]
    for t in range(TICKS):
        sl = tuple(a[:, t:t + 1] for a in live)
        results.append(ds.step_detections(ids, *_dev(sl)))
        xs.append(encode_detections_numpy(*sl, ids, tables_np, _cone(), 6))
    torch.cuda.synchronize()
    assert ds.verify_launches() == 0
    x_ref = np.concatenate(xs, axis=1)
    _same_bits(torch.cat([r.x for r in results], dim=1).cpu().numpy(), x_ref)
    assert np.array_equal(ds.tables.cpu().numpy(), tables_np)
    y = torch.cat([r.y for r in results], dim=1)
    lg = torch.cat([r.logits for r in results], dim=2).cpu().numpy()
    assert torch.equal(torch.cat([r.boxes_px for r in results], dim=1), postprocess_and_iou(y)[0])
    y = y.cpu().numpy()
    y_ref, lg_ref = oo.opnet_forward(x_ref, params, np.float64)
    err_y, err_lg = np.abs(y - y_ref).max(), np.abs(lg - lg_ref).max()
    print(f"detector backlog {BACKLOG} persistent + {TICKS} chain ticks: max|dy|={err_y:.3e} max|dlogits|={err_lg:.3e}")
    assert err_y < TOL_Y and err_lg < TOL_LOGITS
    # the backlog alone has the bits of the whole-clip 4-clip forward of the same rows
    with torch.no_grad():
        y_m, lg_m = m(torch.from_numpy(x_ref[:, :BACKLOG]).to(DEV))
    torch.cuda.synchronize()
    assert m.verify_launches() == 0
    _same_bits(y[:, :BACKLOG], y_m.cpu().numpy())
    _same_bits(lg[:, :, :BACKLOG], lg_m.cpu().numpy())


def test_a_replay_derives_the_pixel_boxes_again(monkeypatch):
    """boxes_px is computed from y right behind the step.  If a persistent step gave up, y is rewritten at verify_launches():
    by the replay of that step and of every step behind it.  The pixel boxes the caller holds must follow.  No launch gives
    up here: the log of clean launches is kept and replayed, with boxes_px spoilt first, as an aborted step would leave it."""
    from objectpermanence_amd import DetectorStreams, ModelsFactory
    from objectpermanence_amd.metrics import postprocess_and_iou
    m = ModelsFactory.get_model("opnet", CFG)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.opnet_synth_params(CFG).items()})
    m.eval().to(DEV)
    n = 3
    det = _dev(_clips(n, 40, seed=11)[0])
    backlog, tick = tuple(a[:, :39] for a in det), tuple(a[:, 39:] for a in det)

    chain = DetectorStreams(m, capacity=4)
    ids = chain.open(n)
    ref = [chain.step_detections(ids, *backlog), chain.step_detections(ids, *tick)]

    monkeypatch.setattr(m._monitor, "reap", lambda: 0)      # nothing is reaped: the launches stay unverified, the log is kept
    ds = DetectorStreams(m, capacity=4)
    ids = ds.open(n)
    got = [ds.step_detections(ids, *backlog, engine="persistent"), ds.step_detections(ids, *tick)]
    torch.cuda.synchronize()
    log = ds.pool._log
    assert [e.payload[0] for e in log.entries] == ["step", "call", "step", "call"]
    for r in got:
        assert torch.equal(r.boxes_px, postprocess_and_iou(r.y)[0])
        r.boxes_px.fill_(-1)
    assert log.replay(log.entries[0]) == 4
    torch.cuda.synchronize()
    for r, r_ref in zip(got, ref):                          # everything the caller holds is what a chain-only run gives
        assert torch.equal(r.boxes_px, postprocess_and_iou(r.y)[0])
        _same_bits(r.y.cpu().numpy(), r_ref.y.cpu().numpy())
        _same_bits(r.logits.cpu().numpy(), r_ref.logits.cpu().numpy())
        assert torch.equal(r.boxes_px, r_ref.boxes_px)
    monkeypatch.undo()
    assert ds.verify_launches() == 0 and len(log) == 0
