"""GPU tests of the stateful OPNet streams (objectpermanence_amd/streaming.py, csrc/opnet_stream_kernels.hip): any chunking
of a clip's frames gives the bits of one whole-clip call and of the launch-chain forward of the same clips, within the
fp64 oracle's tolerance, with ragged progress, state round trips, OPNetLstmMlp, weight updates and side streams.
`pytest -m gpu` on the MI355X box."""
import numpy as np
import pytest
import torch

from oracle import opnet_oracle as oo
from oracle import synth

pytestmark = pytest.mark.gpu

REAL_CFG = {"object_to_track_pred_dim": 15, "object_to_track_hidden_dim": 256, "videos_hidden_dim": 512}
TOL_Y = 2e-5          # fp32 through 300 recurrent steps, as tests/test_opnet_gpu.py
TOL_LOGITS = 1e-4
DEV = "cuda:0"
T = 300


def _model(name="opnet"):
    from objectpermanence_amd import ModelsFactory
    m = ModelsFactory.get_model(name, REAL_CFG)
    fn = synth.opnet_synth_params if name == "opnet" else synth.opnet_lstm_mlp_synth_params
    params = fn(REAL_CFG)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    return m.eval().to(DEV), params


def _forward(m, boxes, use_xcd="auto"):
    """model(boxes) -> numpy; use_xcd = "0": the launch chain"""
    if hasattr(m, "use_xcd"):
        m.use_xcd = use_xcd
    with torch.no_grad():
        y, lg = m(torch.from_numpy(boxes).to(DEV))
    torch.cuda.synchronize()
    if hasattr(m, "use_xcd"):
        m.use_xcd = "auto"
    return y.cpu().numpy(), lg.cpu().numpy()


def _stepped(streams, ids, boxes, chunks):
    """run boxes [n, T, 15, 6] through `streams` in frame chunks; the outputs concatenated over time, numpy"""
    assert sum(chunks) == boxes.shape[1]
    xb = torch.from_numpy(boxes).to(DEV)
    ys, lgs, t = [], [], 0
    for k in chunks:
        y, lg = streams.step(ids, xb[:, t:t + k])
        ys.append(y)
        lgs.append(lg)
        t += k
    torch.cuda.synchronize()
    return torch.cat(ys, dim=1).cpu().numpy(), torch.cat(lgs, dim=2).cpu().numpy()


def _run(model, boxes, chunks, capacity=64):
    from objectpermanence_amd import OPNetStreams
    streams = OPNetStreams(model, capacity=capacity)
    ids = streams.open(boxes.shape[0])
    return _stepped(streams, ids, boxes, chunks)


def _same_bits(a, b):
    assert a.shape == b.shape
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"max |diff| {np.abs(a - b).max():.3e}"


CHUNKINGS = {"k1": [1] * T, "k300": [T], "mixed": [1, 7, 64, 3, 225]}


def test_chunk_invariance_and_oracle():
    m, params = _model()
    boxes, _ = synth.make_batch(0, 5, T)
    out = {name: _run(m, boxes, ch) for name, ch in CHUNKINGS.items()}
    y_ref, lg_ref = oo.opnet_forward(boxes, params, np.float64)
    y_def, lg_def = _forward(m, boxes)              # the default engine for 5 clips
    for name, (y, lg) in out.items():
        _same_bits(y, out["k300"][0])
        _same_bits(lg, out["k300"][1])
        assert np.abs(y - y_ref).max() < TOL_Y, name
        assert np.abs(lg - lg_ref).max() < TOL_LOGITS, name
        assert np.abs(y - y_def).max() < 2e-5 and np.abs(lg - lg_def).max() < 5e-5, name
    _same_bits(out["k300"][0], _forward(m, boxes, use_xcd="0")[0])


@pytest.mark.parametrize("n", [1, 32, 33, 70])
def test_one_call_matches_launch_chain(n):
    m, params = _model()
    boxes, _ = synth.make_batch(11, n, T)
    y, lg = _run(m, boxes, [T], capacity=128)
    y_c, lg_c = _forward(m, boxes, use_xcd="0")
    _same_bits(y, y_c)
    _same_bits(lg, lg_c)
    y_ref, lg_ref = oo.opnet_forward(boxes, params, np.float64)
    assert np.abs(y - y_ref).max() < TOL_Y
    assert np.abs(lg - lg_ref).max() < TOL_LOGITS


def test_ragged_progress_in_one_call():
    from objectpermanence_amd import OPNetStreams
    m, _ = _model()
    boxes, _ = synth.make_batch(20, 3, 180)
    p_clip, q_clip, r_clip = boxes[0:1], boxes[1:2, :60], boxes[2:3, :60]
    streams = OPNetStreams(m, capacity=16)
    ids = streams.open(10)
    streams.close([ids[0], ids[2], ids[3], ids[5], ids[8]])
    p = ids[7]
    _stepped(streams, [p], p_clip[:, :120], [120])          # p reaches frame 120 alone
    q, r = ids[4], ids[1]
    # rows that the next call does not name hold arbitrary data, which must survive it bit for bit
    g = torch.Generator(device=DEV).manual_seed(3)
    named = [r, p, q]
    others = [i for i in range(16) if i not in named]
    noise = torch.randn((len(others), streams.state.shape[1]), device=DEV, generator=g)
    streams.state[others] = noise
    before = streams.state.clone()
    # three streams in one call, slots out of order and not contiguous: r and q from frame 0, p from frame 120
    x = np.concatenate([r_clip, p_clip[:, 120:], q_clip], axis=0)
    y, lg = _stepped(streams, [r, p, q], x, [60])
    after = streams.state
    assert torch.equal(after[others].view(torch.int32), before[others].view(torch.int32))
    for clip, row, lo in ((r_clip, 0, 0), (p_clip, 1, 120), (q_clip, 2, 0)):
        y_c, lg_c = _forward(m, clip, use_xcd="0")
        _same_bits(y[row:row + 1], y_c[:, lo:lo + 60])
        _same_bits(lg[row:row + 1], lg_c[:, :, lo:lo + 60])


def test_state_round_trip_and_reopen():
    from objectpermanence_amd import OPNetStreams
    m, params = _model()
    boxes, _ = synth.make_batch(30, 3, T)
    y_all, lg_all = _run(m, boxes, [T])
    a = OPNetStreams(m, capacity=8)
    ids = a.open(3)
    y1, lg1 = _stepped(a, ids, boxes[:, :100], [100])
    h1, c1, h2, c2 = a.get_state(ids)
    assert h1.shape == (1, 3, 256) and c1.shape == (1, 3, 256) and h2.shape == (1, 3, 512) and c2.shape == (1, 3, 512)
    # the state is nn.LSTM's h_n in torch's unit order: the oracle's hidden sequences at frame 99
    _, _, inter = oo.opnet_forward(boxes[:, :100], params, np.float64, return_intermediates=True)
    assert np.abs(h1[0].cpu().numpy() - inter["h1"][:, -1]).max() < TOL_Y
    assert np.abs(h2[0].cpu().numpy() - inter["h2"][:, -1]).max() < TOL_Y
    b = OPNetStreams(m, capacity=8)
    b.open(2)
    ids_b = b.open(3)                                   # other slot ids than in `a`
    b.set_state(ids_b, h1, c1, h2, c2)
    y2, lg2 = _stepped(b, ids_b, boxes[:, 100:], [200])
    _same_bits(np.concatenate([y1, y2], axis=1), y_all)
    _same_bits(np.concatenate([lg1, lg2], axis=2), lg_all)
    # close + open: the same ids come back with a zero state
    b.close(ids_b)
    assert b.open(3) == ids_b
    for s in b.get_state(ids_b):
        assert not s.any()
    y3, lg3 = _stepped(b, ids_b, boxes[:, :50], [50])
    _same_bits(y3, y_all[:, :50])
    _same_bits(lg3, lg_all[:, :, :50])


def test_lstm_mlp_streams():
    from objectpermanence_amd import OPNetStreams
    m, params = _model("opnet_lstm_mlp")
    boxes, _ = synth.make_batch(40, 5, T)
    out = {name: _run(m, boxes, ch) for name, ch in CHUNKINGS.items()}
    y_ref, lg_ref = oo.opnet_lstm_mlp_forward(boxes, params)
    y_m, lg_m = _forward(m, boxes)                  # OPNetLstmMlp.forward always runs the chain
    _same_bits(out["k300"][0], y_m)
    _same_bits(out["k300"][1], lg_m)
    for name, (y, lg) in out.items():
        _same_bits(y, y_m)
        _same_bits(lg, lg_m)
        assert np.abs(y - y_ref).max() < TOL_Y, name
        assert np.abs(lg - lg_ref).max() < TOL_LOGITS, name
    # no video LSTM: get_state has no h2 / c2 and the pool's h2 / c2 columns are left as they were
    streams = OPNetStreams(m, capacity=4)
    ids = streams.open(2)
    streams.state[:, 512:] = 7.0
    _stepped(streams, ids, boxes[:2, :10], [10])
    assert bool((streams.state[:, 512:] == 7.0).all())
    h1, c1, h2, c2 = streams.get_state(ids)
    assert h2 is None and c2 is None and h1.shape == (1, 2, 256) and h1.abs().sum() > 0


def test_weight_update_and_side_stream():
    from objectpermanence_amd import OPNetStreams
    m, _ = _model()
    boxes, _ = synth.make_batch(50, 4, 200)
    streams = OPNetStreams(m, capacity=8)
    ongoing = streams.open(4)
    _stepped(streams, ongoing, boxes[:, :100], [100])
    y_old_full, _ = _forward(m, boxes, use_xcd="0")
    with torch.no_grad():
        m.prediction_layer.weight.mul_(1.25)
        m.object_to_track_LSTM.weight_hh_l0.add_(1e-3)
    y_next, _ = _stepped(streams, ongoing, boxes[:, 100:], [100])
    assert not np.array_equal(y_next, y_old_full[:, 100:])        # the update took effect on the next call
    fresh = streams.open(4)
    y_new, lg_new = _stepped(streams, fresh, boxes, [200])
    y_c, lg_c = _forward(m, boxes, use_xcd="0")
    _same_bits(y_new, y_c)
    _same_bits(lg_new, lg_c)
    # the same call issued on a side stream gives the same bits
    streams.close(fresh)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ids = streams.open(4)
        y_s, lg_s = streams.step(ids, torch.from_numpy(boxes).to(DEV))
    side.synchronize()
    _same_bits(y_s.cpu().numpy(), y_c)
    _same_bits(lg_s.cpu().numpy(), lg_c)


def test_step_refuses_bad_input():
    from objectpermanence_amd import OPNetStreams
    m, _ = _model()
    streams = OPNetStreams(m, capacity=2)
    ids = streams.open(2)
    with pytest.raises(RuntimeError, match="ROCm"):
        streams.step(ids, torch.zeros(2, 1, 15, 6))
    with pytest.raises(ValueError, match=r"\[n=2"):
        streams.step(ids, torch.zeros(2, 1, 15, 5, device=DEV))
    with pytest.raises(ValueError, match="boxes must be"):
        streams.step(ids[:1], torch.zeros(2, 1, 15, 6, device=DEV))
    with pytest.raises(RuntimeError, match="full"):
        streams.open(1)
    with pytest.raises(ValueError, match="distinct"):
        streams.step([0, 0], torch.zeros(2, 1, 15, 6, device=DEV))
