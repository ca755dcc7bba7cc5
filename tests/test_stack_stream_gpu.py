"""GPU tests of the stateful stacked-LSTM streams (objectpermanence_amd/streaming.py LstmStackStreams,
csrc/seq_stream_kernels.hip) for BaselineLstm and NonLinearLstm: any chunking of a clip's frames gives the bits of one
whole-clip call and of the launch-chain forward of the same clips, within the fp64 oracle's tolerance, with ragged
progress, arbitrary initial states, state round trips, weight updates and side streams.  `pytest -m gpu` on the MI355X box."""
import numpy as np
import pytest
import torch

from oracle import opnet_oracle as oo
from oracle import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T = 300
TOL = 3e-5            # as tests/test_siblings_gpu.py
REAL = {"baseline_lstm": {"videos_hidden_dim": 512},
        "non_linear_lstm": {"boxes_features_dim": 256, "videos_hidden_dim": 512}}
PARAMS = {"baseline_lstm": synth.baseline_lstm_synth_params, "non_linear_lstm": synth.non_linear_lstm_synth_params}
LAYERS = {"baseline_lstm": 1, "non_linear_lstm": 2}
NAMES = ["baseline_lstm", "non_linear_lstm"]


def _model(name, cfg=None):
    from objectpermanence_amd import ModelsFactory
    cfg = REAL[name] if cfg is None else cfg
    m = ModelsFactory.get_model(name, cfg)
    params = PARAMS[name](cfg)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    return m.eval().to(DEV), params


def _x(seed, n, t):
    return synth.boxes5(synth.make_batch(seed, n, t)[0])


def _chain(m, x):
    """the whole-clip launch-chain forward of x [n, T, 15, 5] -> numpy"""
    m._runner.use_xcd = "0"
    try:
        with torch.no_grad():
            y = m(torch.from_numpy(x).to(DEV))
        torch.cuda.synchronize()
    finally:
        m._runner.use_xcd = "auto"
    return y.cpu().numpy()


def _oracle(name, x, p, h0=None, c0=None):
    """fp64: y [n, T, 4] and the final (h_n, c_n) [L, n, H], from (h0, c0) [L, n, H] (None: zero)"""
    B, t = x.shape[:2]
    P = {k: v.astype(np.float64) for k, v in p.items()}
    x = x.astype(np.float64)
    if name == "non_linear_lstm":
        x = np.maximum(x @ P["boxes_linear.weight"].T, 0.0)
    h = x.reshape(B, t, -1)
    hs, cs = [], []
    for l in range(LAYERS[name]):
        h, (hn, cn) = oo.lstm_seq(h, P[f"video_LSTM.weight_ih_l{l}"], P[f"video_LSTM.weight_hh_l{l}"],
                                  None if h0 is None else h0[l], None if c0 is None else c0[l], return_state=True)
        hs.append(hn)
        cs.append(cn)
    return h @ P["predictions_layer.weight"].T, np.stack(hs), np.stack(cs)


def _streams(m, capacity=128):
    from objectpermanence_amd import LstmStackStreams
    return LstmStackStreams(m, capacity=capacity)


def _stepped(streams, ids, x, chunks):
    """run x [n, T, 15, 5] through `streams` in frame chunks; y concatenated over time, numpy"""
    assert sum(chunks) == x.shape[1]
    xb = torch.from_numpy(x).to(DEV)
    ys, t = [], 0
    for k in chunks:
        ys.append(streams.step(ids, xb[:, t:t + k]))
        t += k
    torch.cuda.synchronize()
    return torch.cat(ys, dim=1).cpu().numpy()


def _state(streams, ids):
    h, c = streams.get_state(ids)
    torch.cuda.synchronize()
    return h.cpu().numpy(), c.cpu().numpy()


def _same_bits(a, b):
    assert a.shape == b.shape
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"max |diff| {np.abs(a - b).max():.3e}"


CHUNKINGS = {"k1": [1] * T, "k300": [T], "mixed": [1, 7, 64, 3, 225]}


@pytest.mark.parametrize("name", NAMES)
def test_chunk_invariance_chain_and_oracle(name):
    m, p = _model(name)
    x = _x(0, 5, T)
    y_ref, h_ref, c_ref = _oracle(name, x, p)
    y_chain = _chain(m, x)
    assert np.abs(y_chain - y_ref).max() < TOL
    first = None
    for cname, ch in CHUNKINGS.items():
        s = _streams(m)
        ids = s.open(5)
        y = _stepped(s, ids, x, ch)
        h, c = _state(s, ids)
        _same_bits(y, y_chain)
        assert np.abs(y - y_ref).max() < TOL, cname
        # get_state after 300 frames: the oracle's final (h, c) of every layer
        assert h.shape == c.shape == (LAYERS[name], 5, 512)
        assert np.abs(h - h_ref).max() < TOL, cname
        assert np.abs(c - c_ref).max() < TOL, cname
        if first is None:
            first = (h, c)
        else:
            _same_bits(h, first[0])
            _same_bits(c, first[1])


BATCHES = [("baseline_lstm", n) for n in (1, 5, 32, 33, 70)] + [("non_linear_lstm", n) for n in (1, 5, 24, 32, 33, 70)]


@pytest.mark.parametrize("name,n", BATCHES)
def test_batch_sizes_match_chain(name, n):
    """one-frame calls (NonLinearLstm: the skinny input product, 16 * ceil(n / 16) rows) and one 280-frame call (the tiled
    GEMM: 280 * 16 rows and more) against the whole-clip chain; at n = 24 the chain's GEMM takes 64-wide tiles (M = 7 200)"""
    m, p = _model(name)
    x = _x(n, n, T)
    s = _streams(m)
    ids = s.open(n)
    y = _stepped(s, ids, x, [1] * 20 + [T - 20])
    _same_bits(y, _chain(m, x))
    if n in (1, 33):
        assert np.abs(y - _oracle(name, x, p)[0]).max() < TOL


@pytest.mark.parametrize("n,k", [(1, 1), (1, 300), (5, 64), (32, 1), (33, 8), (70, 2)])
def test_input_product_routes_give_the_same_bits(n, k):
    """the hoisted layer-0 input product alone (opseq_stream_input_product_f32): the skinny kernel and the tiled GEMM give the
    same xg bits, within fp32 rounding of the fp64 product, zero for the clips past n"""
    from objectpermanence_amd import _lib
    m, p = _model("non_linear_lstm")
    lib = _lib.load()
    L, KX, H = 2, 3840, 512
    RB = (n + 31) // 32
    feats = torch.from_numpy(_x(40 + n, n, k)).to(DEV)
    with torch.no_grad():
        x = torch.relu(feats @ m.boxes_linear.weight.t()).reshape(n, k, KX).contiguous()
    r = m._runner
    wl = [m.video_LSTM.weight_ih_l0, m.video_LSTM.weight_ih_l1, m.video_LSTM.weight_hh_l0, m.video_LSTM.weight_hh_l1,
          m.predictions_layer.weight]
    stream = torch.cuda.current_stream().cuda_stream
    packed = r._packed_weights(wl, torch.device(DEV), stream)
    ws = torch.empty(lib.opseq_stream_workspace_bytes(n, k, L, KX, H), dtype=torch.uint8, device=DEV)
    out = {}
    for route in (0, 1, 2):
        xg = torch.full((k, RB, H, 32, 4), float("nan"), device=DEV)
        _lib.check(lib.opseq_stream_input_product_f32(x.data_ptr(), packed.data_ptr(), xg.data_ptr(), ws.data_ptr(), ws.numel(),
                                                      n, k, L, KX, H, route, stream), "opseq_stream_input_product_f32")
        torch.cuda.synchronize()
        out[route] = xg.cpu().numpy()
    _same_bits(out[1], out[2])
    _same_bits(out[0], out[1])
    g = x.double().cpu().numpy().reshape(n * k, KX) @ p["video_LSTM.weight_ih_l0"].astype(np.float64).T     # [n k][4H]
    ref = g.reshape(n, k, 4, H).transpose(1, 0, 3, 2)                                                      # [k][n][H][gate]
    got = out[1].transpose(0, 1, 3, 2, 4).reshape(k, RB * 32, H, 4)
    assert np.abs(got[:, :n] - ref).max() < 1e-3 * max(1.0, np.abs(ref).max())
    assert not got[:, n:].any()


@pytest.mark.parametrize("k", [1, 8, 300])
def test_skinny_product_gives_the_tiled_bits(monkeypatch, k):
    m, _ = _model("non_linear_lstm")
    x = _x(3, 32, k)
    out = {}
    for rows in ("0", None, "1000000"):          # always tiled, the default routing, always skinny
        if rows is None:
            monkeypatch.delenv("OPSEQ_STREAM_SKINNY_MAX_ROWS", raising=False)
        else:
            monkeypatch.setenv("OPSEQ_STREAM_SKINNY_MAX_ROWS", rows)
        s = _streams(m)
        ids = s.open(32)
        y = _stepped(s, ids, x, [k])
        out[rows] = (y,) + _state(s, ids)
    for key in ("0", "1000000"):
        for a, b in zip(out[key], out[None]):
            _same_bits(a, b)


@pytest.mark.parametrize("name", NAMES)
def test_ragged_progress_matches_solo_runs(name):
    """streams at different frame offsets, named out of order in one call: each equals its own solo run"""
    m, _ = _model(name)
    offsets = [3, 0, 10, 1]
    k = 5
    xs = [_x(20 + i, 1, off + k) for i, off in enumerate(offsets)]
    solo = []
    for xi, off in zip(xs, offsets):
        s = _streams(m, capacity=4)
        ids = s.open(1)
        solo.append(_stepped(s, ids, xi, [off, k] if off else [k]))
    s = _streams(m, capacity=8)
    ids = s.open(4)
    for i, off in enumerate(offsets):
        if off:
            s.step([ids[i]], torch.from_numpy(xs[i][:, :off]).to(DEV))
    order = [3, 0, 2, 1]
    joint = torch.cat([torch.from_numpy(xs[i][:, offsets[i]:]) for i in order]).to(DEV)
    y = s.step([ids[i] for i in order], joint).cpu().numpy()
    for row, i in enumerate(order):
        _same_bits(y[row:row + 1], solo[i][:, offsets[i]:])


@pytest.mark.parametrize("name", NAMES)
def test_unnamed_rows_keep_their_bits(name):
    m, _ = _model(name)
    s = _streams(m, capacity=16)
    ids = s.open(6)
    x = torch.from_numpy(_x(5, 6, 4)).to(DEV)
    s.step(ids, x)
    before = s.state.clone()
    named = [ids[4], ids[1], ids[2]]
    s.step(named, x[:3, :2].contiguous())
    torch.cuda.synchronize()
    after = s.state
    for i in (0, 3, 5):
        assert torch.equal(before[ids[i]].view(torch.int32), after[ids[i]].view(torch.int32))
    for i in (1, 2, 4):
        assert not torch.equal(before[ids[i]], after[ids[i]])
    for i in range(6, 16):          # rows never opened stay zero
        assert not after[i].any()


@pytest.mark.parametrize("name", NAMES)
def test_set_state_matches_the_oracle(name):
    """streams started from an arbitrary (h, c): a unit-order or layout slip in the gather shows here"""
    m, p = _model(name)
    n, L = 6, LAYERS[name]
    rng = np.random.default_rng(11)
    h0 = np.tanh(rng.standard_normal((L, n, 512))).astype(np.float32)
    c0 = (1.5 * rng.standard_normal((L, n, 512))).astype(np.float32)
    x = _x(8, n, 20)
    s = _streams(m)
    ids = s.open(n)
    s.set_state(ids, torch.from_numpy(h0), torch.from_numpy(c0))
    h_back, c_back = _state(s, ids)
    _same_bits(h_back, h0)
    _same_bits(c_back, c0)
    y = _stepped(s, ids, x, [1, 19])
    h, c = _state(s, ids)
    y_ref, h_ref, c_ref = _oracle(name, x, p, h0, c0)
    assert np.abs(y - y_ref).max() < TOL
    assert np.abs(h - h_ref).max() < TOL
    assert np.abs(c - c_ref).max() < TOL


@pytest.mark.parametrize("name", NAMES)
def test_state_round_trip_is_uninterrupted(name):
    m, _ = _model(name)
    x = _x(9, 3, 24)
    s = _streams(m, capacity=8)
    ids = s.open(3)
    y_whole = _stepped(s, ids, x, [24])
    s2 = _streams(m, capacity=8)
    ids2 = s2.open(3)
    y_a = _stepped(s2, ids2, x[:, :10], [10])
    h, c = s2.get_state(ids2)
    s2.close(ids2)
    s2.open(2)                                     # the old rows are taken by others ...
    ids3 = s2.open(3)                              # ... and reopened at a zero state elsewhere
    assert ids3 != ids2
    s2.set_state(ids3, h, c)
    y_b = _stepped(s2, ids3, x[:, 10:], [14])
    _same_bits(np.concatenate([y_a, y_b], axis=1), y_whole)


@pytest.mark.parametrize("name", NAMES)
def test_in_place_weight_update_takes_effect(name):
    m, _ = _model(name)
    x = _x(12, 4, 6)
    s = _streams(m, capacity=8)
    ids = s.open(4)
    _stepped(s, ids, x, [6])
    with torch.no_grad():
        m.video_LSTM.weight_hh_l0.mul_(0.5)
        m.predictions_layer.weight.add_(0.01)
    ids2 = s.open(4)
    y = _stepped(s, ids2, x, [2, 4])
    _same_bits(y, _chain(m, x))


@pytest.mark.parametrize("name", NAMES)
def test_side_stream(name):
    m, _ = _model(name)
    x = _x(13, 7, 9)
    s = _streams(m)
    ids = s.open(7)
    y_default = _stepped(s, ids, x, [1, 8])
    side = torch.cuda.Stream()
    s2 = _streams(m)
    ids2 = s2.open(7)
    with torch.cuda.stream(side):
        xb = torch.from_numpy(x).to(DEV)
        ys = [s2.step(ids2, xb[:, :1]), s2.step(ids2, xb[:, 1:])]
        y_side = torch.cat(ys, dim=1)
    side.synchronize()
    _same_bits(y_side.cpu().numpy(), y_default)


def test_refusals():
    m, _ = _model("non_linear_lstm")
    s = _streams(m, capacity=4)
    ids = s.open(2)
    x = torch.from_numpy(_x(1, 2, 3)).to(DEV)
    with pytest.raises(ValueError, match="15, 5"):
        s.step(ids, torch.zeros((2, 3, 15, 6), device=DEV))
    with pytest.raises(ValueError):
        s.step(ids, x[:1])
    with pytest.raises(ValueError, match="distinct"):
        s.step([ids[0], ids[0]], x)
    with pytest.raises(KeyError, match="not open"):
        s.step([ids[0], 3], x)
    with pytest.raises(RuntimeError, match="ROCm device"):
        s.step(ids, x.cpu())
    with pytest.raises(ValueError, match=r"\[2, 2, 512\]"):
        s.set_state(ids, torch.zeros(1, 2, 512), torch.zeros(1, 2, 512))
    s.close([ids[1]])
    with pytest.raises(KeyError, match="not open"):
        s.step(ids, x)
    assert s.free == 3


@pytest.mark.parametrize("name,cfg", [("non_linear_lstm", {"boxes_features_dim": 32, "videos_hidden_dim": 64}),
                                      ("baseline_lstm", {"videos_hidden_dim": 1024})])
def test_small_and_wide_shapes(name, cfg):
    """NonLinearLstm F = 32 / H = 64 still hoists its input (KX = 480); BaselineLstm H = 1024 streams weight fragments"""
    m, p = _model(name, cfg)
    n = 3
    x = _x(30, n, 40)
    s = _streams(m)
    ids = s.open(n)
    y = _stepped(s, ids, x, [1, 1, 13, 25])
    h, c = _state(s, ids)
    y_ref, h_ref, c_ref = _oracle(name, x, p)
    assert np.abs(y - y_ref).max() < TOL
    assert np.abs(h - h_ref).max() < TOL
    assert np.abs(c - c_ref).max() < TOL
    _same_bits(y, _chain(m, x))
