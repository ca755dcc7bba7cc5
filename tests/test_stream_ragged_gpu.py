"""GPU tests of the ragged stream steps (streaming.py step(..., lengths), opnet_stream_step_ragged_f32,
opseq_stream_step_ragged_f32): valid outputs have the bits of the launch chain over the same n clips, padding outputs are
+0.0, each pool row ends where uniform calls chunked at the lengths leave it, a zero length and an unnamed row keep their
bits, lengths = K is the uniform call, and device lengths run without a host sync.  NaN padding never leaks.  The sizes
cover every step form: one row block, two, and the wide kernel from three.  `pytest -m gpu` on the MI355X box."""
import numpy as np
import pytest
import torch

from oracle import opnet_oracle as oo
from oracle import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = 9
OPNET_CFG = {"object_to_track_pred_dim": 15, "object_to_track_hidden_dim": 256, "videos_hidden_dim": 512}
CFG = {"opnet": OPNET_CFG, "opnet_lstm_mlp": OPNET_CFG, "baseline_lstm": {"videos_hidden_dim": 512},
       "non_linear_lstm": {"boxes_features_dim": 256, "videos_hidden_dim": 512}}
PARAMS = {"opnet": synth.opnet_synth_params, "opnet_lstm_mlp": synth.opnet_lstm_mlp_synth_params,
          "baseline_lstm": synth.baseline_lstm_synth_params, "non_linear_lstm": synth.non_linear_lstm_synth_params}
OPNET_MODELS = ("opnet", "opnet_lstm_mlp")
TOL = {"opnet": (2e-5, 1e-4), "opnet_lstm_mlp": (2e-5, 1e-4), "baseline_lstm": (3e-5, None), "non_linear_lstm": (3e-5, None)}
_MODELS = {}


def _model(name):
    if name not in _MODELS:
        from objectpermanence_amd import ModelsFactory
        m = ModelsFactory.get_model(name, CFG[name])
        params = PARAMS[name](CFG[name])
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
        _MODELS[name] = (m.eval().to(DEV), params)
    return _MODELS[name]


def _pool(name, capacity):
    from objectpermanence_amd import LstmStackStreams, OPNetStreams
    m = _model(name)[0]
    return OPNetStreams(m, capacity) if name in OPNET_MODELS else LstmStackStreams(m, capacity)


def _inputs(name, seed, n, k):
    boxes = synth.make_batch(seed, n, k)[0]
    return boxes if name in OPNET_MODELS else synth.boxes5(boxes)


def _step(pool, ids, x, lengths=None):
    """one call -> numpy (y, logits or None)"""
    out = pool.step(ids, torch.from_numpy(np.ascontiguousarray(x)).to(DEV), lengths) if lengths is not None else \
        pool.step(ids, torch.from_numpy(np.ascontiguousarray(x)).to(DEV))
    y, lg = out if isinstance(out, tuple) else (out, None)
    torch.cuda.synchronize()
    return y.cpu().numpy(), None if lg is None else lg.cpu().numpy()


def _chain(name, x):
    """the whole-clip launch-chain forward of the same n clips -> numpy (y, logits or None)"""
    m = _model(name)[0]
    saved = {a: getattr(m, a) for a in ("use_xcd", "use_xcd4") if hasattr(m, a)}
    runner = getattr(m, "_runner", None)
    if not hasattr(runner, "use_xcd"):
        runner = None
    if runner is not None:
        saved_r = runner.use_xcd
        runner.use_xcd = "0"
    for a in saved:
        setattr(m, a, "0")
    try:
        with torch.no_grad():
            out = m(torch.from_numpy(x).to(DEV))
        torch.cuda.synchronize()
    finally:
        for a, v in saved.items():
            setattr(m, a, v)
        if runner is not None:
            runner.use_xcd = saved_r
    y, lg = out if isinstance(out, tuple) else (out, None)
    return y.cpu().numpy(), None if lg is None else lg.cpu().numpy()


def _oracle(name, x):
    p = {k: v.astype(np.float64) for k, v in _model(name)[1].items()}
    if name == "opnet":
        return oo.opnet_forward(x, _model(name)[1], np.float64)
    if name == "opnet_lstm_mlp":
        return None
    h = x.astype(np.float64)
    B, t = h.shape[:2]
    if name == "non_linear_lstm":
        h = np.maximum(h @ p["boxes_linear.weight"].T, 0.0)
    h = h.reshape(B, t, -1)
    for l in range(1 if name == "baseline_lstm" else 2):
        h = oo.lstm_seq(h, p[f"video_LSTM.weight_ih_l{l}"], p[f"video_LSTM.weight_hh_l{l}"], None, None,
                        return_state=True)[0]
    return h @ p["predictions_layer.weight"].T, None


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b, what=""):
    assert a.shape == b.shape, what
    assert np.array_equal(_bits(a), _bits(b)), f"{what}: max |diff| {np.nanmax(np.abs(a - b)):.3e}"


def _rows(pool, ids):
    with torch.cuda.device(pool.device):
        r = pool.state.index_select(0, torch.tensor(list(ids), device=pool.device)).cpu().numpy()
    return r


def _lengths(n, seed):
    """0, 1, K and repeats among random lengths"""
    base = [0, 1, K, K, 3, 1]
    rng = np.random.default_rng(seed)
    if n == 1:
        return np.array([4], np.int32)
    return np.array([base[i] if i < len(base) else rng.integers(0, K + 1) for i in range(n)], np.int32)[rng.permutation(n)]


def _padded(x, lengths):
    xp = x.copy()
    for i, L in enumerate(lengths):
        xp[i, L:] = np.nan
    return xp


CASES = [("opnet", 1), ("opnet", 5), ("opnet", 33), ("opnet", 70), ("opnet_lstm_mlp", 70),
         ("baseline_lstm", 1), ("baseline_lstm", 24), ("baseline_lstm", 33), ("baseline_lstm", 70),
         ("non_linear_lstm", 1), ("non_linear_lstm", 24), ("non_linear_lstm", 33), ("non_linear_lstm", 70)]


@pytest.mark.parametrize("name,n", CASES)
def test_ragged_bits_state_and_padding(name, n):
    lens1, lens2 = _lengths(n, 1), _lengths(n, 2)
    x1, x2 = _inputs(name, 10 + n, n, K), _inputs(name, 20 + n, n, K)
    # pool A: two ragged calls, NaN in every padding frame, with an unnamed open stream beside them
    A = _pool(name, n + 8)
    extra = A.open(3)
    ids = A.open(n)
    with torch.cuda.device(A.device):
        A.state[extra] = torch.randn((3, A.state.shape[1]), device=A.device)
    extra_before = _rows(A, extra)
    y1, lg1 = _step(A, ids, _padded(x1, lens1), lens1)
    state1 = _rows(A, ids)
    y2, lg2 = _step(A, ids, _padded(x2, lens2), lens2)
    state2 = _rows(A, ids)
    _same_bits(_rows(A, extra), extra_before, "unnamed rows")

    # first call from the zero state: valid frames are the launch chain's bits over the same n clips, padding +0.0
    yc, lgc = _chain(name, x1)
    tol_y, tol_l = TOL[name]
    ref = _oracle(name, x1)
    for i, L in enumerate(lens1):
        _same_bits(y1[i, :L], yc[i, :L], f"y stream {i}")
        assert not _bits(y1[i, L:]).any(), "padding y is +0.0"
        if lg1 is not None:
            _same_bits(lg1[i, :, :L], lgc[i, :, :L], f"logits stream {i}")
            assert not _bits(lg1[i, :, L:]).any(), "padding logits are +0.0"
        if ref is not None and L:
            assert np.abs(y1[i, :L] - ref[0][i, :L]).max() < tol_y
            if ref[1] is not None:
                assert np.abs(lg1[i, :, :L] - ref[1][i, :, :L]).max() < tol_l

    # pool B: the same n streams through uniform calls chunked at the distinct lengths; a stream's row is read right after
    # the chunk that ends at its length
    B = _pool(name, n + 8)
    idsB = B.open(n)
    for x, lens, y, lg, want in ((x1, lens1, y1, lg1, state1), (x2, lens2, y2, lg2, state2)):
        start = _rows(B, idsB)
        got = np.where((lens == 0)[:, None], start, np.nan).astype(np.float32)
        t = 0
        for d in sorted(set(int(v) for v in lens if v > 0)):
            yb, lgb = _step(B, idsB, x[:, t:d])
            for i in np.flatnonzero(lens >= d):
                _same_bits(y[i, t:d], yb[i], f"y stream {i} frames {t}:{d}")
                if lg is not None:
                    _same_bits(lg[i, :, t:d], lgb[i], f"logits stream {i} frames {t}:{d}")
            rows = _rows(B, idsB)
            got[lens == d] = rows[lens == d]
            t = d
        _same_bits(want, got, "pool rows")
        with torch.cuda.device(B.device):           # both pools continue from A's states after this call
            B.state[idsB] = torch.from_numpy(want).to(B.device)
        zero = lens == 0
        if zero.any():
            _same_bits(want[zero], start[zero], "len 0 rows")


@pytest.mark.parametrize("name,n", [("opnet", 33), ("opnet", 70), ("baseline_lstm", 33), ("non_linear_lstm", 24)])
def test_full_lengths_are_the_uniform_call(name, n):
    x = _inputs(name, 5, n, K)
    U, R = _pool(name, n), _pool(name, n)
    iu, ir = U.open(n), R.open(n)
    for _ in range(2):
        yu, lgu = _step(U, iu, x)
        yr, lgr = _step(R, ir, x, [K] * n)
        _same_bits(yr, yu, "y")
        if lgu is not None:
            _same_bits(lgr, lgu, "logits")
        _same_bits(_rows(R, ir), _rows(U, iu), "state")


@pytest.mark.parametrize("name", ["opnet", "non_linear_lstm"])
def test_device_lengths_no_sync_and_side_stream(name):
    n = 40
    lens = _lengths(n, 7)
    x = _padded(_inputs(name, 8, n, K), lens)
    H = _pool(name, n)
    ih = H.open(n)
    yh, lgh = _step(H, ih, x, lens)
    D = _pool(name, n)
    idd = D.open(n)
    xd = torch.from_numpy(x).to(DEV)
    ld = torch.from_numpy(lens).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = D.step(idd, xd, ld)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    y, lg = out if isinstance(out, tuple) else (out, None)
    torch.cuda.synchronize()
    _same_bits(y.cpu().numpy(), yh, "y")
    if lg is not None:
        _same_bits(lg.cpu().numpy(), lgh, "logits")
    _same_bits(_rows(D, idd), _rows(H, ih), "state")
    # on a side stream
    S = _pool(name, n)
    isd = S.open(n)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        out = S.step(isd, xd, ld)
    side.synchronize()
    y, lg = out if isinstance(out, tuple) else (out, None)
    _same_bits(y.cpu().numpy(), yh, "y side stream")
    _same_bits(_rows(S, isd), _rows(H, ih), "state side stream")


def test_out_of_range_device_lengths_are_clamped():
    n = 6
    x = _inputs("opnet", 9, n, K)
    lens = np.array([-5, 0, 3, K, K + 7, 1 << 30], np.int32)
    clamped = np.clip(lens, 0, K).astype(np.int32)
    A, B = _pool("opnet", n), _pool("opnet", n)
    ia, ib = A.open(n), B.open(n)
    out = A.step(ia, torch.from_numpy(x).to(DEV), torch.from_numpy(lens).to(DEV))
    torch.cuda.synchronize()
    yb, lgb = _step(B, ib, x, clamped)
    _same_bits(out[0].cpu().numpy(), yb)
    _same_bits(out[1].cpu().numpy(), lgb)
    _same_bits(_rows(A, ia), _rows(B, ib))


def test_bad_lengths_are_refused_before_launch():
    n = 3
    P = _pool("baseline_lstm", 4)
    ids = P.open(n)
    x = torch.zeros((n, K, 15, 5), device=DEV)
    for bad, exc in (([1, 2], ValueError), ([1, 2, K + 1], ValueError), ([1.5, 2, 3], TypeError)):
        with pytest.raises(exc):
            P.step(ids, x, bad)
    with pytest.raises(ValueError, match="int32"):
        P.step(ids, x, torch.ones(n, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="int32"):
        P.step(ids, x, torch.ones(n + 1, dtype=torch.int32, device=DEV))
    assert not _rows(P, ids).any()
