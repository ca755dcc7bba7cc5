"""GPU tests of the persistent engine of the stacked-LSTM streams (objectpermanence_amd/streaming.py LstmStackStreams
engine="persistent", csrc/seq_stream_x_kernels.hip, seqx_forward<.., false, true>): a stream step of BaselineLstm /
NonLinearLstm as ONE persistent launch of the 4-clip form that reads each stream's state from the pool and writes it back.

What is pinned: (1) a whole clip in one step from the zero state has the bits of the existing whole-clip 4-clip forward
(_run_xcd); (2) any chunking of the frames into persistent steps gives the same bits, outputs and pool rows; (3) a stream's
bits do not depend on the call's other streams or its position; (4) a stream handed from one engine to the other, or started
from a random state, stays within the project's fp64 bound for these models (the test prints the maxima; DESIGN.md 12f has
them); (5) rows a call does not name keep their bits, states round-trip, a sentinel-patterned NaN is a plain NaN; (6) the chain
engine is what it was; (7) a replay of logged calls equals a chain-only pool; (8) DetectorStreams reaches the engine per call
and nothing synchronises the host.  No test forces a launch to give up.  `pytest -m gpu` on the MI355X box."""
import numpy as np
import pytest
import torch

from oracle import opnet_oracle as oo
from oracle import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T = 300
TOL = 3e-5            # the project's bound for these models (tests/test_siblings_gpu.py, tests/test_stack_stream_gpu.py)
REAL = {"baseline_lstm": {"videos_hidden_dim": 512},
        "non_linear_lstm": {"boxes_features_dim": 256, "videos_hidden_dim": 512}}
PARAMS = {"baseline_lstm": synth.baseline_lstm_synth_params, "non_linear_lstm": synth.non_linear_lstm_synth_params}
LAYERS = {"baseline_lstm": 1, "non_linear_lstm": 2}
NAMES = ["baseline_lstm", "non_linear_lstm"]
_CACHE = {}


def _fresh_model(name):
    from objectpermanence_amd import ModelsFactory
    m = ModelsFactory.get_model(name, REAL[name])
    params = PARAMS[name](REAL[name])
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    return m.eval().to(DEV), params


def _model(name):
    if name not in _CACHE:
        _CACHE[name] = _fresh_model(name)
    return _CACHE[name]


def _x(seed, n, t):
    return synth.boxes5(synth.make_batch(seed, n, t)[0])


def _whole_clip_x(m, x):
    """the model's whole-clip forward of x [n, T, 15, 5] on route "x", the 4-clip persistent launch (_run_xcd), forced as
    tests/test_inference_routes_oracle_gpu.py forces it: the 16-clip form off, the route and the launch count asserted"""
    r = m._runner
    n, t = x.shape[:2]
    cap = int(_lib().opseq_xcd_max_batch(r.L))
    r.use_xcdt = "0"
    try:
        assert r.engine(min(n, cap), t) == "x"
        before = (r.xcd_launches, r.xcdt_launches)
        with torch.no_grad():
            y = m(torch.from_numpy(x).to(DEV)) if n <= cap else _forced_x(m, x)
        torch.cuda.synchronize()
        assert r._monitor.verify() == 0 and r._monitor.aborted == 0
        assert (r.xcd_launches - before[0], r.xcdt_launches - before[1]) == ((n + cap - 1) // cap, 0)
    finally:
        r.use_xcdt = "auto"
    return y.cpu().numpy()


def _forced_x(m, x):
    """more clips than one 4-clip launch carries: the runner's route "x" over whole launches (its merged-pass form)"""
    xt = torch.from_numpy(x).to(DEV)
    lib = _lib()
    with torch.cuda.device(DEV):
        if type(m).__name__ == "NonLinearLstm":
            n, t = x.shape[:2]
            feats = torch.empty((n, t, 15 * m._f), dtype=torch.float32, device=DEV)
            rc = lib.opseq_slot_embed_relu_f32(xt.data_ptr(), m.boxes_linear.weight.data_ptr(), feats.data_ptr(), n * t, 15, m._f,
                                               torch.cuda.current_stream().cuda_stream)
            assert rc == 0
        else:
            feats = xt.view(x.shape[0], x.shape[1], -1)
        return m._runner.run(feats, m.video_LSTM, m.predictions_layer, engine="x")


def _lib():
    from objectpermanence_amd import _lib as L
    return L.load()


def _chain(m, x):
    """the whole-clip launch-chain forward of x -> numpy"""
    m._runner.use_xcd = "0"
    try:
        with torch.no_grad():
            y = m(torch.from_numpy(x).to(DEV))
        torch.cuda.synchronize()
    finally:
        m._runner.use_xcd = "auto"
    return y.cpu().numpy()


def _oracle(name, x, p, h0=None, c0=None):
    """fp64, as tests/test_stack_stream_gpu.py::_oracle: y [n, T, 4] and the final (h_n, c_n) [L, n, H], from (h0, c0)
    [L, n, H] (None: zero)"""
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


def _rows_of(h, c):
    """(h_n, c_n) [L, n, H] -> pool rows [n, 2 L H] = [h_0 | c_0 | h_1 | c_1]"""
    return np.stack([h, c], axis=1).transpose(2, 0, 1, 3).reshape(h.shape[1], -1)


def _pool(m, capacity=384, engine="persistent"):
    from objectpermanence_amd import LstmStackStreams
    return LstmStackStreams(m, capacity=capacity, engine=engine)


def _stepped(streams, ids, x, chunks, engine=None, engines=None):
    """x [n, T, 15, 5] through `streams` in frame chunks (engines: one engine per chunk) -> numpy y"""
    assert sum(chunks) == x.shape[1]
    xb = torch.from_numpy(x).to(DEV)
    ys, t = [], 0
    for i, k in enumerate(chunks):
        ys.append(streams.step(ids, xb[:, t:t + k], engine=engines[i] if engines else engine))
        t += k
    torch.cuda.synchronize()
    assert streams.verify_launches() == 0
    return torch.cat(ys, dim=1).cpu().numpy()


def _same_bits(a, b):
    assert a.shape == b.shape
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"max |diff| {np.nanmax(np.abs(a - b)):.3e}"


def _rows(streams, ids):
    torch.cuda.synchronize()
    return streams.state[torch.tensor(ids, device=DEV)].cpu().numpy()


def _count_watches(monkeypatch, m):
    """the persistent launches the runner's monitor is asked to watch from here on"""
    seen = []
    watch = m._runner._monitor.watch

    def counting(ws, off, redo, what):
        seen.append(what)
        return watch(ws, off, redo, what)
    monkeypatch.setattr(m._runner._monitor, "watch", counting)
    return seen


# ---- 1. whole clip ----------------------------------------------------------------------------------------------------
WHOLE = [(name, n) for name in NAMES for n in (1, 5, 32, 33, 64, 70, 128)] + [("baseline_lstm", 200)]


@pytest.mark.parametrize("name,n", WHOLE)
def test_whole_clip_has_the_bits_of_the_4clip_forward(name, n, monkeypatch):
    m, _ = _model(name)
    x = _x(11, n, T)
    y_m = _whole_clip_x(m, x)
    streams = _pool(m)
    assert streams.engine == "persistent"
    seen = _count_watches(monkeypatch, m)
    y = _stepped(streams, streams.open(n), x, [T])
    nmax = int(_lib().opseq_stream_x_max_streams(LAYERS[name]))
    assert seen == ["opseq_stream_step_x"] * ((n + nmax - 1) // nmax)
    _same_bits(y, y_m)


@pytest.mark.parametrize("name,n", [("baseline_lstm", 300), ("non_linear_lstm", 150)])
def test_more_than_max_streams_run_as_two_launches(name, n, monkeypatch):
    m, _ = _model(name)
    nmax = int(_lib().opseq_stream_x_max_streams(LAYERS[name]))
    assert nmax < n <= 2 * nmax
    x = _x(5, n, 24)
    streams = _pool(m)
    ids = streams.open(n)
    seen = _count_watches(monkeypatch, m)
    y = _stepped(streams, ids, x, [24])
    assert seen == ["opseq_stream_step_x"] * 2
    two = _pool(m)
    ids2 = two.open(n)
    ya = _stepped(two, ids2[:nmax], x[:nmax], [24])
    yb = _stepped(two, ids2[nmax:], x[nmax:], [24])
    _same_bits(y, np.concatenate([ya, yb]))
    _same_bits(_rows(streams, ids), _rows(two, ids2))
    _same_bits(y, _whole_clip_x(m, x))            # and of the whole-clip route over whole launches


# ---- 2. chunk invariance ----------------------------------------------------------------------------------------------
CHUNKINGS = {"k300": [T], "1-299": [1, 299], "150-150": [150, 150], "7-64-229": [7, 64, 229], "k1": [1] * T}


@pytest.mark.parametrize("name", NAMES)
def test_chunk_invariance_within_the_engine(name):
    m, _ = _model(name)
    n = 7
    x = _x(0, n, T)
    out, rows = {}, {}
    for cname, chunks in CHUNKINGS.items():
        streams = _pool(m, capacity=16)
        streams.open(3)
        ids = streams.open(n)
        out[cname] = _stepped(streams, ids, x, chunks)
        rows[cname] = _rows(streams, ids)
    for cname in CHUNKINGS:
        _same_bits(out[cname], out["k300"])
        _same_bits(rows[cname], rows["k300"])
    assert np.abs(rows["k300"]).sum() > 0


# ---- 3. placement independence ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_a_streams_bits_do_not_depend_on_its_company_or_position(name):
    m, _ = _model(name)
    x = _x(3, 70, 40)
    streams = _pool(m)
    ids = streams.open(70)
    y_all = _stepped(streams, ids, x, [13, 27])
    rows_all = _rows(streams, ids)
    # alone; reversed; a subset, shuffled (other columns, other groups, other XCDs)
    for sel in ([37], list(range(69, -1, -1)), [5, 64, 0, 33, 2, 69, 31]):
        fresh = _pool(m)
        fresh.open(2)
        ids_f = fresh.open(len(sel))
        y = _stepped(fresh, ids_f, x[sel], [13, 27])
        _same_bits(y, y_all[sel])
        _same_bits(_rows(fresh, ids_f), rows_all[sel])


# ---- 4. accuracy against the fp64 oracle, with an initial state -----------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("a", [1, 150, 299])
def test_hand_over_between_the_engines(name, a):
    m, p = _model(name)
    n = 5
    x = _x(7, n, T)
    y_ref, _, _ = _oracle(name, x, p)
    _, h_a, c_a = _oracle(name, x[:, :a], p)
    ref_rows = _rows_of(h_a, c_a)
    xb = torch.from_numpy(x).to(DEV)
    for first, second in (("persistent", "chain"), ("chain", "persistent")):
        streams = _pool(m, capacity=8, engine="chain")
        ids = streams.open(n)
        y1 = streams.step(ids, xb[:, :a], engine=first)
        rows = _rows(streams, ids)
        y2 = streams.step(ids, xb[:, a:], engine=second)
        torch.cuda.synchronize()
        assert streams.verify_launches() == 0
        y = torch.cat([y1, y2], dim=1).cpu().numpy()
        err_y, err_rows = np.abs(y - y_ref).max(), np.abs(rows - ref_rows).max()
        print(f"{name} hand-over a={a} {first}->{second}: max|dy|={err_y:.3e} max|drows|={err_rows:.3e}")
        assert err_y < TOL
        assert err_rows < TOL


@pytest.mark.parametrize("name", NAMES)
def test_from_a_random_state_against_the_oracle(name):
    m, p = _model(name)
    n, k, L = 5, 120, LAYERS[name]
    x = _x(21, n, k)
    rng = np.random.default_rng(4)
    h0 = rng.uniform(-0.9, 0.9, (L, n, 512)).astype(np.float32)      # h = o * tanh(c) lies in (-1, 1)
    c0 = rng.normal(0.0, 1.0, (L, n, 512)).astype(np.float32)
    y_ref, h_ref, c_ref = _oracle(name, x, p, h0.astype(np.float64), c0.astype(np.float64))
    streams = _pool(m, capacity=8)
    streams.open(1)
    ids = streams.open(n)
    streams.set_state(ids, torch.from_numpy(h0), torch.from_numpy(c0))
    y = _stepped(streams, ids, x, [50, 70])
    err_y, err_rows = np.abs(y - y_ref).max(), np.abs(_rows(streams, ids) - _rows_of(h_ref, c_ref)).max()
    print(f"{name} from a random state, {k} frames: max|dy|={err_y:.3e} max|drows|={err_rows:.3e}")
    assert err_y < TOL
    assert err_rows < TOL


# ---- 5. rows and state hygiene ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_rows_the_call_does_not_name_keep_their_bits(name):
    m, _ = _model(name)
    x = _x(20, 3, 60)
    streams = _pool(m, capacity=16)
    ids = streams.open(10)
    named = [ids[7], ids[1], ids[4]]
    others = [i for i in range(16) if i not in named]
    g = torch.Generator(device=DEV).manual_seed(3)
    streams.state[others] = torch.randn((len(others), streams.state.shape[1]), device=DEV, generator=g)
    before = streams.state.clone()
    y = _stepped(streams, named, x, [60])
    assert torch.equal(streams.state[others].view(torch.int32), before[others].view(torch.int32))
    assert not torch.equal(streams.state[named], before[named])
    _same_bits(y, _whole_clip_x(m, x))


@pytest.mark.parametrize("name", NAMES)
def test_state_round_trip_across_two_pools(name):
    m, _ = _model(name)
    x = _x(30, 3, T)
    y_all = _whole_clip_x(m, x)
    a = _pool(m, capacity=8)
    ids = a.open(3)
    y1 = _stepped(a, ids, x[:, :100], [100])
    state = a.get_state(ids)
    assert tuple(state[0].shape) == (LAYERS[name], 3, 512)
    b = _pool(m, capacity=8)
    b.open(2)
    ids_b = b.open(3)
    b.set_state(ids_b, *state)
    y2 = _stepped(b, ids_b, x[:, 100:], [200])
    _same_bits(np.concatenate([y1, y2], axis=1), y_all)
    for s, s_b in zip(a.get_state(ids), state):
        assert torch.equal(s, s_b)


# ---- 6. the chain is unchanged ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_chain_engine_is_what_it_was(name):
    from objectpermanence_amd import LstmStackStreams
    m, _ = _model(name)
    x = _x(11, 33, T)
    y_c = _chain(m, x)
    assert m._runner._monitor.verify() == 0
    default = LstmStackStreams(m, capacity=64)
    assert default.engine == "chain"
    explicit = _pool(m, 64)                   # a persistent pool, told to use the chain call by call
    for streams, engine in ((default, None), (explicit, "chain")):
        y = _stepped(streams, streams.open(33), x, [1, 7, 64, 3, 225], engine=engine)
        _same_bits(y, y_c)
    assert len(default._log) == 0 and len(explicit._log) == 0       # no persistent step, no log
    assert m._runner._monitor.pending() == 0


# ---- 7. replay, without a launch that gives up --------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_replay_of_three_clean_calls_equals_a_chain_only_pool(name, monkeypatch):
    m, _ = _model(name)
    x = _x(9, 6, 50)
    xb = torch.from_numpy(x).to(DEV)
    calls = [([0, 1, 2, 3], 0, 20), ([2, 3, 4, 5], 20, 35), ([5, 0, 3], 35, 50)]      # overlapping slot sets

    def run(streams, engines):
        ids = streams.open(6)
        return ids, [streams.step([ids[i] for i in sel], xb[sel, lo:hi], engine=e) for (sel, lo, hi), e in zip(calls, engines)]

    chain = _pool(m, 8, engine="chain")
    ids_c, out_c = run(chain, ["chain"] * 3)
    healed = _pool(m, 8)
    # keep the log although the launches complete clean: as long as the monitor reaps nothing they count as unverified
    monkeypatch.setattr(m._runner._monitor, "reap", lambda: 0)
    ids_h, out_h = run(healed, ["persistent", "chain", "persistent"])
    torch.cuda.synchronize()
    assert len(healed._log) == 3 and not np.array_equal(_rows(healed, ids_h), _rows(chain, ids_c))
    assert healed._log.replay(healed._log.entries[0]) == 3
    assert healed.healed_calls == 3
    torch.cuda.synchronize()
    for y_h, y_c in zip(out_h, out_c):                                # healed in place: the tensors the caller holds
        _same_bits(y_h.cpu().numpy(), y_c.cpu().numpy())
    _same_bits(_rows(healed, ids_h), _rows(chain, ids_c))
    monkeypatch.undo()
    assert healed.verify_launches() == 0 and len(healed._log) == 0    # empty after a clean verify


def test_set_state_and_open_are_logged_while_the_log_is_kept(monkeypatch):
    m, _ = _model("baseline_lstm")
    x = torch.from_numpy(_x(2, 4, 10)).to(DEV)
    streams = _pool(m, 8)
    ids = streams.open(4)
    monkeypatch.setattr(m._runner._monitor, "reap", lambda: 0)
    streams.step(ids[:2], x[:2])
    h = torch.full((1, 2, 512), 0.25, device=DEV)
    streams.set_state(ids[2:], h, -h)
    new = streams.open(1)
    torch.cuda.synchronize()
    assert [e.payload[0] for e in streams._log.entries] == ["step", "rows", "rows"]
    want = _rows(streams, ids + new)
    streams.state.fill_(7.0)                                          # whatever an aborted run might have left
    streams.state[ids[:2]] = 0.0                                      # ... except the rows of the step itself (left as before)
    assert streams._log.replay(streams._log.entries[0]) == 3
    got = _rows(streams, ids + new)
    assert np.array_equal(got[2:], want[2:])                          # set_state and open were repeated, bit for bit
    chain = _pool(m, 8, engine="chain")
    ids_c = chain.open(2)
    chain.step(ids_c, x[:2])
    _same_bits(got[:2], _rows(chain, ids_c))                          # the step ran again on the chain
    monkeypatch.undo()
    assert streams.verify_launches() == 0 and len(streams._log) == 0


# ---- 8. DetectorStreams on a BaselineLstm pool ----------------------------------------------------------------------------
def test_detector_streams_backlog_persistent_then_chain_ticks():
    from objectpermanence_amd import DetectorStreams
    from objectpermanence_amd.datasets import slot_order
    from objectpermanence_amd.detector_streams import encode_detections_numpy
    from objectpermanence_amd.metrics import postprocess_and_iou
    from test_detector_streams_gpu import _clips, _cone, _dev
    name = "baseline_lstm"
    m, p = _model(name)
    n, backlog, ticks = 5, 300, 6
    det, raws = _clips(n, backlog, seed=50)
    live, _ = _clips(n, ticks, seed=80)
    with pytest.raises(ValueError, match="OPNet only"):     # the constructor's engine= stays OPNet's
        DetectorStreams(m, capacity=16, engine="persistent")
    ds = DetectorStreams(m, capacity=16)
    ds.open(3)
    ids = ds.open(n, classes=[slot_order(lab) for _, lab in raws])
    tables_np = ds.tables.cpu().numpy()
    with pytest.raises(ValueError, match="ragged"):         # refused before anything is encoded
        ds.step_detections(ids, *_dev(det), lengths=[backlog] * n, engine="persistent")
    assert np.array_equal(ds.tables.cpu().numpy(), tables_np)
    warm = ds.open(n)                                       # first calls: weight images, workspaces, the monitor's pinned buffer
    ds.step_detections(warm, *_dev(tuple(a[:, :2] for a in det)), engine="persistent")
    ds.step_detections(warm, *_dev(tuple(a[:, :1] for a in live)))
    dev_backlog, dev_live = _dev(det), [_dev(tuple(a[:, t:t + 1] for a in live)) for t in range(ticks)]
    torch.cuda.synchronize()
    assert ds.verify_launches() == 0
    torch.cuda.set_sync_debug_mode("error")
    try:
        results = [ds.step_detections(ids, *dev_backlog, engine="persistent")]
        results += [ds.step_detections(ids, *d) for d in dev_live]
        with pytest.raises(RuntimeError):
            results[0].y.sum().item()                       # the mode is live on this build
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert ds.verify_launches() == 0 and len(ds.pool._log) == 0
    xs = [encode_detections_numpy(*det, ids, tables_np, _cone(), 5)]
    xs += [encode_detections_numpy(*(a[:, t:t + 1] for a in live), ids, tables_np, _cone(), 5) for t in range(ticks)]
    x_ref = np.concatenate(xs, axis=1)
    _same_bits(torch.cat([r.x for r in results], dim=1).cpu().numpy(), x_ref)
    y = torch.cat([r.y for r in results], dim=1)
    assert torch.equal(torch.cat([r.boxes_px for r in results], dim=1), postprocess_and_iou(y)[0])
    y = y.cpu().numpy()
    err_y = np.abs(y - _oracle(name, x_ref, p)[0]).max()
    print(f"detector backlog {backlog} persistent + {ticks} chain ticks ({name}): max|dy|={err_y:.3e}")
    assert err_y < TOL
    # the backlog alone has the bits of the whole-clip 4-clip forward of the same rows
    _same_bits(y[:, :backlog], _whole_clip_x(m, x_ref[:, :backlog]))


def test_detector_streams_replay_derives_the_pixel_boxes_again(monkeypatch):
    """DetectorStreams registers its pixel boxes behind the step with any pool that keeps a log, not only with OPNetStreams"""
    from objectpermanence_amd import DetectorStreams
    from objectpermanence_amd.metrics import postprocess_and_iou
    from test_detector_streams_gpu import _clips, _dev
    m, _ = _model("baseline_lstm")
    n = 3
    det = _dev(_clips(n, 40, seed=11)[0])
    backlog, tick = tuple(a[:, :39] for a in det), tuple(a[:, 39:] for a in det)
    chain = DetectorStreams(m, capacity=4)
    ids = chain.open(n)
    ref = [chain.step_detections(ids, *backlog), chain.step_detections(ids, *tick)]
    monkeypatch.setattr(m._runner._monitor, "reap", lambda: 0)
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
    for r, r_ref in zip(got, ref):
        _same_bits(r.y.cpu().numpy(), r_ref.y.cpu().numpy())
        assert torch.equal(r.boxes_px, r_ref.boxes_px)
    monkeypatch.undo()
    assert ds.verify_launches() == 0 and len(log) == 0


# ---- other conditions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_weight_update_and_side_stream(name):
    m, _ = _fresh_model(name)
    x = _x(50, 4, 200)
    streams = _pool(m, capacity=16)
    ongoing = streams.open(4)
    _stepped(streams, ongoing, x[:, :100], [100])
    y_old = _whole_clip_x(m, x)
    with torch.no_grad():
        m.predictions_layer.weight.mul_(1.25)
        m.video_LSTM.weight_hh_l0.add_(1e-3)
        if name == "non_linear_lstm":
            m.boxes_linear.weight.mul_(0.9)
    y_next = _stepped(streams, ongoing, x[:, 100:], [100])
    assert not np.array_equal(y_next, y_old[:, 100:])                 # the update took effect on the next call
    y_new = _whole_clip_x(m, x)
    fresh = streams.open(4)
    _same_bits(_stepped(streams, fresh, x, [200]), y_new)
    streams.close(fresh)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ids = streams.open(4)
        y_s = streams.step(ids, torch.from_numpy(x).to(DEV))
    side.synchronize()
    assert streams.verify_launches() == 0
    _same_bits(y_s.cpu().numpy(), y_new)


def test_refusals():
    from objectpermanence_amd import LstmStackStreams, ModelsFactory
    m, _ = _model("baseline_lstm")
    streams = LstmStackStreams(m, capacity=4)
    ids = streams.open(2)
    x = torch.zeros(2, 3, 15, 5, device=DEV)
    with pytest.raises(ValueError, match="no automatic choice"):
        streams.step(ids, x, engine="auto")
    with pytest.raises(ValueError, match="ragged"):
        streams.step(ids, x, [1, 2], engine="persistent")
    with pytest.raises(ValueError, match="engine='chain'"):
        streams.step(ids, x, torch.tensor([1, 2], dtype=torch.int32, device=DEV), engine="persistent")
    small = ModelsFactory.get_model("baseline_lstm", {"videos_hidden_dim": 32}).eval().to(DEV)
    with pytest.raises(ValueError, match="reference shapes"):
        LstmStackStreams(small, capacity=4, engine="persistent")
    pool = LstmStackStreams(small, capacity=4)
    with pytest.raises(ValueError, match="reference shapes"):
        pool.step(pool.open(1), x[:1], engine="persistent")
    lib = _lib()
    lib.opseq_xcd_enable(0)                                           # the existing switch: "not served", the pool refuses
    try:
        with pytest.raises(ValueError, match="OPSEQ_XCD"):
            LstmStackStreams(m, capacity=4, engine="persistent")
    finally:
        lib.opseq_xcd_enable(1)
    assert float(streams.state.abs().sum()) == 0.0                    # nothing ran
    assert LstmStackStreams(m, capacity=4, engine="persistent").engine == "persistent"


# ---- a state word with the sentinel's bits (keep this test last, and to ONE call per model) --------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_a_sentinel_patterned_nan_in_the_state_is_a_plain_nan(name):
    """the exchange buffers mark "not published" with 0xffffffff; a state word with those bits must enter slot 0 as the
    canonical NaN (seq_stream_x_prologue: seq_stream_x_word), or every consumer of it would wait for a publication that never
    comes"""
    m, _ = _model(name)
    L = LAYERS[name]
    x = _x(2, 5, 2)
    clean = _pool(m, 8)
    ids = clean.open(5)
    _stepped(clean, ids, _x(4, 5, 6), [6])                             # some state to start from
    state = [s.clone() for s in clean.get_state(ids)]
    y_ref = _stepped(clean, ids, x, [2])
    rows_ref = _rows(clean, ids)
    bad = _pool(m, 8)
    ids_b = bad.open(5)
    h, c = state[0].clone(), state[1].clone()
    h.view(torch.int32)[0, 2, 17] = -1                                 # 0xffffffff in h of stream 2 (every layer)
    h.view(torch.int32)[L - 1, 2, 5] = -1
    c.view(torch.int32)[0, 3, 200] = -1                                # and in the cell state of stream 3: c never enters an
    c.view(torch.int32)[L - 1, 3, 9] = -1                              # exchange buffer, but the h computed from it does
    bad.set_state(ids_b, h, c)
    y = bad.step(ids_b, torch.from_numpy(x).to(DEV))
    torch.cuda.synchronize()
    assert bad.verify_launches() == 0                                  # no spin-out
    y = y.cpu().numpy()
    assert np.isnan(y[[2, 3]]).all()
    keep = [0, 1, 4]
    _same_bits(y[keep], y_ref[keep])
    _same_bits(_rows(bad, ids_b)[keep], rows_ref[keep])
