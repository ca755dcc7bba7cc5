"""GPU tests of the persistent engine of the OPNet streams (objectpermanence_amd/streaming.py engine="persistent",
csrc/opnet_stream_x4_kernels.hip, opnet_xcd4_forward<false, true>): a stream step as ONE persistent launch of the 4-clip form
that reads each stream's state from the pool and writes it back.

What is pinned: (1) a whole clip in one step has the bits of the existing 4-clip forward; (2) any chunking of the frames into
persistent steps gives the same bits, outputs and pool rows; (3) a stream's bits do not depend on the call's other streams
or its position; (4) a stream handed from one engine to the other stays within the fp64 oracle's bounds of each engine
alone (the measured maxima are in DESIGN.md 12e; the test prints them); (5) rows a call does not name keep their bits, states
round-trip; (6) nothing synchronises the host; (7) the chain engine is what it was.  `pytest -m gpu` on the MI355X box."""
import numpy as np
import pytest
import torch

from oracle import opnet_oracle as oo
from oracle import synth

pytestmark = pytest.mark.gpu

REAL_CFG = {"object_to_track_pred_dim": 15, "object_to_track_hidden_dim": 256, "videos_hidden_dim": 512}
TOL_Y = 2e-5          # the project's bounds for each engine alone over 300 steps (tests/test_opnet_stream_gpu.py)
TOL_LOGITS = 1e-4
DEV = "cuda:0"
T = 300
_CACHE = {}


def _model():
    if "m" not in _CACHE:
        from objectpermanence_amd import ModelsFactory
        m = ModelsFactory.get_model("opnet", REAL_CFG)
        params = synth.opnet_synth_params(REAL_CFG)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
        _CACHE["m"] = (m.eval().to(DEV), params)
    return _CACHE["m"]


def _fresh_model():
    from objectpermanence_amd import ModelsFactory
    m = ModelsFactory.get_model("opnet", REAL_CFG)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.opnet_synth_params(REAL_CFG).items()})
    return m.eval().to(DEV)


def _np(*ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


def _x4_forward(m, boxes):
    """the existing whole-clip 4-clip persistent forward of up to 128 clips -> numpy"""
    xb = torch.from_numpy(boxes).to(DEV)
    with torch.no_grad(), torch.cuda.device(DEV):
        y, lg = m._forward_xcd4(xb, torch.cuda.current_stream().cuda_stream)
    out = _np(y, lg)
    assert m.verify_launches() == 0
    return out


def _chain_forward(m, boxes):
    m.use_xcd = "0"
    try:
        with torch.no_grad():
            y, lg = m(torch.from_numpy(boxes).to(DEV))
    finally:
        m.use_xcd = "auto"
    return _np(y, lg)


def _stepped(streams, ids, boxes, chunks, engine=None, engines=None):
    """boxes [n, T, 15, 6] through `streams` in frame chunks (engines: one engine per chunk) -> numpy (y, logits)"""
    assert sum(chunks) == boxes.shape[1]
    xb = torch.from_numpy(boxes).to(DEV)
    ys, lgs, t = [], [], 0
    for i, k in enumerate(chunks):
        y, lg = streams.step(ids, xb[:, t:t + k], engine=engines[i] if engines else engine)
        ys.append(y)
        lgs.append(lg)
        t += k
    torch.cuda.synchronize()
    assert streams.verify_launches() == 0
    return torch.cat(ys, dim=1).cpu().numpy(), torch.cat(lgs, dim=2).cpu().numpy()


def _pool(m, capacity=256, engine="persistent"):
    from objectpermanence_amd import OPNetStreams
    return OPNetStreams(m, capacity=capacity, engine=engine)


def _same_bits(a, b):
    assert a.shape == b.shape
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"max |diff| {np.abs(a - b).max():.3e}"


def _rows(streams, ids):
    torch.cuda.synchronize()
    return streams.state[torch.tensor(ids, device=DEV)].cpu().numpy()


# ---- 1. whole clip ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 32, 33, 64, 70, 128])
def test_whole_clip_has_the_bits_of_the_4clip_forward(n):
    m, _ = _model()
    boxes, _ = synth.make_batch(11, n, T)
    streams = _pool(m)
    assert streams.engine == "persistent"
    y, lg = _stepped(streams, streams.open(n), boxes, [T])
    if n <= 64:       # the default engine of a small request
        with torch.no_grad():
            y_m, lg_m = _np(*m(torch.from_numpy(boxes).to(DEV)))
        assert m.verify_launches() == 0
    else:
        y_m, lg_m = _x4_forward(m, boxes)
    _same_bits(y, y_m)
    _same_bits(lg, lg_m)


# ---- 2. chunk invariance ----------------------------------------------------------------------------------------------
CHUNKINGS = {"k300": [T], "k1": [1] * T, "mixed": [1, 7, 64, 3, 225]}


@pytest.mark.parametrize("n", [5, 70])
def test_chunk_invariance_within_the_engine(n):
    m, _ = _model()
    boxes, _ = synth.make_batch(0, n, T)
    out, rows = {}, {}
    for name, chunks in CHUNKINGS.items():
        streams = _pool(m)
        streams.open(3)
        ids = streams.open(n)
        out[name] = _stepped(streams, ids, boxes, chunks)
        rows[name] = _rows(streams, ids)
    for name in CHUNKINGS:
        _same_bits(out[name][0], out["k300"][0])
        _same_bits(out[name][1], out["k300"][1])
        _same_bits(rows[name], rows["k300"])
    assert np.abs(rows["k300"]).sum() > 0


# ---- 3. placement independence ----------------------------------------------------------------------------------------
def test_a_streams_bits_do_not_depend_on_its_company_or_position():
    m, _ = _model()
    boxes, _ = synth.make_batch(3, 70, 40)
    streams = _pool(m)
    y_all, lg_all = _stepped(streams, streams.open(70), boxes, [13, 27])
    # alone; reversed; a subset, shuffled (other columns, other XCDs, other row blocks)
    for sel in ([37], list(range(69, -1, -1)), [5, 64, 0, 33, 2, 69, 31]):
        fresh = _pool(m)
        fresh.open(2)
        y, lg = _stepped(fresh, fresh.open(len(sel)), boxes[sel], [13, 27])
        _same_bits(y, y_all[sel])
        _same_bits(lg, lg_all[sel])


# ---- 4. hand-over between the engines ---------------------------------------------------------------------------------
def _oracle_state(boxes, params, a):
    """(h1, c1, h2, c2) of the fp64 oracle after frame a - 1, [n, H] each"""
    _, _, inter = oo.opnet_forward(boxes[:, :a], params, np.float64, return_intermediates=True)
    P = {k: v.astype(np.float64) for k, v in params.items()}
    n = boxes.shape[0]
    scene = boxes[:, :a].astype(np.float64).reshape(n, a, -1)
    _, (h1, c1) = oo.lstm_seq(scene, P["object_to_track_LSTM.weight_ih_l0"], P["object_to_track_LSTM.weight_hh_l0"],
                              return_state=True)
    _, (h2, c2) = oo.lstm_seq(inter["frames_boxes"], P["video_LSTM.weight_ih_l0"], P["video_LSTM.weight_hh_l0"],
                              return_state=True)
    assert np.array_equal(h1, inter["h1"][:, -1]) and np.array_equal(h2, inter["h2"][:, -1])
    return h1, c1, h2, c2


@pytest.mark.parametrize("a", [1, 150, 299])
def test_hand_over_between_the_engines(a):
    m, params = _model()
    n = 5
    boxes, _ = synth.make_batch(7, n, T)
    y_ref, lg_ref = oo.opnet_forward(boxes, params, np.float64)
    ref_state = np.concatenate(_oracle_state(boxes, params, a), axis=1)          # the pool row's [h1 | c1 | h2 | c2]
    for first, second in (("persistent", "chain"), ("chain", "persistent")):
        streams = _pool(m, engine="chain")
        ids = streams.open(n)
        xb = torch.from_numpy(boxes).to(DEV)
        y1, lg1 = streams.step(ids, xb[:, :a], engine=first)
        rows = _rows(streams, ids)
        y2, lg2 = streams.step(ids, xb[:, a:], engine=second)
        torch.cuda.synchronize()
        assert streams.verify_launches() == 0
        y = torch.cat([y1, y2], dim=1).cpu().numpy()
        lg = torch.cat([lg1, lg2], dim=2).cpu().numpy()
        err_y, err_lg, err_rows = np.abs(y - y_ref).max(), np.abs(lg - lg_ref).max(), np.abs(rows - ref_state).max()
        print(f"hand-over a={a} {first}->{second}: max|dy|={err_y:.3e} max|dlogits|={err_lg:.3e} max|drows|={err_rows:.3e}")
        assert err_y < TOL_Y and err_lg < TOL_LOGITS
        assert err_rows < TOL_Y


# ---- 5. untouched rows, state round trips -------------------------------------------------------------------------------
def test_rows_the_call_does_not_name_keep_their_bits():
    m, _ = _model()
    boxes, _ = synth.make_batch(20, 3, 60)
    streams = _pool(m, capacity=16)
    ids = streams.open(10)
    named = [ids[7], ids[1], ids[4]]
    others = [i for i in range(16) if i not in named]
    g = torch.Generator(device=DEV).manual_seed(3)
    streams.state[others] = torch.randn((len(others), streams.state.shape[1]), device=DEV, generator=g)
    before = streams.state.clone()
    y, lg = _stepped(streams, named, boxes, [60])
    assert torch.equal(streams.state[others].view(torch.int32), before[others].view(torch.int32))
    assert not torch.equal(streams.state[named], before[named])
    y_m, lg_m = _x4_forward(m, boxes)
    _same_bits(y, y_m)
    _same_bits(lg, lg_m)


def test_state_round_trip_across_two_pools():
    m, _ = _model()
    boxes, _ = synth.make_batch(30, 3, T)
    y_all, lg_all = _x4_forward(m, boxes)
    a = _pool(m, capacity=8)
    ids = a.open(3)
    y1, lg1 = _stepped(a, ids, boxes[:, :100], [100])
    state = a.get_state(ids)
    b = _pool(m, capacity=8)
    b.open(2)
    ids_b = b.open(3)
    b.set_state(ids_b, *state)
    y2, lg2 = _stepped(b, ids_b, boxes[:, 100:], [200])
    _same_bits(np.concatenate([y1, y2], axis=1), y_all)
    _same_bits(np.concatenate([lg1, lg2], axis=2), lg_all)
    for s, s_b in zip(a.get_state(ids), state):
        assert torch.equal(s, s_b)


# ---- 6. no host sync ----------------------------------------------------------------------------------------------------
def test_persistent_steps_do_not_sync():
    from objectpermanence_amd import DetectorStreams
    from test_detector_streams_gpu import _clips, _dev
    m, _ = _model()
    det = _dev(_clips(4, 10, seed=7)[0])
    ds = DetectorStreams(m, capacity=8, engine="persistent")
    ids = ds.open(4)
    boxes = torch.from_numpy(synth.make_batch(1, 4, 10)[0]).to(DEV)
    slots = torch.tensor(ids, dtype=torch.int32, device=DEV)
    ds.step_detections(ids, *det)             # first call: weight image, workspaces, the monitor's pinned buffer
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r = ds.step_detections(ids, *det)
        r2 = ds.step_detections(ids, *det, engine="chain")
        y, lg = ds.pool._step_slots(slots, boxes, engine="persistent")
        with pytest.raises(RuntimeError):
            y.sum().item()                    # the mode is live on this build
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert ds.verify_launches() == 0
    assert r.y.shape == (4, 10, 4) and r2.logits.shape == (4, 15, 10) and bool(torch.isfinite(y).all())


# ---- 7. the chain is unchanged ------------------------------------------------------------------------------------------
def test_the_chain_engine_is_what_it_was():
    from objectpermanence_amd import OPNetStreams
    m, _ = _model()
    boxes, _ = synth.make_batch(11, 33, T)
    y_c, lg_c = _chain_forward(m, boxes)
    default = OPNetStreams(m, capacity=64)
    assert default.engine == "chain"
    explicit = _pool(m, 64)                   # a persistent pool, told to use the chain call by call
    for streams, engine in ((default, None), (explicit, "chain")):
        y, lg = _stepped(streams, streams.open(33), boxes, [1, 7, 64, 3, 225], engine=engine)
        _same_bits(y, y_c)
        _same_bits(lg, lg_c)
    assert len(default._log) == 0             # no persistent step, no log
    assert m._monitor.pending() == 0


# ---- more than one launch a call, side streams, weight updates ----------------------------------------------------------
def test_200_streams_run_as_two_launches():
    m, _ = _model()
    boxes, _ = synth.make_batch(5, 200, 24)
    streams = _pool(m)
    ids = streams.open(200)
    y, lg = _stepped(streams, ids, boxes, [24])
    two = _pool(m)
    ids2 = two.open(200)
    ya, lga = _stepped(two, ids2[:128], boxes[:128], [24])
    yb, lgb = _stepped(two, ids2[128:], boxes[128:], [24])
    _same_bits(y, np.concatenate([ya, yb]))
    _same_bits(lg, np.concatenate([lga, lgb]))
    _same_bits(_rows(streams, ids), _rows(two, ids2))


def test_weight_update_and_side_stream():
    m = _fresh_model()
    boxes, _ = synth.make_batch(50, 4, 200)
    streams = _pool(m, capacity=8)
    ongoing = streams.open(4)
    _stepped(streams, ongoing, boxes[:, :100], [100])
    y_old, _ = _x4_forward(m, boxes)
    with torch.no_grad():
        m.prediction_layer.weight.mul_(1.25)
        m.object_to_track_LSTM.weight_hh_l0.add_(1e-3)
    y_next, _ = _stepped(streams, ongoing, boxes[:, 100:], [100])
    assert not np.array_equal(y_next, y_old[:, 100:])                 # the update took effect on the next call
    y_new, lg_new = _x4_forward(m, boxes)
    fresh = streams.open(4)
    y, lg = _stepped(streams, fresh, boxes, [200])
    _same_bits(y, y_new)
    _same_bits(lg, lg_new)
    streams.close(fresh)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ids = streams.open(4)
        y_s, lg_s = streams.step(ids, torch.from_numpy(boxes).to(DEV))
    side.synchronize()
    assert streams.verify_launches() == 0
    _same_bits(y_s.cpu().numpy(), y_new)
    _same_bits(lg_s.cpu().numpy(), lg_new)


def test_refusals():
    from objectpermanence_amd import DetectorStreams, ModelsFactory, OPNetStreams
    m, _ = _model()
    streams = OPNetStreams(m, capacity=4)
    ids = streams.open(2)
    x = torch.zeros(2, 3, 15, 6, device=DEV)
    with pytest.raises(ValueError, match="no automatic choice"):
        streams.step(ids, x, engine="auto")
    with pytest.raises(ValueError, match="ragged"):
        streams.step(ids, x, [1, 2], engine="persistent")
    small = ModelsFactory.get_model("opnet", {"object_to_track_pred_dim": 15, "object_to_track_hidden_dim": 16,
                                              "videos_hidden_dim": 32}).eval().to(DEV)
    with pytest.raises(ValueError, match="reference hidden sizes"):
        OPNetStreams(small, capacity=4, engine="persistent")
    pool = OPNetStreams(small, capacity=4)
    with pytest.raises(ValueError, match="reference hidden sizes"):
        pool.step(pool.open(1), x[:1], engine="persistent")
    mlp = ModelsFactory.get_model("opnet_lstm_mlp", REAL_CFG).eval().to(DEV)
    with pytest.raises(TypeError, match="OPNet only"):
        OPNetStreams(mlp, capacity=4, engine="persistent")
    pool = OPNetStreams(mlp, capacity=4)
    with pytest.raises(TypeError, match="OPNet only"):
        pool.step(pool.open(2), x, engine="persistent")
    bl = ModelsFactory.get_model("baseline_lstm", {"videos_hidden_dim": 512}).eval().to(DEV)
    with pytest.raises(ValueError, match="OPNet only"):
        DetectorStreams(bl, capacity=4, engine="persistent")
    assert float(streams.state.abs().sum()) == 0.0                    # nothing ran


# ---- healing, without a launch that gives up ----------------------------------------------------------------------------
def test_replay_of_three_clean_calls_equals_a_chain_only_pool(monkeypatch):
    m, _ = _model()
    boxes, _ = synth.make_batch(9, 6, 50)
    xb = torch.from_numpy(boxes).to(DEV)
    calls = [([0, 1, 2, 3], 0, 20), ([2, 3, 4, 5], 20, 35), ([5, 0, 3], 35, 50)]      # overlapping slot sets

    def run(streams, engines):
        ids = streams.open(6)
        return ids, [streams.step([ids[i] for i in sel], xb[sel, lo:hi], engine=e) for (sel, lo, hi), e in zip(calls, engines)]

    chain = _pool(m, 8, engine="chain")
    ids_c, out_c = run(chain, ["chain"] * 3)
    healed = _pool(m, 8)
    # keep the log although the launches complete clean: as long as the monitor reaps nothing they count as unverified
    monkeypatch.setattr(m._monitor, "reap", lambda: 0)
    ids_h, out_h = run(healed, ["persistent", "chain", "persistent"])
    torch.cuda.synchronize()
    assert len(healed._log) == 3 and not np.array_equal(_rows(healed, ids_h), _rows(chain, ids_c))
    assert healed._log.replay(healed._log.entries[0]) == 3
    assert healed.healed_calls == 3
    for (y_h, lg_h), (y_c, lg_c) in zip(out_h, out_c):                # healed in place: the tensors the caller holds
        _same_bits(*_np(y_h, y_c))
        _same_bits(*_np(lg_h, lg_c))
    _same_bits(_rows(healed, ids_h), _rows(chain, ids_c))
    monkeypatch.undo()
    assert healed.verify_launches() == 0 and len(healed._log) == 0    # empty after a clean verify


# ---- a state word with the sentinel's bits (keep this test last, and to ONE call) -----------------------------------------
def test_a_sentinel_patterned_nan_in_the_state_is_a_plain_nan():
    """the exchange rings mark "not published" with 0xffffffff; a state word with those bits must enter the ring as the
    canonical NaN (opnet_stream_x4_prologue: stream_x4_word), or every consumer of it would wait for a publication that
    never comes"""
    m, _ = _model()
    boxes, _ = synth.make_batch(2, 5, 2)
    clean = _pool(m, 8)
    ids = clean.open(5)
    _stepped(clean, ids, synth.make_batch(4, 5, 6)[0], [6])           # some state to start from
    state = [s.clone() for s in clean.get_state(ids)]
    y_ref, lg_ref = _stepped(clean, ids, boxes, [2])
    bad = _pool(m, 8)
    ids_b = bad.open(5)
    h1 = state[0].clone()
    h1.view(torch.int32)[0, 2, 17] = -1                                # 0xffffffff in stream 2
    h2 = state[2].clone()
    h2.view(torch.int32)[0, 2, 5] = -1
    c1, c2 = state[1].clone(), state[3].clone()                        # and in the cell states of stream 3: c never enters a
    c1.view(torch.int32)[0, 3, 200] = -1                               # ring, but the h computed from it does
    c2.view(torch.int32)[0, 3, 9] = -1
    bad.set_state(ids_b, h1, c1, h2, c2)
    y, lg = bad.step(ids_b, torch.from_numpy(boxes).to(DEV))
    torch.cuda.synchronize()
    assert bad.verify_launches() == 0
    y, lg = y.cpu().numpy(), lg.cpu().numpy()
    assert np.isnan(y[[2, 3]]).all() and np.isnan(lg[[2, 3]]).all()
    keep = [0, 1, 4]
    _same_bits(y[keep], y_ref[keep])
    _same_bits(lg[keep], lg_ref[keep])
