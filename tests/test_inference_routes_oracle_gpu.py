"""The inference routes of the sibling reasoners at full length, against the fp64 port of the reference (oracle/torch_port.py
evaluated on the GPU) at the shapes they were built for:
  A. the stacked LSTM at T = 300 (BaselineLstm: L = 1; NonLinearLstm: L = 2 with the hoisted layer-0 product) on the 4-clip
     latency form (csrc/seq_xcd_kernels.hip) up to its launch maximum, the 16-clip throughput form (csrc/seq_xcdt_kernels.hip)
     from XCDT_MIN_BATCH clips to one full launch and past it (two launches), and the launch chain (csrc/seq_kernels.hip), also at
     the sizes the persistent forms refuse;
  B. both sides of the T-dependent boundaries, found with the library's own sizing functions: the largest T at which
     opseq_xcdt_max_batch still carries its T = 1 batch and the next T, where it shrinks; the largest T at which NonLinearLstm's
     128-clip latency launch fits its 2 GiB workspace and the next T, where the runner takes the chain;
  C. TransformerLstm at T = 300 (2 and 4 heads): lone forwards of 1 - 33 clips (S = 300 .. 9 900 tokens: the attention's key
     split and two query fragments, the tiled encoder products, the throughput stack at 33) and served passes of one-clip
     requests through forward_segments, every request against its own fp64 forward;
  D. OPNetLstmMlp (one route, the launch chain) at 32 and 70 clips x 300 frames, y and the selection logits.
Every case asserts its route (_LstmStackRunner.engine / TransformerLstm.last_pass_engine, the persistent launch counters
including the number of chunks, no aborted launch) and compares every clip at every frame.  fp32 recurrence error grows with t,
so these are the shapes where a wrong group, slot, chunk or 32-bit offset shows.

Non-vacuity: the fp64 outputs must spread at least 100x the bound (max over clips of |y[c] - y[c + 16]|; with 16 clips or fewer,
max over frames of |y[0, t] - y[0, t + 16]|), so a clip in the wrong group or slot, a dropped group or a stale frame cannot pass.

Bounds on max|y - y64| (absolute; the synthetic y spans about +-2): at most 4x the worst measured on the MI355X, recorded in
BOUND below.  At the long-T boundaries the bound is 2x the error of the fp32 port on the same device + 1e-6.  Measured there
(kernel / fp32 port):
  BaselineLstm, throughput form: T0 = 884 carries 1 024 clips, 885 carries 1 008: 1.9e-6 / 5.0e-6 on both sides;
  NonLinearLstm, throughput form: T0 = 511 carries 512 clips, 512 carries 496: 1.7e-6 / 2.2e-6 on both sides;
  NonLinearLstm, 128 clips: T0 = 1 169 runs the latency form on 2 145 914 880 B of workspace (1.3e-6 / 1.9e-6), 1 170 the
  launch chain (1.4e-6 / 1.9e-6)."""
import gc

import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

REAL = {"baseline_lstm": {"videos_hidden_dim": 512},
        "non_linear_lstm": {"boxes_features_dim": 256, "videos_hidden_dim": 512},
        "transformer_lstm": {"boxes_features_dim": 256, "num_attention_heads": 2, "num_attention_layers": 2,
                             "num_lstm_layers": 2, "lstm_hidden_dim": 512},
        "opnet_lstm_mlp": {"object_to_track_pred_dim": 15, "object_to_track_hidden_dim": 256, "videos_hidden_dim": 512}}
PARAMS = {"baseline_lstm": synth.baseline_lstm_synth_params, "non_linear_lstm": synth.non_linear_lstm_synth_params,
          "opnet_lstm_mlp": synth.opnet_lstm_mlp_synth_params, "transformer_lstm": synth.transformer_lstm_synth_params}
LAYERS = {"baseline_lstm": 1, "non_linear_lstm": 2}

# max|y - y64| per route, each at most 4x the worst measured on the MI355X (in the comment, with its case)
BOUND = {
    "baseline_lstm x": 5e-6,              # A. latency form: 1.28e-6 (256 clips)
    "non_linear_lstm x": 5e-6,            #    1.25e-6 (32 and 128 clips)
    "baseline_lstm t": 6e-6,              # A. throughput form: 1.65e-6 (1 024 and 1 027 clips)
    "non_linear_lstm t": 5e-6,            #    1.40e-6 (33 .. 515 clips)
    "baseline_lstm c": 4e-6,              # A. launch chain, H = 512: 1.02e-6
    "non_linear_lstm c": 4e-6,            #    1.23e-6
    "baseline_lstm c wide": 5e-6,         # A. launch chain, H = 1024: 1.48e-6
    "non_linear_lstm c small": 3e-6,      #    (F, H) = (32, 64): 7.6e-7
    "transformer_lstm lone": 1e-4,        # C. lone forwards: 3.21e-5 (32 clips, 4 heads; 1 clip 3.3e-6, 16 clips 1.1e-5)
    "transformer_lstm exact": 1.5e-5,     # C. served, exact = True: 4.8e-6
    "transformer_lstm pass": 5e-5,        # C. served, throughput form: 1.29e-5 (256 and 512 requests)
    "opnet_lstm_mlp y": 1e-5,             # D. 2.65e-6
    "opnet_lstm_mlp logits": 1.5e-5,      #    3.94e-6
}


@pytest.fixture(autouse=True)
def _release_memory():
    """these cases hold several GiB of inputs, fp64 temporaries and workspaces: hand them back before the next one"""
    yield
    gc.collect()
    torch.cuda.empty_cache()


_pool = {}


def _clips(T, B, first=20000):
    """the 6-track boxes of clips first .. first + B - 1 of synth.make_batch at T frames, from a pool grown as needed (a clip
    depends only on its index); one T is kept at a time"""
    for k in [k for k in _pool if k != T]:
        del _pool[k]
    have = _pool.get(T)
    n = 0 if have is None else len(have)
    if n < B:
        more = synth.make_batch(first + n, B - n, T)[0]
        _pool[T] = more if have is None else np.concatenate([have, more])
    return _pool[T][:B]


_params = {}


def _np_params(name, cfg):
    key = (name, tuple(sorted(cfg.items())))
    if key not in _params:
        _params[key] = PARAMS[name](cfg)
    return _params[key]


def _model(name, cfg, xcd="auto", xcdt="auto"):
    from objectpermanence_amd import ModelsFactory
    m = ModelsFactory.get_model(name, cfg)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in _np_params(name, cfg).items()})
    if hasattr(m, "_runner"):
        m._runner.use_xcd, m._runner.use_xcdt = xcd, xcdt
    return m.eval().to("cuda:0")


def _port(name, cfg, x, dtype=torch.float64, n_seg=None):
    """the port's forward of x (host array) on the GPU in `dtype`; n_seg: TransformerLstm.forward_segments' reference"""
    from oracle import torch_port as tp
    p = {k: torch.tensor(v, dtype=dtype, device="cuda") for k, v in _np_params(name, cfg).items()}
    xt = torch.tensor(x, dtype=dtype, device="cuda")
    with torch.no_grad():
        if name == "baseline_lstm":
            return tp.baseline_lstm_forward(xt, p)
        if name == "non_linear_lstm":
            return tp.non_linear_lstm_forward(xt, p)
        if name == "opnet_lstm_mlp":
            return tp.opnet_lstm_mlp_forward(xt, p, with_logits=True)
        nhead = cfg["num_attention_heads"]
        if n_seg is None:
            return tp.transformer_lstm_forward(xt, p, nhead)
        return tp.transformer_lstm_segments_forward(xt, p, nhead, n_seg)


def _run(m, call, engine, launches=1):
    """call() under no_grad on the stack route `engine` ("x" the 4-clip persistent launch, "t" the 16-clip one, "c" the launch
    chain) in `launches` persistent launches: asserted from the runner's counters, its launch monitor and, for TransformerLstm,
    last_pass_engine"""
    r = m._runner
    before = (r.xcd_launches, r.xcdt_launches)
    with torch.no_grad():
        y = call()
    torch.cuda.synchronize()
    assert r._monitor.verify() == 0 and r._monitor.aborted == 0
    if type(m).__name__ == "TransformerLstm":
        assert m.last_pass_engine == engine, (m.last_pass_engine, engine)
    delta = (r.xcd_launches - before[0], r.xcdt_launches - before[1])
    assert delta == {"x": (launches, 0), "t": (0, launches), "c": (0, 0)}[engine], (engine, launches, delta)
    return y


def _stack_forward(m, x, engine, launches=1):
    B, T = x.shape[:2]
    assert m._runner.engine(B, T) == engine, (m._runner.engine(B, T), engine)
    xt = torch.from_numpy(x).cuda()
    return _run(m, lambda: m(xt), engine, launches)


def _spread(ref):
    """what a misplaced result would at least be off by: max over clips of |ref[c] - ref[c + 16]| (a clip in another group or
    slot), with 16 clips or fewer max over frames of |ref[0, t] - ref[0, t + 16]| (a stale frame)"""
    if ref.shape[0] > 16:
        return float((ref[16:] - ref[:-16]).abs().max())
    return float((ref[0, 16:] - ref[0, :-16]).abs().max())


def _check(what, y, ref, bound):
    """y [B, T, ...] against the fp64 ref at every clip and frame: the worst (clip, frame) within `bound`, and the fp64 spread at
    least 100x the bound"""
    assert tuple(y.shape) == tuple(ref.shape), what
    assert bool(torch.isfinite(y).all()), f"{what}: not finite"
    d = (y.double() - ref).abs().flatten(2).amax(-1)               # [B, T]
    c, t = divmod(int(d.argmax()), d.shape[1])
    err, sp = float(d[c, t]), _spread(ref)
    print(f"ERR {what}: {err:.3e} at clip {c} frame {t}; bound {bound:.1e}; spread {sp:.2e}")
    assert sp >= 100 * bound, f"{what}: fp64 spread {sp:.2e} < 100x the bound {bound:.1e}"
    assert err <= bound, f"{what}: max|y - y64| = {err:.3e} at clip {c} frame {t} > {bound:.1e}"
    return err


def _fp32_bound(name, cfg, x, ref):
    """the long-T bound: 2x the error of the fp32 port on the same device + 1e-6"""
    assert not torch.backends.cuda.matmul.allow_tf32
    e32 = float((_port(name, cfg, x, torch.float32).double() - ref).abs().max())
    print(f"ERR {name} fp32 port at {tuple(x.shape[:2])}: {e32:.3e}")
    return 2 * e32 + 1e-6


def _lib():
    from objectpermanence_amd import _lib as lib
    return lib.load()


# ---- A. stacked LSTM at T = 300 ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["baseline_lstm", "non_linear_lstm"])
@pytest.mark.parametrize("B", [1, 5, 32, "max"])
def test_latency_stack_at_300_frames(name, B):
    """one clip / a ragged group / every XCD busy / opseq_xcd_max_batch (256 / 128: eight groups per XCD, or per pair)"""
    cfg = REAL[name]
    if B == "max":
        B = int(_lib().opseq_xcd_max_batch(LAYERS[name]))
        assert B == (256 if name == "baseline_lstm" else 128)
    x = synth.boxes5(_clips(300, B))
    y = _stack_forward(_model(name, cfg, xcdt="0"), x, "x")
    _check(f"{name} latency B={B}", y, _port(name, cfg, x), BOUND[f"{name} x"])


@pytest.mark.parametrize("name", ["baseline_lstm", "non_linear_lstm"])
@pytest.mark.parametrize("which", ["min", "ragged", "max", "max+3"])
def test_throughput_stack_at_300_frames(name, which):
    """the product's route from XCDT_MIN_BATCH clips (65 / 33), a ragged last group (257 / 129), one full launch
    (opseq_xcdt_max_batch: 1024 / 512) and three clips past it (two launches); the full sizes give the same bits twice"""
    cfg = REAL[name]
    m = _model(name, cfg)
    r = m._runner
    cap = int(_lib().opseq_xcdt_max_batch(300, r.L, r.KX, r.H))
    assert cap == (1024 if name == "baseline_lstm" else 512)
    B = {"min": r.XCDT_MIN_BATCH, "ragged": 257 if name == "baseline_lstm" else 129, "max": cap, "max+3": cap + 3}[which]
    launches = -(-B // cap)
    x = synth.boxes5(_clips(300, B))
    y = _stack_forward(m, x, "t", launches)
    _check(f"{name} throughput B={B}", y, _port(name, cfg, x), BOUND[f"{name} t"])
    if which.startswith("max"):
        assert torch.equal(_stack_forward(m, x, "t", launches), y)


@pytest.mark.parametrize("name,cfg,route", [
    ("baseline_lstm", REAL["baseline_lstm"], "c"), ("non_linear_lstm", REAL["non_linear_lstm"], "c"),
    # sizes the persistent forms refuse: the product itself routes them to the chain
    ("baseline_lstm", {"videos_hidden_dim": 1024}, "c wide"),
    ("non_linear_lstm", {"boxes_features_dim": 32, "videos_hidden_dim": 64}, "c small")])
def test_launch_chain_at_300_frames(name, cfg, route):
    """32 clips on the launch chain: forced at H = 512 (use_xcd = "0"), the route of H = 1024 and (F, H) = (32, 64)"""
    x = synth.boxes5(_clips(300, 32))
    y = _stack_forward(_model(name, cfg, xcd="0" if route == "c" else "auto"), x, "c")
    _check(f"{name} chain {cfg}", y, _port(name, cfg, x), BOUND[f"{name} {route}"])


# ---- C. TransformerLstm at T = 300 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("B", [1, 16, 28, 32, 33])
def test_transformer_lone_forward_at_300_frames(heads, B):
    """S = 300 / 4 800 / 8 400 / 9 600 / 9 900 tokens: one clip, the tiled encoder products and key split, two query fragments,
    the throughput stack from XCDT_MIN_BATCH (33) clips"""
    cfg = dict(REAL["transformer_lstm"], num_attention_heads=heads)
    m = _model("transformer_lstm", cfg)
    engine = "t" if B >= m._runner.XCDT_MIN_BATCH else "x"
    assert m._runner.engine(B, 300) == engine
    x = synth.boxes5(_clips(300, B))
    xt = torch.from_numpy(x).cuda()
    y = _run(m, lambda: m(xt), engine)
    _check(f"transformer_lstm heads={heads} lone B={B}", y, _port("transformer_lstm", cfg, x), BOUND["transformer_lstm lone"])


@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("n,exact", [(16, True), (40, False), (256, False), ("pass", False)])
def test_transformer_served_pass_at_300_frames(heads, n, exact):
    """n one-clip requests in one forward_segments pass: exact = True (the segmented encoder and the 4-clip stack, the lone
    request's kernels) and the throughput form up to max_requests_per_pass(1, 300) requests (one full 16-clip launch).  Every
    request against its own fp64 forward: the port's segmented composite, pinned to transformer_lstm_forward on three requests"""
    cfg = dict(REAL["transformer_lstm"], num_attention_heads=heads)
    m = _model("transformer_lstm", cfg)
    if n == "pass":
        n = m.max_requests_per_pass(1, 300)
        assert n > 256
    engine = "x" if exact else "t"
    assert m.pass_engine(n, 1, 300, exact) == engine
    x = synth.boxes5(_clips(300, n))
    xt = torch.from_numpy(x).cuda()
    y = _run(m, lambda: m.forward_segments(xt, n, exact=exact), engine)
    ref = _port("transformer_lstm", cfg, x, n_seg=n)
    for r in (0, n // 2, n - 1):
        lone = _port("transformer_lstm", cfg, x[r:r + 1])
        assert float((ref[r:r + 1] - lone).abs().max()) <= 1e-10, r
    _check(f"transformer_lstm heads={heads} pass n={n} exact={exact}", y, ref,
           BOUND["transformer_lstm exact" if exact else "transformer_lstm pass"])


# ---- D. OPNetLstmMlp -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [32, 70])
def test_opnet_lstm_mlp_at_300_frames(B):
    """its one route, the launch chain of opnet_mlp_forward_f32 (no persistent form to force): y and logits [B, 15, T]"""
    cfg = REAL["opnet_lstm_mlp"]
    m = _model("opnet_lstm_mlp", cfg)
    assert not hasattr(m, "_runner")
    boxes = np.ascontiguousarray(_clips(300, B))
    with torch.no_grad():
        y, logits = m(torch.from_numpy(boxes).cuda())
    torch.cuda.synchronize()
    y_ref, logits_ref = _port("opnet_lstm_mlp", cfg, boxes)
    _check(f"opnet_lstm_mlp B={B} y", y, y_ref, BOUND["opnet_lstm_mlp y"])
    _check(f"opnet_lstm_mlp B={B} logits", logits.transpose(1, 2), logits_ref.transpose(1, 2), BOUND["opnet_lstm_mlp logits"])


# ---- B. around the T-dependent boundaries --------------------------------------------------------------------------------------
# (last in the file: their clips are longer than 300 frames, and _clips keeps one T at a time)

def _last_T(pred, hi=1 << 14):
    """the largest T >= 1 with pred(T), pred monotone (true up to some T, false beyond)"""
    assert pred(1) and not pred(hi)
    lo = 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo


@pytest.mark.parametrize("name", ["baseline_lstm", "non_linear_lstm"])
@pytest.mark.parametrize("side", ["at", "past"])
def test_throughput_stack_around_the_launch_cap_boundary(name, side):
    """T0 = the largest T at which opseq_xcdt_max_batch still returns its T = 1 cap, and T0 + 1, where it shrinks; a full launch
    of the returned cap at each"""
    cfg = REAL[name]
    m = _model(name, cfg)
    r = m._runner
    lib = _lib()
    cap = lambda T: int(lib.opseq_xcdt_max_batch(T, r.L, r.KX, r.H))
    T0 = _last_T(lambda T: cap(T) == cap(1))
    assert cap(T0 + 1) < cap(T0)
    print(f"BOUNDARY {name} xcdt: T0 = {T0} carries {cap(T0)} clips, T0 + 1 carries {cap(T0 + 1)}")
    T = T0 if side == "at" else T0 + 1
    B = cap(T)
    x = synth.boxes5(_clips(T0 + 1, cap(T0))[:B, :T])
    y = _stack_forward(m, x, "t")
    ref = _port(name, cfg, x)
    _check(f"{name} throughput T={T} B={B}", y, ref, _fp32_bound(name, cfg, x, ref))
    assert torch.equal(_stack_forward(m, x, "t"), y)


@pytest.mark.parametrize("side", ["at", "past"])
def test_latency_stack_around_the_workspace_boundary(side):
    """NonLinearLstm's 128-clip latency launch: T0 = the largest T at which opseq_xcd_workspace_bytes is nonzero (the persistent
    form runs on a workspace just under 2 GiB), and T0 + 1, where the runner takes the launch chain"""
    name, cfg = "non_linear_lstm", REAL["non_linear_lstm"]
    m = _model(name, cfg, xcdt="0")
    r = m._runner
    lib = _lib()
    B = int(lib.opseq_xcd_max_batch(2))
    T0 = _last_T(lambda T: int(lib.opseq_xcd_workspace_bytes(B, T, r.L, r.KX, r.H)) > 0)
    assert int(lib.opseq_xcd_workspace_bytes(B, T0, r.L, r.KX, r.H)) > (1 << 31) - (64 << 20)
    print(f"BOUNDARY {name} xcd: T0 = {T0} ({int(lib.opseq_xcd_workspace_bytes(B, T0, r.L, r.KX, r.H))} B of workspace)")
    T = T0 if side == "at" else T0 + 1
    x = synth.boxes5(_clips(T0 + 1, B)[:, :T])
    y = _stack_forward(m, x, "x" if side == "at" else "c")
    ref = _port(name, cfg, x)
    _check(f"{name} {'latency' if side == 'at' else 'chain'} T={T} B={B}", y, ref, _fp32_bound(name, cfg, x, ref))
