"""The opt-in gradients of OPNet / OPNetLstmMlp - through the selection logits (`model(x, logits_grad=True)`) and to the
input boxes (`boxes.requires_grad`) - against oracle/torch_port.py in fp64 under torch autograd.

Loss of the oracle cases: l1_mean(y, labels) + 0.5 * cross_entropy(logits, targets, ignore_index=-100), seeded targets, about
a quarter of them ignored.  Bound (the project's own, tests/test_train_gpu.py::test_gradients_match_torch_port_ragged):
max|g - ref| <= 1e-4 * max(1e-2, max|ref|) for the six weight gradients and for d boxes, the loss within 2e-6.  torch_port in
fp32 against fp64 stays below 1 % of that bound at these shapes, d boxes included.

A step with an extra runs its reverse recurrence on the launch chain.  Routes reached by the shapes (reference hidden sizes):
    (1, 1), (2, 5)   fused chain behind the 4-clip persistent forward
    (33, 6)          two sliced chains (4-clip persistent forward)
    (70, 3)          sliced
    (131, 4)         five row blocks: three slices behind the 16-clip persistent forward; OPNetLstmMlp: the split pair
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import synth, torch_port

pytestmark = pytest.mark.gpu

REAL_CFG = {"object_to_track_pred_dim": 15, "object_to_track_hidden_dim": 256, "videos_hidden_dim": 512}
PARAMS = {"opnet": synth.opnet_synth_params, "opnet_lstm_mlp": synth.opnet_lstm_mlp_synth_params}
FORWARD = {"opnet": torch_port.opnet_forward,
           "opnet_lstm_mlp": lambda x, p: torch_port.opnet_lstm_mlp_forward(x, p, with_logits=True)}
SHAPES = [(1, 1), (2, 5), (33, 6), (70, 3), (131, 4)]


def _targets(B, T):
    u = synth.counter_uniform(synth.name_seed("selection_targets", B * 1000 + T), 2 * B * T)
    tg = np.minimum((u[:B * T] * 15).astype(np.int64), 14).reshape(B, T)
    drop = (u[B * T:] < 0.25).reshape(B, T)
    drop[0, 0] = False                      # (a batch of one frame keeps its target: the mean over nothing is not a loss)
    tg[drop] = -100
    return tg


def _model(name, cfg):
    from objectpermanence_amd import ModelsFactory
    m = ModelsFactory.get_model(name, cfg)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in PARAMS[name](cfg).items()})
    return m.to("cuda:0").train(True)


_ORACLE = {}


def _oracle(name, cfg, B, T, loss_kind="both"):
    """fp64 loss, the weight gradients and d boxes; computed once per case and shared (read-only)"""
    key = (name, json.dumps(cfg, sort_keys=True), B, T, loss_kind)
    if key not in _ORACLE:
        boxes, labels = synth.make_batch(200, B, T)
        p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in PARAMS[name](cfg).items()}
        x = torch.tensor(boxes, dtype=torch.float64, requires_grad=True)
        y, logits = FORWARD[name](x, p)
        l1 = torch_port.l1_mean(y, torch.tensor(labels, dtype=torch.float64))
        ce = torch.nn.functional.cross_entropy(logits, torch.tensor(_targets(B, T)), ignore_index=-100)
        loss = {"both": l1 + 0.5 * ce, "logits": ce, "l1": l1}[loss_kind]
        loss.backward()
        grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in p.items()}
        _ORACLE[key] = (float(loss.detach()), grads, x.grad.numpy())
    return _ORACLE[key]


def _hip(name, cfg, B, T, loss_kind="both", boxes_grad=True):
    from objectpermanence_amd import l1_mean
    from objectpermanence_amd.optim import selection_cross_entropy
    boxes, labels = synth.make_batch(200, B, T)
    m = _model(name, cfg)
    x = torch.from_numpy(boxes).cuda()
    if boxes_grad:
        x.requires_grad_()
    y, logits = m(x, logits_grad=loss_kind != "l1")
    lab, tg = torch.from_numpy(labels).cuda(), torch.from_numpy(_targets(B, T)).cuda()
    if loss_kind == "both":
        loss = l1_mean(y, lab) + 0.5 * selection_cross_entropy(logits, tg)
    elif loss_kind == "logits":
        loss = selection_cross_entropy(logits, tg)
    else:
        loss = l1_mean(y, lab)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
    return float(loss.detach()), grads, (x.grad.cpu().numpy() if boxes_grad else None)


def _check(tag, got, ref, boxes_grad=True):
    loss, grads, dboxes = got
    ref_loss, ref_grads, ref_dboxes = ref
    print(f"{tag}: loss {loss:.7f} ref {ref_loss:.7f}")
    items = list(grads.items()) + ([("d boxes", dboxes)] if boxes_grad else [])
    errs = {}
    for k, g in items:
        r = ref_dboxes if k == "d boxes" else ref_grads[k]
        assert g.shape == r.shape, k
        errs[k] = (np.abs(g - r).max(), 1e-4 * max(1e-2, np.abs(r).max()))
        print(f"  {k}: max|g - ref| {errs[k][0]:.3e}  bound {errs[k][1]:.3e}  max|ref| {np.abs(r).max():.3e}")
    assert loss == pytest.approx(ref_loss, abs=2e-6)
    for k, (e, bound) in errs.items():
        assert np.isfinite(e) and e <= bound, (tag, k, e, bound)


@pytest.mark.parametrize("B,T", SHAPES)
def test_opnet_both_extras_match_the_oracle(B, T):
    _check(f"opnet {B}x{T}", _hip("opnet", REAL_CFG, B, T), _oracle("opnet", REAL_CFG, B, T))


def test_opnet_split_pair_head_matches_the_oracle(monkeypatch):
    """OPNET_BWD_MODE=split: the head of opnet_bwd_cell carries both extras too"""
    monkeypatch.setenv("OPNET_BWD_MODE", "split")
    _check("opnet split 33x6", _hip("opnet", REAL_CFG, 33, 6), _oracle("opnet", REAL_CFG, 33, 6))


@pytest.mark.parametrize("B,T", [(2, 5), (131, 4)])      # 131: five row blocks reach the split pair unaided
def test_opnet_lstm_mlp_both_extras_match_the_oracle(B, T):
    _check(f"opnet_lstm_mlp {B}x{T}", _hip("opnet_lstm_mlp", REAL_CFG, B, T), _oracle("opnet_lstm_mlp", REAL_CFG, B, T))


@pytest.mark.parametrize("name", ["opnet", "opnet_lstm_mlp"])
def test_small_hidden_sizes(name, golden_dir):
    """the tiny golden's hidden sizes (16 / 32): one hexadecet of K per wave of the box-gradient product"""
    g = np.load(os.path.join(golden_dir, "opnet_train_tiny.npz"))
    cfg = json.loads(str(g["cfg"]))
    B, T = int(g["n_clips"]), int(g["t_frames"])
    _check(f"{name} tiny {B}x{T}", _hip(name, cfg, B, T), _oracle(name, cfg, B, T))


@pytest.mark.parametrize("name,B,T", [("opnet", 2, 5), ("opnet", 33, 6), ("opnet_lstm_mlp", 2, 5)])
def test_logit_gradient_alone(name, B, T):
    """a loss on the selection only: grad_y is None, the video stage gets zero gradients"""
    got = _hip(name, REAL_CFG, B, T, loss_kind="logits", boxes_grad=False)
    _check(f"{name} logits only {B}x{T}", got, _oracle(name, REAL_CFG, B, T, "logits"), boxes_grad=False)
    assert not np.any(got[1]["prediction_layer.weight"])


@pytest.mark.parametrize("name,B,T", [("opnet", 2, 5), ("opnet", 33, 6), ("opnet_lstm_mlp", 2, 5)])
def test_box_gradient_alone(name, B, T):
    """boxes.requires_grad under the plain L1 loss, the logits non-differentiable as ever"""
    _check(f"{name} boxes only {B}x{T}", _hip(name, REAL_CFG, B, T, loss_kind="l1"), _oracle(name, REAL_CFG, B, T, "l1"))


def test_box_gradient_of_a_frozen_model():
    """saliency on a model whose weights do not train: `boxes` alone asks for a gradient"""
    from objectpermanence_amd import l1_mean
    B, T = 2, 5
    boxes, labels = synth.make_batch(200, B, T)
    m = _model("opnet", REAL_CFG)
    for p in m.parameters():
        p.requires_grad_(False)
    x = torch.from_numpy(boxes).cuda().requires_grad_()
    l1_mean(m(x)[0], torch.from_numpy(labels).cuda()).backward()
    ref = _oracle("opnet", REAL_CFG, B, T, "l1")[2]
    assert np.abs(x.grad.cpu().numpy() - ref).max() <= 1e-4 * max(1e-2, np.abs(ref).max())
    assert all(p.grad is None for p in m.parameters())


# ---- unchanged when not asked ------------------------------------------------------------------
def test_logits_stay_non_differentiable_by_default():
    boxes, _ = synth.make_batch(5, 2, 4)
    m = _model("opnet", REAL_CFG)
    x = torch.from_numpy(boxes).cuda()
    y, logits = m(x)
    assert y.requires_grad and not logits.requires_grad
    y, logits = m(x, logits_grad=True)
    assert y.requires_grad and logits.requires_grad
    with torch.no_grad():
        y, logits = m(x, logits_grad=True)
    assert not y.requires_grad and not logits.requires_grad
    m2 = _model("opnet_lstm_mlp", REAL_CFG)
    assert not m2(x)[1].requires_grad and m2(x, logits_grad=True)[1].requires_grad


def _six(m, x, lab, logits_grad, through_logits):
    from objectpermanence_amd import l1_mean
    m.zero_grad(set_to_none=True)
    y, logits = m(x, logits_grad=logits_grad)
    loss = l1_mean(y, lab)
    if through_logits:
        loss = loss + 0.0 * logits.sum()          # an all-zero gradient arrives through the logits: the route with extras
    loss.backward()
    torch.cuda.synchronize()
    return {k: p.grad.clone() for k, p in m.named_parameters()}


def test_unused_logits_change_nothing():
    """(6, 50): a step with logits_grad=True whose loss ignores the logits - or reaches them with a zero gradient, which runs
    the chain where the plain step runs the persistent reverse recurrence - gives the plain step's gradients within the bound"""
    boxes, labels = synth.make_batch(5, 6, 50)
    m = _model("opnet", REAL_CFG)
    x, lab = torch.from_numpy(boxes).cuda(), torch.from_numpy(labels).cuda()
    plain = _six(m, x, lab, False, False)
    for through in (False, True):
        got = _six(m, x, lab, True, through)
        for k, r in plain.items():
            assert float((got[k] - r).abs().max()) <= 1e-4 * max(1e-2, float(r.abs().max())), (through, k)


def test_unused_logits_are_bit_equal_on_the_chain(monkeypatch):
    """... and with the reverse recurrence on the chain on both sides (OPNET_XCD4_BWD=0) the same bits"""
    monkeypatch.setenv("OPNET_XCD4_BWD", "0")
    boxes, labels = synth.make_batch(5, 6, 50)
    m = _model("opnet", REAL_CFG)
    x, lab = torch.from_numpy(boxes).cuda(), torch.from_numpy(labels).cuda()
    plain = _six(m, x, lab, False, False)
    for through in (False, True):
        got = _six(m, x, lab, True, through)
        for k, r in plain.items():
            assert torch.equal(got[k], r), (through, k)


def test_backward_after_second_forward_is_still_refused():
    from objectpermanence_amd.optim import selection_cross_entropy
    boxes, _ = synth.make_batch(5, 2, 8)
    tg = torch.from_numpy(_targets(2, 8)).cuda()
    for name in ("opnet", "opnet_lstm_mlp"):
        m = _model(name, REAL_CFG)
        x = torch.from_numpy(boxes).cuda().requires_grad_()
        _, lg1 = m(x, logits_grad=True)
        _, lg2 = m(x, logits_grad=True)
        with pytest.raises(RuntimeError, match="overwritten"):
            selection_cross_entropy(lg1, tg).backward()
        selection_cross_entropy(lg2, tg).backward()
        assert x.grad is not None


# ---- integration -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["opnet", "opnet_lstm_mlp"])
def test_train_step_with_selection_targets(name):
    """training.train_step(..., selection_targets=..., selection_weight=0.5): the loss is the oracle's, and one FusedAdam step
    moves the weights as the oracle's gradients say.  First Adam step: u = lr * g / (|g| + eps), so |u| <= lr whatever g is
    (hard bound on any difference: 2 lr), and where |g_ref| exceeds ten times the gradient bound d the sign is certain and
    the step differs by at most lr * eps * d / (9 d)^2 < 2e-7 plus the rounding of the weight - checked at 1e-6."""
    from objectpermanence_amd import FusedAdam
    from objectpermanence_amd.training import train_step
    B, T, lr = 33, 6, 1e-3
    boxes, labels = synth.make_batch(200, B, T)
    m = _model(name, REAL_CFG)
    opt = FusedAdam(m.parameters(), lr=lr)
    loss = train_step(name, m, opt, torch.from_numpy(boxes).cuda(), torch.from_numpy(labels).cuda(),
                      selection_targets=torch.from_numpy(_targets(B, T)).cuda(), selection_weight=0.5)
    torch.cuda.synchronize()
    ref_loss, ref_grads, _ = _oracle(name, REAL_CFG, B, T)
    assert float(loss) == pytest.approx(ref_loss, abs=2e-6)
    ref_w = {k: v.copy() for k, v in PARAMS[name](REAL_CFG).items()}
    torch_port.adam_step(ref_w, {k: v.astype(np.float32) for k, v in ref_grads.items()}, {}, lr=lr)
    for k, p in m.named_parameters():
        w, g = p.detach().cpu().numpy(), ref_grads[k]
        diff = np.abs(w - ref_w[k])
        assert diff.max() <= 2.1 * lr, k
        sure = np.abs(g) > 10 * 1e-4 * max(1e-2, np.abs(g).max())
        assert sure.any() and diff[sure].max() <= 1e-6, (k, diff[sure].max())


def test_train_step_without_targets_is_the_plain_step():
    from objectpermanence_amd import FusedAdam
    from objectpermanence_amd.training import train_step
    boxes, labels = synth.make_batch(5, 6, 20)
    x, lab = torch.from_numpy(boxes).cuda(), torch.from_numpy(labels).cuda()
    out = []
    for kw in ({}, {"selection_targets": None, "selection_weight": 3.0}):
        m = _model("opnet", REAL_CFG)
        loss = train_step("opnet", m, FusedAdam(m.parameters(), lr=1e-3), x, lab, **kw)
        torch.cuda.synchronize()
        out.append((loss.clone(), [p.detach().clone() for p in m.parameters()]))
    assert torch.equal(out[0][0], out[1][0])
    assert all(torch.equal(a, b) for a, b in zip(out[0][1], out[1][1]))


def test_opnet_lstm_mlp_step_over_a_dirty_workspace():
    """131 clips at the reference sizes: the status words of the training workspace are those of OPNet's 16-clip persistent
    forward, which OPNetLstmMlp never runs - its forward has to clear them, or whatever the allocator left there turns every
    gradient into NaN.  The history is allocated over a block of 0xFF bytes (same size: the caching allocator hands it back)."""
    from objectpermanence_amd import _lib, l1_mean
    B, T = 131, 4
    n = _lib.load().opnet_train_workspace_bytes(B, T, 256, 512)
    dirty = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    del dirty
    boxes, labels = synth.make_batch(200, B, T)
    m = _model("opnet_lstm_mlp", REAL_CFG)
    for extras in (False, True):
        m.zero_grad(set_to_none=True)
        x = torch.from_numpy(boxes).cuda().requires_grad_(extras)
        l1_mean(m(x)[0], torch.from_numpy(labels).cuda()).backward()
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters()), extras
        assert not extras or bool(torch.isfinite(x.grad).all())
