"""optim.selection_cross_entropy (opnet_selection_ce_f32) against torch.nn.functional.cross_entropy in fp64: value, gradient,
ignored targets (some and all), both target dtypes, logits up to +-30 (the softmax is recomputed, it has to be stable), and
bit-equal repeats (fixed-order reduction).

Bounds: the value within 2e-6 absolute - l1_mean's bound in tests/test_train_gpu.py; at +-30 the mean is below 32, where
half an fp32 ulp of the returned scalar is 0.95e-6.  The gradient within 1e-4 * max(1e-2, max|ref|), the project's gradient
bound."""
import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 7), (33, 300)]


def _case(B, T, scale, ignore):
    """seeded logits in [-scale, scale] and targets; ignore: "none" / "some" (about a quarter) / "all" """
    n = B * T
    u = synth.counter_uniform(synth.name_seed("selection_ce", B * 1000 + T), n * 17)
    logits = ((u[:n * 15] * 2.0 - 1.0) * scale).astype(np.float32).reshape(B, 15, T)
    tg = np.minimum((u[n * 15:n * 16] * 15).astype(np.int64), 14).reshape(B, T)
    if ignore == "some":
        drop = (u[n * 16:] < 0.25).reshape(B, T)
        drop[0, 0] = False                  # (1, 1) keeps its one target
        tg[drop] = -100
    elif ignore == "all":
        tg[:] = -100
    return logits, tg


def _ref(logits, tg, ignore_index=-100):
    lg = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(tg, dtype=torch.int64)
    if bool((t == ignore_index).all()):
        return 0.0, np.zeros(logits.shape)
    loss = torch.nn.functional.cross_entropy(lg, t, ignore_index=ignore_index)
    loss.backward()
    return float(loss.detach()), lg.grad.numpy()


def _hip(logits, tg, dtype, ignore_index=-100):
    from objectpermanence_amd.optim import selection_cross_entropy
    lg = torch.from_numpy(logits).cuda().requires_grad_()
    loss = selection_cross_entropy(lg, torch.from_numpy(tg).to(dtype).cuda(), ignore_index)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), lg.grad


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("ignore", ["none", "some"])
@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("B,T", SHAPES)
def test_value_and_gradient_match_torch_fp64(B, T, scale, ignore, dtype):
    logits, tg = _case(B, T, scale, ignore)
    ref_loss, ref_grad = _ref(logits, tg)
    loss, grad = _hip(logits, tg, dtype)
    err_v = abs(float(loss) - ref_loss)
    err_g = np.abs(grad.cpu().numpy() - ref_grad).max()
    print(f"selection_ce B={B} T={T} scale={scale} ignore={ignore}: loss {float(loss):.7f} ref {ref_loss:.7f} "
          f"|dv| {err_v:.2e} |dg| {err_g:.2e}")
    assert err_v <= 2e-6
    assert err_g <= 1e-4 * max(1e-2, np.abs(ref_grad).max())


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("B,T", SHAPES)
def test_all_targets_ignored_is_zero_not_nan(B, T, dtype):
    logits, tg = _case(B, T, 30.0, "all")
    loss, grad = _hip(logits, tg, dtype)
    assert float(loss) == 0.0
    assert torch.count_nonzero(grad) == 0 and bool(torch.isfinite(grad).all())


def test_another_ignore_index():
    logits, tg = _case(3, 7, 5.0, "none")
    tg[1, 2] = tg[2, 6] = 7                 # slot 7 is "no label" here
    ref_loss, ref_grad = _ref(logits, tg, ignore_index=7)
    loss, grad = _hip(logits, tg, torch.int64, ignore_index=7)
    assert abs(float(loss) - ref_loss) <= 2e-6
    assert np.abs(grad.cpu().numpy() - ref_grad).max() <= 1e-4 * max(1e-2, np.abs(ref_grad).max())


@pytest.mark.parametrize("B,T", SHAPES)
def test_two_runs_are_bit_equal(B, T):
    logits, tg = _case(B, T, 30.0, "some")
    l1, g1 = _hip(logits, tg, torch.int64)
    l2, g2 = _hip(logits, tg, torch.int64)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_gradient_scales_with_the_upstream_gradient():
    from objectpermanence_amd.optim import selection_cross_entropy
    logits, tg = _case(3, 7, 2.0, "some")
    _, g1 = _hip(logits, tg, torch.int64)
    lg = torch.from_numpy(logits).cuda().requires_grad_()
    (0.5 * selection_cross_entropy(lg, torch.from_numpy(tg).cuda())).backward()
    assert torch.equal(lg.grad, g1 * 0.5)
