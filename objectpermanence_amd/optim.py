"""Loss and optimiser of the reference's training step on device.

* ``l1_mean(y, labels)``  == ``torch.mean(nn.L1Loss(reduction="none")(y, labels))``
  (reference baselines/training_main.py:152,192,204) - one fused forward+backward kernel pair.
* ``selection_cross_entropy(logits, targets)`` == ``F.cross_entropy(logits, targets, ignore_index=-100)`` on the
  selection logits [B,15,T] of OPNet / OPNetLstmMlp (which the reference permutes "for CE loss",
  learned_models.py:49-50) - one HIP call for value and gradient.
* ``FusedAdam``           == ``torch.optim.Adam(params, lr)`` with the reference's defaults
  (training_main.py:150): betas (0.9, 0.999), eps 1e-8, no weight decay.  It is a
  ``torch.optim.Optimizer`` so ``ReduceLROnPlateau`` (training_main.py:151,247) drives it unchanged.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib


class _L1Mean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, labels, beta=0.0):
        if not y.is_cuda:
            raise RuntimeError("l1_mean runs on the GPU only (no CPU fallback)")
        lib = _lib.load()
        y = y.contiguous().float()
        labels = labels.to(y.device).contiguous().float()
        n = y.numel()
        loss = torch.empty((), dtype=torch.float32, device=y.device)
        dy = torch.empty_like(y)
        scratch = torch.empty(4096, dtype=torch.uint8, device=y.device)
        with torch.cuda.device(y.device):
            st = torch.cuda.current_stream(y.device).cuda_stream
            if beta > 0:
                rc = lib.opnet_smooth_l1_loss_f32(y.data_ptr(), labels.data_ptr(), loss.data_ptr(), dy.data_ptr(), n,
                                                  float(beta), scratch.data_ptr(), scratch.numel(), st)
            else:
                rc = lib.opnet_l1_loss_f32(y.data_ptr(), labels.data_ptr(), loss.data_ptr(), dy.data_ptr(), n,
                                           scratch.data_ptr(), scratch.numel(), st)
        _lib.check(rc, "opnet_l1_loss_f32")
        ctx.save_for_backward(dy)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (dy,) = ctx.saved_tensors
        return dy * grad_out, None, None


def loss_and_grad(y: torch.Tensor, labels: torch.Tensor, beta: float = 0.0):
    """(loss, dloss/dy) of the supervised loss WITHOUT an autograd node: a training step that calls `y.backward(dy)` itself
    saves the two launches `loss.backward()` spends on the implicit gradient 1.0 (a fill) and on `dy * 1.0`."""
    if not y.is_cuda:
        raise RuntimeError("loss_and_grad runs on the GPU only (no CPU fallback)")
    lib = _lib.load()
    yd = y.detach().contiguous().float()
    labels = labels.to(yd.device).contiguous().float()
    n = yd.numel()
    loss = torch.empty((), dtype=torch.float32, device=yd.device)
    dy = torch.empty_like(yd)
    scratch = torch.empty(4096, dtype=torch.uint8, device=yd.device)
    with torch.cuda.device(yd.device):
        st = torch.cuda.current_stream(yd.device).cuda_stream
        if beta > 0:
            rc = lib.opnet_smooth_l1_loss_f32(yd.data_ptr(), labels.data_ptr(), loss.data_ptr(), dy.data_ptr(), n, float(beta),
                                              scratch.data_ptr(), scratch.numel(), st)
        else:
            rc = lib.opnet_l1_loss_f32(yd.data_ptr(), labels.data_ptr(), loss.data_ptr(), dy.data_ptr(), n, scratch.data_ptr(),
                                       scratch.numel(), st)
    _lib.check(rc, "opnet_l1_loss_f32")
    return loss, dy


def l1_mean(y: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    return _L1Mean.apply(y, labels, 0.0)


def smooth_l1_mean(y: torch.Tensor, labels: torch.Tensor, beta: float = 1.0) -> torch.Tensor:
    """torch.nn.SmoothL1Loss(beta=beta)(y, labels) - the loss BASELINE.json's config 2 names (the reference
    trains with L1; this is the extra knob SURVEY.md section 0 asks for)."""
    return _L1Mean.apply(y, labels, float(beta))


def selection_loss_and_grad(logits: torch.Tensor, targets: torch.Tensor, ignore_index: int = -100):
    """(loss, dloss/dlogits) of the mean cross-entropy of the selection logits [B,15,T] against targets [B,T] (int32 or int64
    slot indices; ignore_index entries do not count) WITHOUT an autograd node - see loss_and_grad.  One call of
    opnet_selection_ce_f32: fixed-order reduction (the same bits every run), all targets ignored gives loss 0 / gradient 0."""
    if not logits.is_cuda:
        raise RuntimeError("selection_cross_entropy runs on the GPU only (no CPU fallback)")
    if logits.dim() != 3 or logits.shape[1] != 15:
        raise ValueError(f"logits must be [B, 15, T], got {tuple(logits.shape)}")
    B, T = int(logits.shape[0]), int(logits.shape[2])
    if tuple(targets.shape) != (B, T):
        raise ValueError(f"targets must be [B, T] = [{B}, {T}], got {tuple(targets.shape)}")
    if targets.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"targets must be int32 or int64, got {targets.dtype}")
    lib = _lib.load()
    lg = logits.detach().contiguous().float()
    tg = targets.to(lg.device).contiguous()
    loss = torch.empty((), dtype=torch.float32, device=lg.device)
    dlg = torch.empty_like(lg)
    scratch = torch.empty(16384, dtype=torch.uint8, device=lg.device)
    with torch.cuda.device(lg.device):
        rc = lib.opnet_selection_ce_f32(lg.data_ptr(), tg.data_ptr(), int(tg.dtype == torch.int64), int(ignore_index), loss.data_ptr(),
                                        dlg.data_ptr(), B, T, scratch.data_ptr(), scratch.numel(),
                                        torch.cuda.current_stream(lg.device).cuda_stream)
    _lib.check(rc, "opnet_selection_ce_f32")
    return loss, dlg


class _SelectionCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, ignore_index):
        loss, dlg = selection_loss_and_grad(logits, targets, ignore_index)
        ctx.save_for_backward(dlg)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (dlg,) = ctx.saved_tensors
        return dlg * grad_out, None, None


def selection_cross_entropy(logits: torch.Tensor, targets: torch.Tensor, ignore_index: int = -100) -> torch.Tensor:
    """torch.nn.functional.cross_entropy(logits [B,15,T], targets [B,T], ignore_index=ignore_index): which slot the model
    should look at in each frame.  The logits must come from a forward with logits_grad=True for the loss to reach the
    weights."""
    return _SelectionCE.apply(logits, targets, int(ignore_index))


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, grad_scale: float = 1.0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, grad_scale=grad_scale))
        # device-side guards of the next step() (opnet_adam_multi_step_guarded_f32; set by training.train_step, None = off):
        # abort word of the persistent launches behind the gradients | the loss (skip if not finite) | data-parallel guard
        self.abort_ptr = None
        self.loss_ptr = None
        self.guard_ptr = None
        self._last_stepped = []

    def rollback_step_count(self) -> None:
        """undo the step COUNTERS of the last step(): for a step whose update the device-side guard skipped (parameters and
        moments untouched) and that the caller is about to repeat"""
        for st in self._last_stepped:
            st["step"] -= 1
        self._last_stepped = []

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        self._last_stepped = []
        for group in self.param_groups:
            b1, b2 = group["betas"]
            # parameters of one device that are at the same step share ONE launch (opnet_adam_multi_step_f32: up to 16 tensors)
            batches = {}
            keep = []
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise RuntimeError("FusedAdam runs on the GPU only (no CPU fallback)")
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["step"] += 1
                self._last_stepped.append(st)
                g = p.grad.contiguous()
                keep.append(g)
                batches.setdefault((p.device, int(st["step"])), []).append((p, g, st))
            for (dev, step_no), items in batches.items():
                with torch.cuda.device(dev):
                    stream = torch.cuda.current_stream(dev).cuda_stream
                    for lo in range(0, len(items), 16):
                        chunk = items[lo:lo + 16]
                        n = len(chunk)
                        arr = lambda vals: (ctypes.c_void_p * n)(*vals)
                        rc = lib.opnet_adam_multi_step_guarded_f32(
                            n, arr([p.data_ptr() for p, _, _ in chunk]), arr([g.data_ptr() for _, g, _ in chunk]),
                            arr([st["exp_avg"].data_ptr() for _, _, st in chunk]),
                            arr([st["exp_avg_sq"].data_ptr() for _, _, st in chunk]),
                            (ctypes.c_long * n)(*[p.numel() for p, _, _ in chunk]), float(group["lr"]), float(b1), float(b2),
                            float(group["eps"]), step_no, float(group["grad_scale"]), self.abort_ptr, self.loss_ptr,
                            self.guard_ptr, stream)
                        _lib.check(rc, "opnet_adam_multi_step_guarded_f32")
                # the update happened outside torch's view: bump the version counters so that consumers keyed on them
                # (the modules' packed-weight caches) see the parameters as modified
                for p, _, _ in items:
                    torch.autograd.graph.increment_version(p)
        return loss
