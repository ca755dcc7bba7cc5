"""Host checks of training from a carried state: the state validation of `model(boxes, state=...)` names the
offending operand, the new C entry points are declared, exported and refuse null pointers before anything is enqueued, and
`training.train_step` returns the loss alone without `state` and (loss, detached new state) with it.  No GPU work."""
import inspect

import pytest
import torch

H1, H2, B = 16, 32, 3


def _state(mlp=False, **over):
    s = {"h1": torch.zeros(1, B, H1), "c1": torch.zeros(1, B, H1),
         "h2": None if mlp else torch.zeros(1, B, H2), "c2": None if mlp else torch.zeros(1, B, H2)}
    s.update(over)
    return s["h1"], s["c1"], s["h2"], s["c2"]


def _check(state, mlp=False, device="cpu"):
    from objectpermanence_amd.learned_models import check_state
    return check_state(state, B, H1, H2, mlp, device)


def test_a_valid_state_passes():
    s = _state()
    assert _check(s) == s
    assert _check(list(s)) == s
    m = _state(mlp=True)
    assert _check(m, mlp=True) == m


@pytest.mark.parametrize("bad", [(), (torch.zeros(1, B, H1),) * 2, (torch.zeros(1, B, H1),) * 5, torch.zeros(4, 1, B, H1), None, "h1"])
def test_tuple_length(bad):
    with pytest.raises(ValueError, match=r"tuple \(h1, c1, h2, c2\)"):
        _check(bad)


@pytest.mark.parametrize("name,H", [("h1", H1), ("c1", H1), ("h2", H2), ("c2", H2)])
def test_refusals_name_the_operand(name, H):
    other = H2 if H == H1 else H1
    for shape in ((1, B, other), (1, B + 1, H), (B, H), (2, B, H), (B, 1, H)):
        with pytest.raises(ValueError, match=rf"{name} must be \[1, {B}, {H}\]"):
            _check(_state(**{name: torch.zeros(shape)}))
    for dtype in (torch.float64, torch.float16, torch.int32):
        with pytest.raises(TypeError, match=rf"{name} must be float32"):
            _check(_state(**{name: torch.zeros(1, B, H, dtype=dtype)}))
    with pytest.raises(TypeError, match=rf"{name} must be a tensor"):
        _check(_state(**{name: [[0.0] * H] * B}))
    on_meta = tuple(t.to("meta") for t in _state())
    assert _check(on_meta, device="meta") == on_meta
    with pytest.raises(ValueError, match=rf"{name} is on cpu, the model on meta"):
        _check(tuple(torch.zeros(1, B, H) if n == name else t for n, t in zip(("h1", "c1", "h2", "c2"), on_meta)), device="meta")
    with pytest.raises(ValueError, match=r"h1 is on cpu, the model on cuda:0"):
        _check(_state(), device="cuda:0")
    with pytest.raises(ValueError, match=rf"{name} is on meta"):
        _check(_state(**{name: torch.zeros(1, B, H, device="meta")}))


def test_video_state_must_match_the_model():
    for name in ("h2", "c2"):
        with pytest.raises(ValueError, match=rf"OPNet needs h2 and c2: {name} must be a tensor"):
            _check(_state(**{name: None}))
        with pytest.raises(ValueError, match=rf"OPNetLstmMlp has no video LSTM: {name} must be None"):
            _check(_state(mlp=True, **{name: torch.zeros(1, B, H2)}), mlp=True)
    for name in ("h1", "c1"):
        with pytest.raises(ValueError, match=rf"{name} must be a tensor, got None"):
            _check(_state(mlp=True, **{name: None}), mlp=True)


def test_forward_signatures_and_zero_state():
    from objectpermanence_amd import ModelsFactory
    cfg = {"object_to_track_pred_dim": 15, "object_to_track_hidden_dim": H1, "videos_hidden_dim": H2}
    for name in ("opnet", "opnet_lstm_mlp"):
        m = ModelsFactory.get_model(name, cfg)
        p = inspect.signature(m.forward).parameters
        assert list(p) == ["boxes", "logits_grad", "state", "return_state"]
        assert p["state"].default is None and p["return_state"].default is False
        s = m.zero_state(B)
        assert len(s) == 4 and s[0].shape == (1, B, H1) and s[1].shape == (1, B, H1) and not s[0].any() and not s[1].any()
        if name == "opnet":
            assert s[2].shape == (1, B, H2) and s[3].shape == (1, B, H2) and s[2].dtype == torch.float32
        else:
            assert s[2] is None and s[3] is None
        # boxes are checked before the state: there is still no CPU path
        with pytest.raises(RuntimeError, match="MI355X only"):
            m(torch.zeros(B, 2, 15, 6), state=s, return_state=True)


def test_entry_points_refuse_null_pointers():
    from objectpermanence_amd import _lib, build
    build.build()
    lib = _lib.load()
    for name in ("opnet_train_forward_state_f32", "opnet_train_backward_state_f32"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.opnet_train_forward_state_f32(None, None, None, None, None, 0, 1, 1, 16, 16, 0, None, None, None) == -1
    assert b"null pointer" in lib.opnet_last_error()
    assert lib.opnet_train_backward_state_f32(None, None, None, 0, None, None, None, None, None, None, 1, 1, 16, 16, 0,
                                              None, None, None, 0, None, None, None) == -1
    assert b"null pointer" in lib.opnet_last_error()


class _FakeOPNet(torch.nn.Module):
    """a double-output model with OPNet's calling convention on the CPU: y_t = w * (sum of the frame's boxes + h), h' = y_T"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(0.5))
        self.calls = []

    def zero_state(self, n):
        return torch.zeros(1, n, 1), torch.zeros(1, n, 1), None, None

    def forward(self, boxes, logits_grad=False, state=None, return_state=False):
        self.calls.append((state is not None, return_state))
        h = state[0][0] if state is not None else boxes.new_zeros(boxes.shape[0], 1)
        y = self.w * (boxes.sum(dim=(2, 3)).unsqueeze(-1) + h.unsqueeze(1)).expand(-1, -1, 4)
        logits = boxes.new_zeros(boxes.shape[0], 15, boxes.shape[1])
        if not return_state:
            return y, logits
        return y, logits, (y[:, -1, :1].unsqueeze(0), torch.zeros(1, boxes.shape[0], 1), None, None)


def test_train_step_return_type():
    from objectpermanence_amd.training import train_step
    # (opnet_no_labels: the one OPNet loss made of torch ops, so the step runs without a GPU)
    boxes, labels, mask = torch.ones(2, 3, 15, 6), torch.zeros(2, 3, 4), torch.ones(2, 3, 4)
    m = _FakeOPNet()
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    loss = train_step("opnet_no_labels", m, opt, boxes, labels, mask)
    assert isinstance(loss, torch.Tensor) and loss.dim() == 0
    assert m.calls == [(False, False)]                      # no state argument reaches a model that was not given one
    out = train_step("opnet_no_labels", m, opt, boxes, labels, mask, state=m.zero_state(2))
    assert isinstance(out, tuple) and len(out) == 2
    loss2, new_state = out
    assert isinstance(loss2, torch.Tensor) and loss2.dim() == 0
    assert isinstance(new_state, tuple) and len(new_state) == 4 and new_state[2] is None and new_state[3] is None
    assert new_state[0].shape == (1, 2, 1) and not new_state[0].requires_grad and not new_state[1].requires_grad
    assert float(new_state[0].abs().sum()) > 0
    assert m.calls[-1] == (True, True)
    # the returned state is the next chunk's argument
    loss3, _ = train_step("opnet_no_labels", m, opt, boxes, labels, mask, state=new_state)
    assert float(loss3) > float(loss2)


def test_train_step_refuses_state_for_stateless_models():
    from objectpermanence_amd.training import train_step
    m = torch.nn.Linear(1, 1)
    with pytest.raises(ValueError, match="takes no initial state"):
        train_step("baseline_lstm", m, torch.optim.SGD(m.parameters(), lr=1e-3), torch.zeros(1, 1, 15, 5),
                   torch.zeros(1, 1, 4), state=(None,) * 4)
