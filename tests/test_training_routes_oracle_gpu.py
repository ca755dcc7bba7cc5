"""The training routes built for the large shapes, against the fp64 port of the reference (oracle/torch_port.py evaluated on
the GPU) at the shapes they were built for:
  a. OPNet training steps of 48 .. 256 clips x 300 frames: the 4-clip persistent forward (<= 96 clips), the 16-clip persistent
     forward (97+), the reverse recurrence as 2 - 4 launch chains over slices of the batch (OPNET_BWD_SLICES);
  b. the stacked LSTM's reverse recurrence as one persistent launch (seqx_backward) at 32 and 37 clips x 300 frames;
  c. one encoder layer through its training ABI (opseq_encoder_layer_train_{forward,backward}_f32) at S = 300 / 4 800 / 9 600
     tokens: the flash attention with its routed, and forced, sweep splits and fragment counts, and the chunked form;
  d. whole transformer_lstm training steps at S = 4 800 / 9 600;
  e. a seeded cut of the randomised sweep of these routes (ragged batches, T = 1 / 2 / 13, short sequences).
Every tensor is held element-wise relative to max|ref| and in the Frobenius norm.  fp32 recurrence error grows with t, so these
are the shapes where a wrong slice boundary or a mis-ordered partial sum shows against a HIP form that shares it.

The FFN's ReLU is kept away from zero so that the gradients can be held element-wise (a pre-activation within rounding of zero
flips a hidden unit between fp32 and fp64): linear1.bias gets + c and linear2.bias - c * linear2.weight.sum(1), with c chosen from
the fp64 pre-activations so that every one of them is >= 0.5 after the shift (asserted).  The HIP step and the fp64 port both run
the shifted weights; the FFN then passes every unit, and linear2's bias takes the shift back out.  The slot embedding's
ReLU has no bias to shift: slot-0 boxes whose pre-activations come within 1e-4 of zero are nudged by < 1e-3 until none does
(asserted; an all-zero box gives exact zeros in either precision).

Worst errors measured on the MI355X (element-wise / max|ref|, Frobenius / |ref|_F; each bound below is at most
4x the worst measured under it):
  a. gradients 2.7e-6 / 1.4e-6, y 6.6e-7 / 3.0e-7, loss 8.2e-8 absolute
  b. gradients 2.7e-6 / 1.5e-6, y 9.2e-7 / 4.6e-7, loss 3.1e-8
  c. z_out 1.4e-5 / 1.0e-5 (S = 9 600 as one unsplit sweep, OPSEQ_ATTN_ZS=1), dz_in and gradients 5.9e-6 / 3.9e-6
  d. gradients 1.1e-5 / 7.3e-6 (video_LSTM.weight_hh_l0 at 32 clips), y 6.0e-6 / 3.2e-6, loss 1.2e-6
  e. transformer_lstm: gradients 1.1e-5 / 4.3e-6, y 2.6e-6 / 1.8e-6, loss 5.7e-7; OPNet: gradients 6.8e-7 / 3.4e-7, y 7.3e-7 / 5.3e-7"""
import ctypes

import numpy as np
import pytest

from oracle import synth

pytestmark = pytest.mark.gpu

REAL_CFG = {"object_to_track_pred_dim": 15, "object_to_track_hidden_dim": 256, "videos_hidden_dim": 512}
SEQ_CFG = {"baseline_lstm": {"videos_hidden_dim": 512},
           "non_linear_lstm": {"boxes_features_dim": 256, "videos_hidden_dim": 512}}
SEQ_PARAMS = {"baseline_lstm": synth.baseline_lstm_synth_params, "non_linear_lstm": synth.non_linear_lstm_synth_params}
PROF_XCD, PROF_ATTN_TF, PROF_ATTN_TB, PROF_SEQXB = 0, 5, 6, 7        # csrc/opnet_abi.hip


def _close(what, got, ref, elem, fro, floor=1e-3):
    """finite, then max|got - ref| <= elem * max|ref| and |got - ref|_F <= fro * |ref|_F (ref fp64)"""
    a, b = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == b.shape, what
    assert np.isfinite(a).all(), f"{what}: not finite"
    e = np.abs(a - b).max() / max(floor, np.abs(b).max())
    f = np.sqrt(((a - b) ** 2).sum()) / max(1e-12, np.sqrt((b ** 2).sum()))
    print(f"ERR {what}: elem {e:.3e} fro {f:.3e}")
    assert e <= elem, f"{what}: element-wise {e:.3e} > {elem:.1e} of max|ref|"
    assert f <= fro, f"{what}: Frobenius {f:.3e} > {fro:.1e}"


class _Profile:
    """launch counts of the profiled kernels (opnet_xcd_profile) over the block"""

    def __enter__(self):
        from objectpermanence_amd import _lib
        self.lib = _lib.load()
        _lib.check(self.lib.opnet_xcd_profile(1), "opnet_xcd_profile")
        return self

    def launches(self, tag):
        from objectpermanence_amd import _lib
        ms, n = ctypes.c_double(), ctypes.c_int()
        _lib.check(self.lib.opnet_kernel_profile_read(tag, ctypes.byref(ms), ctypes.byref(n)), "opnet_kernel_profile_read")
        return n.value

    def __exit__(self, *exc):
        self.lib.opnet_xcd_profile(0)


def _hip_step(name, cfg, params, x, labels, dropout=None):
    import torch
    from objectpermanence_amd import ModelsFactory, l1_mean
    m = ModelsFactory.get_model(name, cfg)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    m.to("cuda:0").train(True)
    if dropout is not None:
        m.dropout = dropout
    out = m(torch.from_numpy(x).cuda())
    y = out[0] if isinstance(out, tuple) else out
    loss = l1_mean(y, torch.from_numpy(labels).cuda())
    loss.backward()
    torch.cuda.synchronize()
    assert not m.training_step_aborted()
    return float(loss.detach()), y.detach().cpu().numpy(), {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}


# bounds (element-wise / max|ref|, Frobenius / |ref|_F): at most 4x the worst measured on the MI355X (module docstring); the loss
# within 2e-6 absolute throughout
RECURRENCE = dict(g_elem=1e-5, g_fro=5e-6, y_elem=4e-6, y_fro=2e-6)         # a, b, e (OPNet)
TRANSFORMER = dict(g_elem=4e-5, g_fro=2.5e-5, y_elem=2e-5, y_fro=1e-5)      # d, e (transformer_lstm)


def _check_step(what, hip, ref, g_elem, g_fro, y_elem, y_fro):
    loss, y, g = hip
    rloss, rg, ry = ref
    assert np.isfinite(loss) and abs(loss - rloss) <= 2e-6, (what, loss, rloss)
    print(f"ERR {what} loss: abs {abs(loss - rloss):.3e}")
    _close(f"{what} y", y, ry, y_elem, y_fro, floor=1.0)
    assert set(g) == set(rg)
    for k in rg:
        _close(f"{what} {k}", g[k], rg[k], g_elem, g_fro)


# ---- a. OPNet ------------------------------------------------------------------------------------------------------------------

_opnet_ref = {}


def _opnet_case(B, T, seed):
    import torch
    from oracle import torch_port
    p = synth.opnet_synth_params(REAL_CFG)
    boxes, labels = synth.make_batch(seed, B, T)
    key = (B, T, seed)
    if key not in _opnet_ref:
        _opnet_ref.clear()
        _opnet_ref[key] = torch_port.loss_and_grads(boxes, labels, p, dtype=torch.float64, device="cuda")
    return p, boxes, labels, _opnet_ref[key]


@pytest.mark.parametrize("B,slices", [(48, None), (64, None), (64, "2"), (128, None), (128, "4"), (160, None), (256, None),
                                      (256, "4")])
def test_opnet_training_step_at_300_frames(monkeypatch, B, slices):
    """48 / 64 clips: the 4-clip persistent forward; 128 / 160 / 256: the 16-clip persistent forward (160 = 5 row blocks of 32
    clips: routed to 3 slices of the reverse recurrence, a ragged cut); the reverse recurrence as 2 - 4 chains over slices"""
    if slices is not None:
        monkeypatch.setenv("OPNET_BWD_SLICES", slices)
    p, boxes, labels, ref = _opnet_case(B, 300, 3000 + B)
    with _Profile() as prof:
        hip = _hip_step("opnet", REAL_CFG, p, boxes, labels)
        if B >= 128:
            assert prof.launches(PROF_XCD) > 0, "the 16-clip persistent training forward did not run"
    _check_step(f"a B={B} slices={slices}", hip, ref, **RECURRENCE)


# ---- b. stacked LSTM reverse recurrence ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,B", [("baseline_lstm", 32), ("non_linear_lstm", 32), ("baseline_lstm", 37)])
def test_stacked_lstm_reverse_recurrence_at_300_frames(name, B):
    """32 clips = 8 4-clip groups, 37 = a ragged last group; one and two LSTM layers"""
    import torch
    from oracle import torch_port
    cfg = SEQ_CFG[name]
    p = SEQ_PARAMS[name](cfg)
    boxes, labels = synth.make_batch(4000 + B, B, 300)
    x = synth.boxes5(boxes)
    if name == "non_linear_lstm":
        x = _nudge_slot_embedding(x, p["boxes_linear.weight"], slots=15)
    with _Profile() as prof:
        hip = _hip_step(name, cfg, p, x, labels)
        assert prof.launches(PROF_SEQXB) > 0, "seqx_backward did not run"
    ref = torch_port.sibling_loss_and_grads(name, x, labels, p, dtype=torch.float64, device="cuda")
    _check_step(f"b {name} B={B}", hip, ref, **RECURRENCE)


# ---- ReLU margins -----------------------------------------------------------------------------------------------------------

def _nudge_slot_embedding(x, w, slots=1, eps=1e-4, seed=0):
    """x [B, T, 15, 5] with the first `slots` boxes moved (first four coordinates, by < 1e-3) wherever relu(box @ w.T) has a
    pre-activation within eps of zero; boxes of all zeros stay (their pre-activations are exact zeros in any precision)"""
    x = x.copy()
    rng = np.random.default_rng(seed)
    w64 = w.astype(np.float64)
    for _ in range(20):
        pre = x[:, :, :slots, :].astype(np.float64) @ w64.T
        live = np.abs(x[:, :, :slots, :]).sum(-1) > 0
        bad = live & (np.abs(pre) < eps).any(-1)
        if not bad.any():
            break
        idx = np.nonzero(bad)
        x[idx[0], idx[1], idx[2], :4] += rng.uniform(-1e-3, 1e-3, size=(len(idx[0]), 4)).astype(np.float32)
    pre = x[:, :, :slots, :].astype(np.float64) @ w64.T
    live = np.abs(x[:, :, :slots, :]).sum(-1) > 0
    assert not (live[..., None] & (np.abs(pre) < eps)).any(), "slot-embedding pre-activation within 1e-4 of zero"
    return x


def _shift_ffn_bias(p, prefix, z1):
    """p[prefix + linear1.bias] += c, p[prefix + linear2.bias] -= c * linear2.weight.sum(1) (fp32 params, in place), c from the
    fp64 FFN input z1 [S, E] (torch, cuda) so that every pre-activation is >= 0.5 afterwards (asserted)"""
    import torch
    w1 = torch.from_numpy(p[prefix + "linear1.weight"]).to(z1.device, torch.float64)
    b1 = torch.from_numpy(p[prefix + "linear1.bias"]).to(z1.device, torch.float64)
    c = max(0.0, 0.55 - float((z1 @ w1.t() + b1).min()))
    p[prefix + "linear1.bias"] = (p[prefix + "linear1.bias"].astype(np.float64) + c).astype(np.float32)
    p[prefix + "linear2.bias"] = (p[prefix + "linear2.bias"].astype(np.float64)
                                  - c * p[prefix + "linear2.weight"].astype(np.float64).sum(1)).astype(np.float32)
    b1 = torch.from_numpy(p[prefix + "linear1.bias"]).to(z1.device, torch.float64)
    assert float((z1 @ w1.t() + b1).min()) >= 0.5, "FFN pre-activation within 0.5 of zero after the shift"
    return c


def _prepare_transformer(p, x, nhead):
    """the bias shift of every encoder layer, each from the fp64 activations that reach it through the layers below it (already
    shifted), and the slot embedding's margin; returns the shifted params and the nudged x"""
    import torch
    from oracle import torch_port
    p = {k: v.copy() for k, v in p.items()}
    x = _nudge_slot_embedding(x, p["boxes_linear.weight"])
    with torch.no_grad():
        t = {k: torch.from_numpy(v).to("cuda", torch.float64) for k, v in p.items()}
        B, T = x.shape[:2]
        z = torch.relu(torch.from_numpy(x[:, :, 0, :]).to("cuda", torch.float64) @ t["boxes_linear.weight"].t()).reshape(B * T, -1)
        li = 0
        while f"attention_encoder.layers.{li}.linear1.weight" in p:
            pre = f"attention_encoder.layers.{li}."
            _shift_ffn_bias(p, pre, torch_port.encoder_attention_block(z, t, pre, nhead))
            t = {k: torch.from_numpy(v).to("cuda", torch.float64) for k, v in p.items()}
            z = torch_port.encoder_layer_forward(z, t, pre, nhead)
            li += 1
    return p, x


# ---- c. one encoder layer through the training ABI ------------------------------------------------------------------------------

ENC_KEYS = ["self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
            "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
            "norm2.bias"]
_enc_ref = {}


def _encoder_case(S, E, nhead):
    """layer-0 weights (FFN bias shifted), the slot embedding of S / 300 real clips as z_in, a random dz_out, and the fp64
    reference (z_out, dz_in, grads) - cached per shape across the routing variants"""
    import torch
    from oracle import torch_port
    key = (S, E, nhead)
    if key in _enc_ref:
        return _enc_ref[key]
    _enc_ref.clear()
    cfg = {"boxes_features_dim": E, "num_attention_heads": nhead, "num_attention_layers": 1, "num_lstm_layers": 1,
           "lstm_hidden_dim": 48}
    full = synth.transformer_lstm_synth_params(cfg)
    boxes, _ = synth.make_batch(5000 + S, S // 300, 300)
    x = synth.boxes5(boxes)
    emb = np.maximum(x[:, :, 0, :].reshape(S, 5) @ full["boxes_linear.weight"].T, 0).astype(np.float32)
    pre = "attention_encoder.layers.0."
    p = {pre + k: full[pre + k].copy() for k in ENC_KEYS}
    z64 = torch.from_numpy(emb).to("cuda", torch.float64)
    with torch.no_grad():
        t = {k: torch.from_numpy(v).to("cuda", torch.float64) for k, v in p.items()}
        _shift_ffn_bias(p, pre, torch_port.encoder_attention_block(z64, t, pre, nhead))
    g = torch.Generator().manual_seed(S + nhead)
    dz_out = torch.randn(S, E, generator=g, dtype=torch.float32).numpy()
    t = {k: torch.from_numpy(v).to("cuda", torch.float64).requires_grad_(True) for k, v in p.items()}
    zin = z64.clone().requires_grad_(True)
    out = torch_port.encoder_layer_forward(zin, t, pre, nhead)
    out.backward(torch.from_numpy(dz_out).to("cuda", torch.float64))
    ref = (out.detach().cpu().numpy(), zin.grad.cpu().numpy(), {k: t[pre + k].grad.cpu().numpy() for k in ENC_KEYS})
    del out, t, zin
    torch.cuda.empty_cache()
    _enc_ref[key] = (emb, dz_out, [p[pre + k] for k in ENC_KEYS], ref)
    return _enc_ref[key]


def _hip_encoder_layer(z_in, dz_out, weights, S, E, nhead, ffn=2048):
    import torch
    from objectpermanence_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    nsaved = lib.opseq_encoder_train_saved_bytes(S, E, nhead, ffn)
    nscr = lib.opseq_encoder_train_scratch_bytes(S, E, nhead, ffn)
    assert nsaved > 0 and nscr > 0
    saved = torch.empty(nsaved, dtype=torch.uint8, device=dev)
    scratch = torch.empty(nscr, dtype=torch.uint8, device=dev)
    w = [torch.from_numpy(a).to(dev) for a in weights]
    z = torch.from_numpy(z_in).to(dev)
    dz = torch.from_numpy(dz_out).to(dev)
    z_out, dz_in = torch.empty_like(z), torch.empty_like(z)
    grads = [torch.empty_like(a) for a in w]
    _lib.check(lib.opseq_encoder_layer_train_forward_f32(z.data_ptr(), z_out.data_ptr(), *(a.data_ptr() for a in w),
                                                         saved.data_ptr(), nsaved, scratch.data_ptr(), nscr, S, E, nhead, ffn,
                                                         0.0, 0, st), "opseq_encoder_layer_train_forward_f32")
    in_w, _, out_w, _, l1_w, _, l2_w, _, n1_w, _, n2_w, _ = w
    _lib.check(lib.opseq_encoder_layer_train_backward_f32(dz.data_ptr(), dz_in.data_ptr(), in_w.data_ptr(), out_w.data_ptr(),
                                                          l1_w.data_ptr(), l2_w.data_ptr(), n1_w.data_ptr(), n2_w.data_ptr(),
                                                          *(g.data_ptr() for g in grads), saved.data_ptr(), nsaved,
                                                          scratch.data_ptr(), nscr, S, E, nhead, ffn, 0.0, 0, st),
               "opseq_encoder_layer_train_backward_f32")
    torch.cuda.synchronize()
    return z_out.cpu().numpy(), dz_in.cpu().numpy(), {k: g.cpu().numpy() for k, g in zip(ENC_KEYS, grads)}


ENC_CASES = [(300, 2, {}), (300, 4, {}), (4800, 2, {}), (4800, 4, {}), (4800, 4, {"OPSEQ_ATTN_FLASH": "0"}),
             (9600, 2, {}), (9600, 2, {"OPSEQ_ATTN_ZS": "1"}), (9600, 2, {"OPSEQ_ATTN_ZS": "3"}),
             (9600, 4, {}), (9600, 4, {"OPSEQ_ATTN_ZS": "1"}), (9600, 4, {"OPSEQ_ATTN_ZS": "3"}), (9600, 4, {"OPSEQ_ATTN_AF": "1"})]


@pytest.mark.parametrize("S,nhead,env", ENC_CASES, ids=[f"S{s}-h{h}-" + ("-".join(f"{k}={v}" for k, v in e.items()) or "routed")
                                                         for s, h, e in ENC_CASES])
def test_encoder_layer_training_at_long_sequences(monkeypatch, S, nhead, env):
    """E = 256: head size 128 (2 heads) and 64 (4 heads, two stationary fragments per wave where routed); S = 4 800 / 9 600 route to
    split sweeps (attention_train_merge / attention_bwd_reduce); OPSEQ_ATTN_FLASH=0: the chunked form"""
    E = 256
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    z_in, dz_out, weights, (rz, rdz, rg) = _encoder_case(S, E, nhead)
    flash = env.get("OPSEQ_ATTN_FLASH") != "0"
    with _Profile() as prof:
        z_out, dz_in, g = _hip_encoder_layer(z_in, dz_out, weights, S, E, nhead)
        nf, nb = prof.launches(PROF_ATTN_TF), prof.launches(PROF_ATTN_TB)
    assert (nf > 0 and nb > 0) if flash else (nf == 0 and nb == 0), (nf, nb)
    what = f"c S={S} h={nhead} {env}"
    _close(f"{what} z_out", z_out, rz, 4e-5, 3e-5, floor=1.0)
    _close(f"{what} dz_in", dz_in, rdz, 2e-5, 1.5e-5)
    for k in ENC_KEYS:
        _close(f"{what} {k}", g[k], rg[k], 2e-5, 1.5e-5)


# ---- d. transformer_lstm whole training step -----------------------------------------------------------------------------------

def _transformer_case(what, B, T, nhead, seed, salt=0):
    import torch
    from oracle import torch_port
    cfg = {"boxes_features_dim": 256, "num_attention_heads": nhead, "num_attention_layers": 2, "num_lstm_layers": 2,
           "lstm_hidden_dim": 512}
    boxes, labels = synth.make_batch(seed, B, T)
    p, x = _prepare_transformer(synth.transformer_lstm_synth_params(cfg, salt=salt), synth.boxes5(boxes), nhead)
    hip = _hip_step("transformer_lstm", cfg, p, x, labels, dropout=0.0)
    ref = torch_port.sibling_loss_and_grads("transformer_lstm", x, labels, p, dtype=torch.float64, nhead=nhead, device="cuda")
    torch.cuda.empty_cache()
    _check_step(what, hip, ref, **TRANSFORMER)


@pytest.mark.parametrize("B,nhead", [(16, 2), (16, 4), (32, 2), (32, 4)])
def test_transformer_lstm_training_step_at_long_sequences(B, nhead):
    """16 / 32 clips x 300 frames: attention over S = 4 800 / 9 600 tokens, two encoder layers, two LSTM layers of 512"""
    _transformer_case(f"d B={B} h={nhead}", B, 300, nhead, 6000 + B)


# ---- e. a seeded cut of the randomised sweep -------------------------------------------------------------------------------------
# drawn once (numpy default_rng(141), the choice lists of the sweep) so that it holds the ragged 65 / 97 / 129 / 257 clips and
# T = 1 / 2 / 13; OPNet case i uses weights salt 100 + i and clips 7000 + i, transformer case i clips 9000 + i

FUZZ_OPNET = [(0, 97, 8), (1, 200, 13), (2, 257, 1), (3, 129, 2), (4, 65, 5), (5, 257, 5), (6, 40, 3)]
FUZZ_TRANSFORMER = [(0, 2, 7, 2), (1, 5, 100, 4), (2, 5, 100, 4)]


@pytest.mark.parametrize("case,B,T", FUZZ_OPNET)
def test_opnet_seeded_sweep_cut(case, B, T):
    import torch
    from oracle import torch_port
    p = synth.opnet_synth_params(REAL_CFG, salt=100 + case)
    boxes, labels = synth.make_batch(7000 + case, B, T)
    hip = _hip_step("opnet", REAL_CFG, p, boxes, labels)
    ref = torch_port.loss_and_grads(boxes, labels, p, dtype=torch.float64, device="cuda")
    _check_step(f"e opnet B={B} T={T}", hip, ref, **RECURRENCE)


@pytest.mark.parametrize("case,B,T,nhead", FUZZ_TRANSFORMER)
def test_transformer_lstm_seeded_sweep_cut(case, B, T, nhead):
    _transformer_case(f"e transformer B={B} T={T} h={nhead}", B, T, nhead, 9000 + case)


# ---- the port on the device ------------------------------------------------------------------------------------------------------

def test_fp64_port_on_the_device_equals_the_host_port():
    """the reference every test above compares with: the fp64 port on cuda against the fp64 port on the host (<= 1e-10 relative)"""
    import torch
    from oracle import torch_port

    def same(a, b):
        for k in b[1]:
            assert np.abs(a[1][k] - b[1][k]).max() <= 1e-10 * max(1e-30, np.abs(b[1][k]).max()), k
        assert np.abs(a[2] - b[2]).max() <= 1e-10 * np.abs(b[2]).max()
        assert abs(a[0] - b[0]) <= 1e-10 * abs(b[0])

    p = synth.opnet_synth_params(REAL_CFG)
    boxes, labels = synth.make_batch(8000, 3, 11)
    same(torch_port.loss_and_grads(boxes, labels, p, dtype=torch.float64, device="cuda"),
         torch_port.loss_and_grads(boxes, labels, p, dtype=torch.float64))
    cfg = {"boxes_features_dim": 64, "num_attention_heads": 4, "num_attention_layers": 2, "num_lstm_layers": 2,
           "lstm_hidden_dim": 48}
    p = synth.transformer_lstm_synth_params(cfg)
    boxes, labels = synth.make_batch(8100, 2, 13)
    x = synth.boxes5(boxes)
    same(torch_port.sibling_loss_and_grads("transformer_lstm", x, labels, p, dtype=torch.float64, nhead=4, device="cuda"),
         torch_port.sibling_loss_and_grads("transformer_lstm", x, labels, p, dtype=torch.float64, nhead=4))
