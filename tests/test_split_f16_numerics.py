"""CPU check of the split-f16 arithmetic of csrc/opnet_xcd_split_kernels.hip before any GPU is involved: the whole 300-step
OPNet forward with every matrix operand - weights, x, h1, h2, frames_boxes - replaced at every step by

    hi = RN_f16(a),  lo = RN_f16((a - float(hi)) * 2^11),   a . b ~ hi_a . hi_b + 2^-11 (hi_a . lo_b + lo_a . hi_b)

(fp32 accumulation, numpy's summation order - the MFMA's internal order is not emulated, the GPU tests decide that half)
against the fp64 oracle.  The bound is half of the project's TOL_Y / TOL_LOGITS; the other half is left to the GPU's order.
A three-term bf16 split (16 significant bits instead of 22) must NOT pass TOL_Y: nobody should swap it in."""
import numpy as np

from oracle import opnet_oracle as oo
from oracle import synth

REAL_CFG = {"object_to_track_pred_dim": 15, "object_to_track_hidden_dim": 256, "videos_hidden_dim": 512}
TOL_Y = 2e-5
TOL_LOGITS = 1e-4
B, T = 4, 300


def _rn_bf16(a):
    u = a.astype(np.float32).view(np.uint32)
    u = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return u.view(np.float32)


def _split_f16(a):
    hi = a.astype(np.float16).astype(np.float32)
    lo = ((a - hi) * np.float32(2048.0)).astype(np.float16).astype(np.float32)
    return hi, lo, np.float32(1.0 / 2048.0)


def _split_bf16(a):
    hi = _rn_bf16(a)
    return hi, _rn_bf16(a - hi), np.float32(1.0)


def _sigmoid(x):
    return np.float32(1.0) / (np.float32(1.0) + np.exp(-x))


def _forward(boxes, p, split):
    """oracle.opnet_oracle.opnet_forward in fp32 with split products; weights are split once, activations at every step"""
    f32 = np.float32
    W = {k: split(np.ascontiguousarray(v.astype(f32).T)) for k, v in p.items()}      # [K][N] planes

    def prod(a, name):
        ah, al, sc = split(a)
        wh, wl, _ = W[name]
        main = ah @ wh
        corr = ah @ wl + al @ wh
        return (main + corr * sc).astype(f32)

    def cell(g, c, H):
        i, f, gg, o = _sigmoid(g[:, :H]), _sigmoid(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sigmoid(g[:, 3 * H:])
        c = (f * c + i * gg).astype(f32)
        return (o * np.tanh(c)).astype(f32), c

    n, t_frames = boxes.shape[:2]
    x = boxes.astype(f32)
    h1, c1 = np.zeros((n, 256), f32), np.zeros((n, 256), f32)
    h2, c2 = np.zeros((n, 512), f32), np.zeros((n, 512), f32)
    y, logits = np.empty((n, t_frames, 4), f32), np.empty((n, 15, t_frames), f32)
    for t in range(t_frames):
        g1 = prod(x[:, t].reshape(n, 90), "object_to_track_LSTM.weight_ih_l0") + prod(h1, "object_to_track_LSTM.weight_hh_l0")
        h1, c1 = cell(g1, c1, 256)
        lg = prod(h1, "object_to_track_prediction.weight")
        e = np.exp(lg - lg.max(axis=-1, keepdims=True))
        pr = (e / e.sum(axis=-1, keepdims=True)).astype(f32)
        fb = np.einsum("not,no->nt", x[:, t], pr).astype(f32)          # exact fp32 in the kernel too
        g2 = prod(h2, "video_LSTM.weight_hh_l0") + prod(fb, "video_LSTM.weight_ih_l0")
        h2, c2 = cell(g2, c2, 512)
        y[:, t] = prod(h2, "prediction_layer.weight")
        logits[:, :, t] = lg
    return y, logits


def _case():
    boxes, _ = synth.make_batch(0, B, T)
    params = synth.opnet_synth_params(REAL_CFG)
    y_ref, lg_ref = oo.opnet_forward(boxes, params, dtype=np.float64)
    return boxes, params, y_ref, lg_ref


def test_split_f16_forward_stays_within_half_the_tolerance():
    boxes, params, y_ref, lg_ref = _case()
    y, lg = _forward(boxes, params, _split_f16)
    err_y, err_lg = np.abs(y - y_ref).max(), np.abs(lg - lg_ref).max()
    print(f"split f16: max|dy| {err_y:.2e} max|dlogits| {err_lg:.2e}")
    assert err_y < 1e-5
    assert err_lg < 5e-5


def test_three_term_bf16_split_is_not_enough():
    boxes, params, y_ref, _ = _case()
    y, _ = _forward(boxes, params, _split_bf16)
    err_y = np.abs(y - y_ref).max()
    print(f"split bf16: max|dy| {err_y:.2e}")
    assert err_y > TOL_Y
