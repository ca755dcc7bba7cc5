"""GPU tests of the product-wave gather of the split-f16 persistent forward (csrc/opnet_xcd_split_kernels.hip): with four or more
16-clip groups on an XCD the product waves issue the LDS-DMA gather a finish wave has found ready (OPNET_XCD_PGATHER, default 1).
Who issues a load changes no arithmetic: every result here is held bit for bit - against the finish-wave gather
(OPNET_XCD_PGATHER=0), against digests recorded on the commit before the change (tests/golden/opnet_xcd_split_*.json), against
the write-through protocol and against itself.  `pytest -m gpu` on the MI355X box."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

REAL_CFG = {"object_to_track_pred_dim": 15, "object_to_track_hidden_dim": 256, "videos_hidden_dim": 512}
SEED = 21             # the seed of the recorded digests


@pytest.fixture(scope="module")
def model():
    from objectpermanence_amd import ModelsFactory
    m = ModelsFactory.get_model("opnet", REAL_CFG)
    params = synth.opnet_synth_params(REAL_CFG)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    m.eval()
    m.use_xcd = "1"
    return m.to("cuda:0")


def _run(m, boxes):
    with torch.no_grad():
        y, lg = m(torch.from_numpy(boxes).to("cuda:0"))
    torch.cuda.synchronize()
    for key, st in m.xcd_status().items():
        assert st[0] == 0, f"persistent launch {key} aborted: code {st[0]} block {st[1]} phase {st[2]}"
    return y.cpu().numpy(), lg.cpu().numpy()


_CACHE = {}


def _default(m, B, T):
    """the default build's y, logits on make_batch(SEED, B, T): computed once per shape, never modified"""
    if (B, T) not in _CACHE:
        boxes, _ = synth.make_batch(SEED, B, T)
        y, lg = _run(m, boxes)
        y.setflags(write=False)
        lg.setflags(write=False)
        _CACHE[(B, T)] = (boxes, y, lg)
    return _CACHE[(B, T)]


# (400, 40): XCD 0 carries four groups, the others three - both paths in one launch; its 160 phases make every CU of XCD 0 head CU and
# y CU more than once and wrap the 4-slot rings.  (512, 12): four groups everywhere; (640, 9): five; (1024, 5): eight.
# (130, 9): no XCD reaches four groups - the switch must change nothing.
@pytest.mark.parametrize("B,T", [(400, 40), (512, 12), (640, 9), (1024, 5), (130, 9)])
def test_product_wave_gather_equals_finish_wave_gather(monkeypatch, model, B, T):
    monkeypatch.delenv("OPNET_XCD_PGATHER", raising=False)
    boxes, y, lg = _default(model, B, T)
    monkeypatch.setenv("OPNET_XCD_PGATHER", "0")
    y0, lg0 = _run(model, boxes)
    assert np.isfinite(y).all()
    assert np.array_equal(y, y0) and np.array_equal(lg, lg0)


def test_product_wave_gather_equals_finish_wave_gather_full_history(monkeypatch):
    """OPNET_XCD_RING=0 (another workspace layout: a model of its own): full-history slots instead of the rings"""
    from objectpermanence_amd import ModelsFactory
    monkeypatch.setenv("OPNET_XCD_RING", "0")
    monkeypatch.delenv("OPNET_XCD_PGATHER", raising=False)
    m = ModelsFactory.get_model("opnet", REAL_CFG)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.opnet_synth_params(REAL_CFG).items()})
    m.eval()
    m.use_xcd = "1"
    m = m.to("cuda:0")
    boxes, _ = synth.make_batch(SEED, 512, 12)
    y, lg = _run(m, boxes)
    monkeypatch.setenv("OPNET_XCD_PGATHER", "0")
    y0, lg0 = _run(m, boxes)
    assert np.isfinite(y).all()
    assert np.array_equal(y, y0) and np.array_equal(lg, lg0)


@pytest.mark.parametrize("B,T", [(400, 40), (640, 9)])
def test_bits_are_the_parent_commits(monkeypatch, model, golden_dir, B, T):
    """the default build against the SHA-256 of y and of logits recorded before the product waves gathered"""
    monkeypatch.delenv("OPNET_XCD_PGATHER", raising=False)
    _, y, lg = _default(model, B, T)
    with open(os.path.join(golden_dir, f"opnet_xcd_split_{B}x{T}.json")) as f:
        want = json.load(f)
    assert hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest() == want["y_sha256"]
    assert hashlib.sha256(np.ascontiguousarray(lg).tobytes()).hexdigest() == want["logits_sha256"]


def test_write_through_protocol_gives_the_same_bits(monkeypatch, model):
    monkeypatch.delenv("OPNET_XCD_PGATHER", raising=False)
    boxes, y, lg = _default(model, 512, 12)
    monkeypatch.setenv("OPNET_XCD_SAFE", "1")
    y2, lg2 = _run(model, boxes)
    assert np.array_equal(y2, y) and np.array_equal(lg2, lg)


def test_product_wave_gather_is_deterministic(monkeypatch, model):
    monkeypatch.delenv("OPNET_XCD_PGATHER", raising=False)
    boxes, y, lg = _default(model, 512, 12)
    for _ in range(3):
        y2, lg2 = _run(model, boxes)
        assert np.array_equal(y2, y) and np.array_equal(lg2, lg)
