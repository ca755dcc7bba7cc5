"""The steady-state instantiation of the split-f16 persistent forward (csrc/opnet_xcd_split_kernels.hip, opnet_xcd_forward_split<true, .>):
what a launch with four or more 16-clip groups on every XCD runs by default - ring layout, product-wave gather, no debug bit compiled
in, a leaner finish loop.  It removes instructions, never arithmetic: every result here is held bit for bit against the general
kernel (OPNET_XCD_STEADY=0), against digests recorded on an earlier commit, against the write-through protocol and against itself;
plus the fp64 oracle, the host's routing (no GPU) and the range refusal on the steady route.  `pytest -m gpu` on the MI355X box."""
import hashlib
import json
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import opnet_oracle as oo
from oracle import synth

gpu = pytest.mark.gpu

REAL_CFG = {"object_to_track_pred_dim": 15, "object_to_track_hidden_dim": 256, "videos_hidden_dim": 512}
SEED = 21             # the seed of the recorded digests (tests/golden/opnet_xcd_split_*.json)
TOL_Y = 2e-5          # as tests/test_opnet_xcd_split_gpu.py
TOL_LOGITS = 1e-4
ABORT_RANGE = 3
XCD_COUNT = 8


def _groups_per_xcd(B):
    """xcd_groups of csrc/opnet_xcd_kernels.hip: the 16-clip groups of a B-clip launch, split evenly over the XCDs, the first ones
    taking the remainder"""
    ngt = (B + 15) // 16
    return [ngt // XCD_COUNT + (1 if x < ngt % XCD_COUNT else 0) for x in range(XCD_COUNT)]


def _boundary():
    """the largest B that leaves some XCD with three groups; at B + 1 every XCD carries four"""
    B = max(b for b in range(1, 1025) if min(_groups_per_xcd(b)) == 3)
    assert min(_groups_per_xcd(B + 1)) == 4
    return B


def _lib():
    from objectpermanence_amd import _lib, build
    build.build()
    return _lib.load()


def test_routing_host_only(monkeypatch):
    for name in ("OPNET_XCD_STEADY", "OPNET_XCD_PGATHER", "OPNET_XCD_RING", "OPNET_XCD_DEBUG", "OPNET_XCD_SPLIT", "OPNET_XCD_HO"):
        monkeypatch.delenv(name, raising=False)
    lib = _lib()
    B = _boundary()
    assert lib.opnet_xcd_steady_form(B, 5) == 0
    assert lib.opnet_xcd_steady_form(B + 1, 5) == 1
    assert lib.opnet_xcd_steady_form(1024, 300) == 1
    for name, value in (("OPNET_XCD_STEADY", "0"), ("OPNET_XCD_PGATHER", "0"), ("OPNET_XCD_RING", "0"), ("OPNET_XCD_DEBUG", "1")):
        monkeypatch.setenv(name, value)
        assert lib.opnet_xcd_steady_form(B + 1, 5) == 0, name
        monkeypatch.delenv(name)
        assert lib.opnet_xcd_steady_form(B + 1, 5) == 1


def _new_model(xcd="1"):
    from objectpermanence_amd import ModelsFactory
    m = ModelsFactory.get_model("opnet", REAL_CFG)
    params = synth.opnet_synth_params(REAL_CFG)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    m.eval()
    m.use_xcd = xcd
    return m.to("cuda:0"), params


@pytest.fixture(scope="module")
def model():
    return _new_model()[0]


def _run(m, boxes):
    with torch.no_grad():
        y, lg = m(torch.from_numpy(boxes).to("cuda:0"))
    torch.cuda.synchronize()
    for key, st in m.xcd_status().items():
        assert st[0] == 0, f"persistent launch {key} aborted: code {st[0]} block {st[1]} phase {st[2]}"
    return y, lg


_CACHE = {}


def _steady(monkeypatch, m, B, T):
    """the steady kernel's y, logits on make_batch(SEED, B, T): computed once per shape, never modified"""
    for name in ("OPNET_XCD_STEADY", "OPNET_XCD_SAFE"):
        monkeypatch.delenv(name, raising=False)
    assert _lib().opnet_xcd_steady_form(B, T) == 1
    if (B, T) not in _CACHE:
        boxes, _ = synth.make_batch(SEED, B, T)
        y, lg = _run(m, boxes)
        _CACHE[(B, T)] = (boxes, y, lg)
    return _CACHE[(B, T)]


# boundary + 1 (497): four groups on every XCD, the last group holds one clip.  512 x 1 / 2 / 3: the output head's extra phases and
# fp + 3 < nph at its edges.  640: five groups.  1024: eight (XCD_NGMAX).  1000: XCDs with eight and with seven groups.
@gpu
@pytest.mark.parametrize("B,T", [(None, 5), (512, 1), (512, 2), (512, 3), (640, 9), (1024, 4), (1000, 7)])
def test_steady_equals_general(monkeypatch, model, B, T):
    B = _boundary() + 1 if B is None else B
    boxes, y, lg = _steady(monkeypatch, model, B, T)
    monkeypatch.setenv("OPNET_XCD_STEADY", "0")
    assert _lib().opnet_xcd_steady_form(B, T) == 0
    y0, lg0 = _run(model, boxes)
    assert torch.isfinite(y).all()
    assert torch.equal(y, y0) and torch.equal(lg, lg0)


@gpu
def test_bits_are_an_earlier_commits(monkeypatch, model, golden_dir):
    _, y, lg = _steady(monkeypatch, model, 640, 9)
    with open(os.path.join(golden_dir, "opnet_xcd_split_640x9.json")) as f:
        want = json.load(f)
    assert hashlib.sha256(np.ascontiguousarray(y.cpu().numpy()).tobytes()).hexdigest() == want["y_sha256"]
    assert hashlib.sha256(np.ascontiguousarray(lg.cpu().numpy()).tobytes()).hexdigest() == want["logits_sha256"]


@gpu
def test_write_through_protocol_gives_the_same_bits(monkeypatch, model):
    boxes, y, lg = _steady(monkeypatch, model, 512, 5)
    monkeypatch.setenv("OPNET_XCD_SAFE", "1")
    assert _lib().opnet_xcd_steady_form(512, 5) == 1
    y2, lg2 = _run(model, boxes)
    assert torch.equal(y2, y) and torch.equal(lg2, lg)


@gpu
def test_run_to_run(monkeypatch, model):
    boxes, y, lg = _steady(monkeypatch, model, 640, 9)
    y2, lg2 = _run(model, boxes)
    assert torch.equal(y2, y) and torch.equal(lg2, lg)


@gpu
def test_steady_matches_fp64_oracle(monkeypatch):
    for name in ("OPNET_XCD_STEADY", "OPNET_XCD_SAFE"):
        monkeypatch.delenv(name, raising=False)
    assert _lib().opnet_xcd_steady_form(512, 6) == 1
    boxes, _ = synth.make_batch(200, 512, 6)
    m, params = _new_model()
    y, lg = _run(m, boxes)
    y, lg = y.cpu().numpy(), lg.cpu().numpy()
    y_ref, lg_ref = oo.opnet_forward(boxes, params, dtype=np.float64)
    print(f"steady vs fp64: |dy| {np.abs(y - y_ref).max():.2e} |dlg| {np.abs(lg - lg_ref).max():.2e}")
    assert np.isfinite(y).all()
    assert np.abs(y - y_ref).max() < TOL_Y
    assert np.abs(lg - lg_ref).max() < TOL_LOGITS


@gpu
def test_value_out_of_f16_range_is_refused_on_the_steady_route_and_healed_on_the_chain(monkeypatch):
    for name in ("OPNET_XCD_STEADY", "OPNET_XCD_SAFE"):
        monkeypatch.delenv(name, raising=False)
    assert _lib().opnet_xcd_steady_form(512, 3) == 1
    boxes, _ = synth.make_batch(11, 512, 3)
    boxes[300, 1, 2, 1] = 2.0 ** 15
    m, _ = _new_model()
    with torch.no_grad():
        y, lg = m(torch.from_numpy(boxes).to("cuda:0"))
    torch.cuda.synchronize()
    st = next(iter(m.xcd_status().values()))
    assert st[0] == ABORT_RANGE
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")             # (the monitor warns about the first healed launch of a process)
        assert m.verify_launches() == 1
    m0, _ = _new_model(xcd="0")
    with torch.no_grad():
        y0, lg0 = m0(torch.from_numpy(boxes).to("cuda:0"))
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and torch.equal(lg, lg0)
