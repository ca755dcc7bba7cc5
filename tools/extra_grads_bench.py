"""Time an OPNet training step with and without the opt-in gradients.

Per batch size (300 frames, reference hidden sizes): device time (HIP events around a window of back-to-back steps) of
    plain      training.train_step as ever
    selection  ... with selection_targets (the logit gradient; the reverse recurrence runs on the launch chain)
    boxes      ... with boxes.requires_grad (the box gradient: opnet_dboxes)
    dboxes_us  opnet_dboxes alone (the library's event pair around its launch, profile tag 8) and the HBM rate that is for the
               da1 bytes it has to read (T x row blocks x 4 H1 x 32 clips x 4 B)
in --rounds alternating windows per variant; every window, the minimum and the spread (max - min) / min are reported.  A
build without the feature (the parent commit) reports `plain` only, so both commits are measured by this one script.
Prints one JSON object.

    python tools/extra_grads_bench.py [--batches 32,128] [--rounds 5] [--steps 20] [--out result.json]
"""
import argparse
import ctypes
import inspect
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import synth  # noqa: E402

CFG = {"object_to_track_pred_dim": 15, "object_to_track_hidden_dim": 256, "videos_hidden_dim": 512}
T = 300


def _window(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / steps


def _summary(windows):
    lo = min(windows)
    return {"windows_us": [round(w, 1) for w in windows], "min_us": round(lo, 1), "spread": round((max(windows) - lo) / lo, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,128")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("extra_grads_bench.py needs a ROCm device")
    from objectpermanence_amd import FusedAdam, ModelsFactory, _lib
    from objectpermanence_amd.training import train_step
    lib = _lib.load()
    feature = "selection_targets" in inspect.signature(train_step).parameters
    res = {"T": T, "feature": feature, "rounds": args.rounds, "steps_per_window": args.steps}
    for B in [int(b) for b in args.batches.split(",")]:
        boxes, labels = synth.make_batch(0, min(B, 32), T)
        reps = (B + boxes.shape[0] - 1) // boxes.shape[0]
        x = torch.from_numpy(np.tile(boxes, (reps, 1, 1, 1))[:B].copy()).cuda()
        lab = torch.from_numpy(np.tile(labels, (reps, 1, 1))[:B].copy()).cuda()
        xg = x.clone().requires_grad_()
        tg = torch.randint(0, 15, (B, T), device="cuda")
        m = ModelsFactory.get_model("opnet", CFG)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.opnet_synth_params(CFG).items()})
        m.to("cuda:0").train(True)
        opt = FusedAdam(m.parameters(), lr=1e-5)
        variants = {"plain": lambda: train_step("opnet", m, opt, x, lab)}
        if feature:
            variants["selection"] = lambda: train_step("opnet", m, opt, x, lab, selection_targets=tg)

            def with_boxes():
                xg.grad = None
                train_step("opnet", m, opt, xg, lab)
            variants["boxes"] = with_boxes
        for fn in variants.values():        # warm up every variant: workspaces, packed images, side streams
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        windows = {k: [] for k in variants}
        for _ in range(args.rounds):        # alternating windows: a drift of the clocks hits every variant alike
            for k, fn in variants.items():
                windows[k].append(_window(fn, args.steps))
        out = {k: _summary(w) for k, w in windows.items()}
        if feature:
            ms, n = ctypes.c_double(), ctypes.c_int()
            per_round = []
            for _ in range(args.rounds):
                lib.opnet_xcd_profile(1)
                for _ in range(args.steps):
                    variants["boxes"]()
                torch.cuda.synchronize()
                _lib.check(lib.opnet_kernel_profile_read(8, ctypes.byref(ms), ctypes.byref(n)), "opnet_kernel_profile_read")
                lib.opnet_xcd_profile(0)
                per_round.append(ms.value * 1e3 / max(n.value, 1))
            out["dboxes"] = _summary(per_round)
            da1_bytes = T * ((B + 31) // 32) * 4 * CFG["object_to_track_hidden_dim"] * 32 * 4
            out["dboxes"]["da1_mb"] = round(da1_bytes / 1e6, 1)
            out["dboxes"]["hbm_tb_s"] = round(da1_bytes / (out["dboxes"]["min_us"] * 1e-6) / 1e12, 3)
        res[f"B{B}"] = out
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
