"""Time an OPNet training step from a carried state against the plain step.

Device time (HIP events around a window of back-to-back steps, reference hidden sizes) of
    plain        training.train_step as ever, on the routes a plain step takes (B = 32: the persistent pair)
    plain_chain  ... with OPNET_XCD4=0 OPNET_XCD_TRAIN=0: forward and reverse recurrence on the launch chain, the routes
                 a stateful step takes
    state        train_step(..., state=s): one chunk of truncated BPTT, the state carried from window step to window step
                 (no gradient on the final state, none wanted for the initial one)
    state_grads  a hand-written step whose loss also weighs the final state and whose initial state requires grad: the seeds
                 of the reverse recurrence and d state on top
per (B, T) of --batches x --frames, in --rounds alternating windows per variant; every window, the minimum and the spread
(max - min) / min are reported.  --part plain measures `plain` alone at T = 300: run from a checkout of the parent commit too,
it is the figure that must not have moved (a build without the feature reports nothing else).  Prints one JSON object.

    python tools/state_train_bench.py [--part plain|state] [--batches 32,128] [--frames 300,64,16] [--rounds 3] [--steps 20]
                                      [--out result.json]
"""
import argparse
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
CHAIN_ENV = {"OPNET_XCD4": "0", "OPNET_XCD_TRAIN": "0"}


def _window(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / steps


def _summary(windows, T):
    lo = min(windows)
    return {"windows_us": [round(w, 1) for w in windows], "min_us": round(lo, 1), "spread": round((max(windows) - lo) / lo, 4),
            "us_per_frame": round(lo / T, 2)}


def _on_chain(fn):
    """fn with the persistent training launches switched off (the library reads the switches at every call)"""
    def run():
        os.environ.update(CHAIN_ENV)
        try:
            fn()
        finally:
            for k in CHAIN_ENV:
                del os.environ[k]
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="state", choices=["plain", "state"])
    ap.add_argument("--batches", default="32,128")
    ap.add_argument("--frames", default="300,64,16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20, help="steps per window at T = 300; shorter clips get proportionally more")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("state_train_bench.py needs a ROCm device")
    from objectpermanence_amd import FusedAdam, ModelsFactory
    from objectpermanence_amd.optim import loss_and_grad
    from objectpermanence_amd.training import train_step
    feature = "state" in inspect.signature(train_step).parameters
    if args.part == "state" and not feature:
        raise SystemExit("this build has no train_step(state=): run --part plain")
    frames = [300] if args.part == "plain" else [int(t) for t in args.frames.split(",")]
    res = {"part": args.part, "feature": feature, "rounds": args.rounds, "steps_per_window_at_300": args.steps}
    for B in [int(b) for b in args.batches.split(",")]:
        for T in frames:
            boxes, labels = synth.make_batch(0, min(B, 32), T)
            reps = (B + boxes.shape[0] - 1) // boxes.shape[0]
            x = torch.from_numpy(np.tile(boxes, (reps, 1, 1, 1))[:B].copy()).cuda()
            lab = torch.from_numpy(np.tile(labels, (reps, 1, 1))[:B].copy()).cuda()
            m = ModelsFactory.get_model("opnet", CFG)
            m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.opnet_synth_params(CFG).items()})
            m.to("cuda:0").train(True)
            opt = FusedAdam(m.parameters(), lr=1e-5)
            plain = lambda: train_step("opnet", m, opt, x, lab)
            variants = {"plain": plain}
            if args.part == "state":
                variants["plain_chain"] = _on_chain(plain)
                carried = [m.zero_state(B)]

                def chunk():
                    _, carried[0] = train_step("opnet", m, opt, x, lab, state=carried[0])
                variants["state"] = chunk
                r = tuple(torch.full_like(t, 1e-3) for t in m.zero_state(B))

                def with_grads():
                    opt.zero_grad(set_to_none=True)
                    s = tuple(t.detach().requires_grad_() for t in carried[0])
                    y, _, new = m(x, state=s, return_state=True)
                    _, dy = loss_and_grad(y, lab, 0.0)
                    torch.autograd.backward([y, *new], [dy, *r])
                    opt.step()
                variants["state_grads"] = with_grads
            steps = args.steps * max(1, 300 // T)
            for fn in variants.values():        # warm up every variant: workspaces, packed images, side streams
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            windows = {k: [] for k in variants}
            for _ in range(args.rounds):        # alternating windows: a drift of the clocks hits every variant alike
                for k, fn in variants.items():
                    windows[k].append(_window(fn, steps))
            res[f"B{B}_T{T}"] = {k: _summary(w, T) for k, w in windows.items()}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
