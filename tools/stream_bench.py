"""Time the stateful OPNet streams (objectpermanence_amd/streaming.py) against whole-clip forwards.

For n streams in {1, 32, 256} and k frames a call in {1, 8, 300}: device time per call (HIP events around a window of
back-to-back calls, divided by their count) and host time per call (the enqueue loop, without the synchronise).  Against
that, the whole-clip forward of the same n clips x 300 frames through the launch chain (use_xcd = "0") and through the
default engine: that forward is also what "recompute the prefix each frame" costs for one new output at t = 300, so
prefix_speedup = (default-engine forward at T = 300) / (one k = 1 stream call).  abi_k1: the one-frame call through the
C ABI with its buffers prepared, i.e. without OPNetStreams' per-call Python work.  Prints one JSON object.

--model baseline_lstm / non_linear_lstm times LstmStackStreams the same way (H = 512; NonLinearLstm F = 256).  For
non_linear_lstm it also times the hoisted input product alone through both routes in the same run (the skinny kernel and
the tiled GEMM + repack, alternating windows; HIP events around opseq_stream_input_product_f32), at n x k from one stream to
32 x 32 rows, small n with large k included.

--ragged times one tick of n streams whose new frame counts cycle 1, 2, 3, for OPNet, BaselineLstm and
NonLinearLstm: one ragged call (host lengths, and an int32 device tensor), the same tick as three grouped uniform calls
(one per k, each over the streams with that many frames), and a uniform call of k = 3 over all n.  device_us: HIP events
around the window; wall_us: the window's wall time to the last call's completion, per call.

--engine persistent times the pool's persistent engine (one persistent launch a call: OPNetStreams, DESIGN.md 12e;
LstmStackStreams for --model baseline_lstm / non_linear_lstm) in place of the launch chain; --engine both times the two in alternating windows (--rounds of them each) and reports every window, the minimum and
the spread, per (n, k): stream_k{k} then holds {"chain": ..., "persistent": ..., "persistent_over_chain": ...}.

    python tools/stream_bench.py [--model opnet] [--ns 1,32,256] [--ks 1,8,300] [--engine chain] [--out result.json]
    python tools/stream_bench.py --ragged [--ns 1,32,256] [--out result.json]
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import synth  # noqa: E402

CFG = {"object_to_track_pred_dim": 15, "object_to_track_hidden_dim": 256, "videos_hidden_dim": 512}
T = 300


def _time(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    start.record()
    for _ in range(calls):
        fn()
    host = time.perf_counter() - t0
    end.record()
    end.synchronize()
    wall = time.perf_counter() - t0
    return {"device_us": round(start.elapsed_time(end) * 1e3 / calls, 2), "host_us": round(host * 1e6 / calls, 2),
            "wall_us": round(wall * 1e6 / calls, 2), "calls": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="opnet", choices=["opnet", "baseline_lstm", "non_linear_lstm"])
    ap.add_argument("--ns", default="1,32,256")
    ap.add_argument("--ks", default="1,8,300")
    ap.add_argument("--out", default=None)
    ap.add_argument("--engine", default="chain", choices=["chain", "persistent", "both"], help="the stream pool's engine")
    ap.add_argument("--rounds", type=int, default=3, help="--engine both: alternating windows per engine")
    ap.add_argument("--ragged", action="store_true", help="time ragged ticks (lengths 1, 2, 3) for all three models")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench.py needs a ROCm device")
    if args.ragged:
        res = bench_ragged(args)
    else:
        res = bench_opnet(args) if args.model == "opnet" else bench_stack(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def bench_opnet(args):
    from objectpermanence_amd import ModelsFactory, OPNetStreams, _lib
    dev = "cuda:0"
    m = ModelsFactory.get_model("opnet", CFG)
    params = synth.opnet_synth_params(CFG)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    m.eval().to(dev)
    ns = [int(v) for v in args.ns.split(",")]
    ks = [int(v) for v in args.ks.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "H1": 256, "H2": 512, "T_whole_clip": T, "rows": []}
    for n in ns:
        boxes = torch.from_numpy(synth.make_batch(0, n, T)[0]).to(dev)
        row = {"n": n}
        with torch.no_grad():
            m.use_xcd = "0"
            row["whole_clip_chain"] = _time(lambda: m(boxes), 5, warmup=2)
            m.use_xcd = "auto"
            row["whole_clip_default"] = _time(lambda: m(boxes), 5, warmup=2)
        m.verify_launches()
        streams = OPNetStreams(m, capacity=n)
        ids = streams.open(n)
        for k in ks:
            x = boxes[:, :k].contiguous()
            calls = max(5, min(200, 1200 // k))
            if args.engine == "both":
                row[f"stream_k{k}"] = _alternate(streams, ids, x, calls, args.rounds)
                continue
            row[f"stream_k{k}"] = _time(lambda: streams.step(ids, x, engine=args.engine), calls)
            row[f"stream_k{k}"]["device_us_per_frame"] = round(row[f"stream_k{k}"]["device_us"] / k, 2)
            row["launches_gave_up"] = row.get("launches_gave_up", 0) + streams.verify_launches()
        # the same one-frame call straight through the C ABI with every buffer prepared: the kernels' cost without the
        # Python checks, the slot upload and the output allocations of OPNetStreams.step
        lib = _lib.load()
        x1 = boxes[:, :1].contiguous()
        slots = torch.tensor(ids, dtype=torch.int32, device=dev)
        y1 = torch.empty((n, 1, 4), device=dev)
        lg1 = torch.empty((n, 15, 1), device=dev)
        ws = torch.empty(lib.opnet_stream_workspace_bytes(n, 1, 256, 512), dtype=torch.uint8, device=dev)
        packed = m._packed_weights(torch.device(dev))
        stream = torch.cuda.current_stream().cuda_stream

        def abi_call():
            _lib.check(lib.opnet_stream_step_f32(x1.data_ptr(), slots.data_ptr(), streams.state.data_ptr(), packed.data_ptr(),
                                                 y1.data_ptr(), lg1.data_ptr(), ws.data_ptr(), ws.numel(), n, 1, n, 256, 512, 0,
                                                 stream), "opnet_stream_step_f32")
        row["abi_k1"] = _time(abi_call, 200)
        if 300 in ks and args.engine != "both":
            row["k300_over_chain"] = round(row["stream_k300"]["device_us"] / row["whole_clip_chain"]["device_us"], 3)
        if 1 in ks and args.engine != "both":
            row["prefix_speedup_at_t300"] = round(row["whole_clip_default"]["device_us"] / row["stream_k1"]["device_us"], 1)
            row["prefix_speedup_vs_chain_at_t300"] = round(row["whole_clip_chain"]["device_us"] / row["stream_k1"]["device_us"], 1)
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return res


def _alternate(streams, ids, x, calls, rounds):
    """chain and persistent steps of the same call in alternating windows: every window's device time per call, the minimum
    and the spread (max - min) / min per engine"""
    windows = {"chain": [], "persistent": []}
    gave_up = 0
    for _ in range(rounds):
        for engine in ("chain", "persistent"):
            windows[engine].append(_time(lambda: streams.step(ids, x, engine=engine), calls)["device_us"])
            gave_up += streams.verify_launches()
    out = {"calls": calls, "launches_gave_up": gave_up}
    for engine, w in windows.items():
        out[engine] = {"device_us": min(w), "spread": round((max(w) - min(w)) / min(w), 3), "windows": w}
    out["persistent_over_chain"] = round(out["persistent"]["device_us"] / out["chain"]["device_us"], 3)
    return out


STACK_CFG = {"baseline_lstm": {"videos_hidden_dim": 512},
             "non_linear_lstm": {"boxes_features_dim": 256, "videos_hidden_dim": 512}}
STACK_PARAMS = {"baseline_lstm": synth.baseline_lstm_synth_params, "non_linear_lstm": synth.non_linear_lstm_synth_params}


def bench_stack(args):
    from objectpermanence_amd import LstmStackStreams, ModelsFactory, _lib
    dev = "cuda:0"
    cfg = STACK_CFG[args.model]
    m = ModelsFactory.get_model(args.model, cfg)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in STACK_PARAMS[args.model](cfg).items()})
    m.eval().to(dev)
    r = m._runner
    L, KX, H = r.L, r.KX, r.H
    ns = [int(v) for v in args.ns.split(",")]
    ks = [int(v) for v in args.ks.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "model": args.model, "L": L, "KX": KX, "H": H, "T_whole_clip": T,
           "rows": []}
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    for n in ns:
        x5 = torch.from_numpy(synth.boxes5(synth.make_batch(0, n, T)[0])).to(dev)
        row = {"n": n}
        with torch.no_grad():
            r.use_xcd = "0"
            row["whole_clip_chain"] = _time(lambda: m(x5), 5, warmup=2)
            r.use_xcd = "auto"
            row["whole_clip_default"] = _time(lambda: m(x5), 5, warmup=2)
            row["whole_clip_default_engine"] = r.engine(n, T)
        r._monitor.verify()
        streams = LstmStackStreams(m, capacity=n)
        ids = streams.open(n)
        for k in ks:
            x = x5[:, :k].contiguous()
            calls = max(5, min(200, 1200 // k))
            if args.engine == "both":
                row[f"stream_k{k}"] = _alternate(streams, ids, x, calls, args.rounds)
                continue
            row[f"stream_k{k}"] = _time(lambda: streams.step(ids, x, engine=args.engine), calls)
            row[f"stream_k{k}"]["device_us_per_frame"] = round(row[f"stream_k{k}"]["device_us"] / k, 2)
            row["launches_gave_up"] = row.get("launches_gave_up", 0) + streams.verify_launches()
        # the one-frame call straight through the C ABI with every buffer prepared (NonLinearLstm: its layer-0 input already
        # embedded): the LSTM's kernels without the Python work of LstmStackStreams.step
        if 1 in ks:
            feats = torch.randn((n, 1, KX), device=dev).abs()
            slots = torch.tensor(ids, dtype=torch.int32, device=dev)
            y1 = torch.empty((n, 1, 4), device=dev)
            ws = torch.empty(lib.opseq_stream_workspace_bytes(n, 1, L, KX, H), dtype=torch.uint8, device=dev)
            packed = r._packed_weights(r.weights(m.video_LSTM, m.predictions_layer), torch.device(dev), stream)

            def abi_call():
                _lib.check(lib.opseq_stream_step_f32(feats.data_ptr(), slots.data_ptr(), streams.state.data_ptr(),
                                                     packed.data_ptr(), y1.data_ptr(), ws.data_ptr(), ws.numel(), n, 1, n, L, KX,
                                                     H, stream), "opseq_stream_step_f32")
            row["abi_k1"] = _time(abi_call, 200)
        if 300 in ks and args.engine != "both":
            row["k300_over_chain"] = round(row["stream_k300"]["device_us"] / row["whole_clip_chain"]["device_us"], 3)
        if 1 in ks and args.engine != "both":
            row["prefix_speedup_at_t300"] = round(row["whole_clip_default"]["device_us"] / row["stream_k1"]["device_us"], 1)
            row["prefix_speedup_vs_chain_at_t300"] = round(row["whole_clip_chain"]["device_us"] / row["stream_k1"]["device_us"], 1)
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    if args.model == "non_linear_lstm" and args.engine == "chain":
        res["input_product"] = bench_input_product(m, dev)
    return res


PRODUCT_SHAPES = [(1, 1), (32, 1), (1, 32), (32, 8), (32, 16), (1, 300), (5, 64), (32, 32), (256, 1)]


def bench_input_product(m, dev, rounds=4):
    """the hoisted layer-0 input product alone (opseq_stream_input_product_f32): the skinny kernel against the tiled GEMM +
    repack at n streams x k frames, in alternating windows of 50 launches; rows_skinny = the k * ceil(n / 16) * 16 rows the
    skinny kernel computes (what the router compares with OPSEQ_STREAM_SKINNY_MAX_ROWS)"""
    from objectpermanence_amd import _lib
    lib = _lib.load()
    r = m._runner
    L, KX, H = r.L, r.KX, r.H
    stream = torch.cuda.current_stream().cuda_stream
    packed = r._packed_weights(r.weights(m.video_LSTM, m.predictions_layer), torch.device(dev), stream)
    out = []
    for n, k in PRODUCT_SHAPES:
        x = torch.rand((n, k, KX), device=dev)
        xg = torch.empty((k, (n + 31) // 32, H, 32, 4), device=dev)
        ws = torch.empty(lib.opseq_stream_workspace_bytes(n, k, L, KX, H), dtype=torch.uint8, device=dev)

        def product(route):
            _lib.check(lib.opseq_stream_input_product_f32(x.data_ptr(), packed.data_ptr(), xg.data_ptr(), ws.data_ptr(),
                                                          ws.numel(), n, k, L, KX, H, route, stream),
                       "opseq_stream_input_product_f32")
        times = {"skinny": [], "tiled": []}
        for _ in range(rounds):
            for route, code in (("skinny", 1), ("tiled", 2)):
                times[route].append(_time(lambda: product(code), 50)["device_us"])
        skinny, tiled = min(times["skinny"]), min(times["tiled"])
        out.append({"n": n, "k": k, "rows": n * k, "rows_skinny": k * ((n + 15) // 16) * 16, "skinny_us": skinny,
                    "tiled_us": tiled, "tiled_over_skinny": round(tiled / skinny, 2), "windows": times})
        print(json.dumps(out[-1]), file=sys.stderr, flush=True)
    return out


def bench_ragged(args, calls=100):
    import numpy as np
    from objectpermanence_amd import LstmStackStreams, ModelsFactory, OPNetStreams
    dev = "cuda:0"
    ns = [int(v) for v in args.ns.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "lengths": "1,2,3 cycling", "models": {}}
    for name in ("opnet", "baseline_lstm", "non_linear_lstm"):
        cfg = CFG if name == "opnet" else STACK_CFG[name]
        m = ModelsFactory.get_model(name, cfg)
        params = synth.opnet_synth_params(cfg) if name == "opnet" else STACK_PARAMS[name](cfg)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
        m.eval().to(dev)
        rows = []
        for n in ns:
            boxes = synth.make_batch(0, n, 3)[0]
            x = torch.from_numpy(boxes if name == "opnet" else synth.boxes5(boxes)).to(dev)
            pool = OPNetStreams(m, capacity=n) if name == "opnet" else LstmStackStreams(m, capacity=n)
            ids = pool.open(n)
            lens = np.arange(n, dtype=np.int32) % 3 + 1
            lens_dev = torch.from_numpy(lens).to(dev)
            groups = [([ids[i] for i in np.flatnonzero(lens == k)], x[torch.from_numpy(np.flatnonzero(lens == k)).to(dev), :k]
                       .contiguous(), k) for k in (1, 2, 3) if (lens == k).any()]

            def grouped():
                for gids, gx, _ in groups:
                    pool.step(gids, gx)
            row = {"n": n,
                   "ragged": _time(lambda: pool.step(ids, x, lens), calls),
                   "ragged_device_lengths": _time(lambda: pool.step(ids, x, lens_dev), calls),
                   "grouped_3_calls": _time(grouped, calls),
                   "uniform_k3": _time(lambda: pool.step(ids, x), calls)}
            row["ragged_over_uniform_device"] = round(row["ragged"]["device_us"] / row["uniform_k3"]["device_us"], 3)
            row["grouped_over_ragged_wall"] = round(row["grouped_3_calls"]["wall_us"] / row["ragged"]["wall_us"], 2)
            row["grouped_over_ragged_device"] = round(row["grouped_3_calls"]["device_us"] / row["ragged"]["device_us"], 2)
            rows.append(row)
            print(json.dumps({"model": name, **row}), file=sys.stderr, flush=True)
        res["models"][name] = rows
    return res


if __name__ == "__main__":
    main()
