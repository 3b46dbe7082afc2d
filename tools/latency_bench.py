"""Small-batch inference latency: graph replay with the low-latency switch off against on.

    python tools/latency_bench.py [--configs m,xl,xxs] [--batches 1,2,4,8,16,32] [--out FILE]
    python tools/latency_bench.py --profile [--arm off] --configs m --batches 1   (under rocprofv3, no timing)

Per configuration and batch (bf16 input, random-init weights, 224 x 224 synthetic images):

* ``replay_ms``: one captured eval forward replayed back to back, device events around a window of
  replays long enough to take ~50 ms; the two arms (off = the default kernels, on = planned GEMMs on
  the split-K kernel) alternate window by window in the same process; median and min-max over the
  windows.  ``speedup`` is median off / median on, ``resolved`` says whether the windows of the two
  arms do not overlap (max of the faster < min of the slower).
* ``call_ms``: the same through GraphedForward.__call__ (input copy and stale-weight check
  included), host clock around a window that ends in a synchronise.
* ``eager_ms``: the eager forward (several hundred launches from Python), both arms: with
  ``replay_ms`` it puts the launch-overhead share on record.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "sdp-net_amd"))


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="m,xl,xxs")
    ap.add_argument("--batches", default="1,2,4,8,16,32")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "low_latency_bench.json"))
    ap.add_argument("--profile", action="store_true", help="60 eager forwards of one arm only (run under a profiler)")
    ap.add_argument("--arm", choices=["off", "on"], default="on", help="the arm --profile runs")
    args = ap.parse_args()

    import torch
    import bench
    import model as ours
    import sdpnet_engine
    import sdpnet_hip as sp

    if not torch.cuda.is_available():
        raise SystemExit("latency_bench needs the GPU: a CPU run cannot give a latency")
    dev = torch.device("cuda", 0)
    cfgs = {"m": bench.M_CFG, "xl": bench.XL_CFG, "xxs": bench.XXS_CFG}
    names = {"m": "SdP-Net-M", "xl": "SdP-Net-XL", "xxs": "SdP-Net-XXS"}
    rows = []
    for key in args.configs.split(","):
        torch.manual_seed(231424314)
        m_off = ours.MainModel(**cfgs[key]).to(dev).eval()
        m_off.low_latency = False
        m_on = copy.deepcopy(m_off)
        m_on.low_latency = True
        for B in [int(b) for b in args.batches.split(",")]:
            g = torch.Generator(device="cpu").manual_seed(B)
            x = torch.randn(B, 3, 224, 224, generator=g).to(dev).to(torch.bfloat16)
            if args.profile:
                with torch.no_grad():
                    for _ in range(60):
                        (m_on if args.arm == "on" else m_off)(x)
                torch.cuda.synchronize()
                continue
            arms = {"off": sdpnet_engine.GraphedForward(m_off, x), "on": sdpnet_engine.GraphedForward(m_on, x)}
            y = {k: gf(x).float().clone() for k, gf in arms.items()}
            diff = float((y["on"] - y["off"]).abs().max())
            # planned GEMMs of this forward (counted on an eager call)
            calls, real = [], sp.gemm_splitk
            sp.gemm_splitk = lambda *a, **kw: (calls.append(a[3:8]), real(*a, **kw))[1]
            try:
                m_on(x)
            finally:
                sp.gemm_splitk = real
            torch.cuda.synchronize()

            def replay_window(gf, n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    gf._graph.replay()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / n

            def call_window(gf, n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    gf(x)
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0) / n

            def eager_window(m, n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    m(x)
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0) / n

            est = max(replay_window(arms["off"], 10), 1e-3)
            n = max(20, int(args.window_ms / est))
            rep = {"off": [], "on": []}
            call = {"off": [], "on": []}
            for _ in range(args.windows):
                for k in ("off", "on"):
                    rep[k].append(replay_window(arms[k], n))
                for k in ("off", "on"):
                    call[k].append(call_window(arms[k], max(10, n // 2)))
            eager = {"off": [], "on": []}
            ne = max(5, int(args.window_ms / max(eager_window(m_off, 3), 1e-3)))
            for _ in range(3):
                eager["off"].append(eager_window(m_off, ne))
                eager["on"].append(eager_window(m_on, ne))
            r, c = {k: stats(v) for k, v in rep.items()}, {k: stats(v) for k, v in call.items()}
            fast, slow = ("on", "off") if r["on"]["median"] < r["off"]["median"] else ("off", "on")
            row = {"config": names[key], "batch": B, "dtype": "bf16", "replays_per_window": n, "windows": args.windows,
                   "replay_ms": r, "call_ms": c, "eager_ms": {k: stats(v) for k, v in eager.items()},
                   "speedup": round(r["off"]["median"] / r["on"]["median"], 3),
                   "resolved": r[fast]["max"] < r[slow]["min"],
                   "splitk_gemms": len(calls), "plans": sorted({tuple(c_) for c_ in calls}),
                   "max_abs_logit_diff_on_vs_off": diff, "max_abs_logit": float(y["off"].abs().max())}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del arms
    if not args.profile:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/latency_bench.py", "device": torch.cuda.get_device_name(0),
                       "cus": torch.cuda.get_device_properties(0).multi_processor_count, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
