"""MXFP8 against bf16: the MLP GEMMs alone, and whole forwards with the switch off / on.

    python tools/mx_bench.py [--parts gemm,forward] [--windows 7] [--window-ms 60] [--out FILE]

Non-zero random operands, everything warm, the arms alternate window by window in one process;
device events around a window of back-to-back launches; median and min-max over the windows.
``resolved`` says whether the windows of two arms do not overlap (max of the faster < min of
the slower): only then is a difference claimed.

(a) ``gemm``: the SdP-Net-M bs256 MLP shapes, 50176 x 3072 x 768 (up: bias + GELU) and
    50176 x 768 x 3072 (down: bias + residual + LN partials), three arms each:
    ``bf16`` sdp_gemm as the model calls it (LN fold on the up GEMM), ``mx`` sdp_gemm_mx on
    quantised operands (up writes the MX hidden, down reads it), ``quant+mx`` the up GEMM with the
    quantiser pass of its input in front.
(b) ``forward``: SdP-Net-M at batch 256 and SdP-Net-XL at batch 512 (bf16, random-init weights),
    the eager forward with model.mx_fp8 False / True.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "sdp-net_amd"))


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def resolved(a, b):
    fast, slow = (a, b) if a["median"] < b["median"] else (b, a)
    return fast["max"] < slow["min"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="gemm,forward")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=60.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mx_fp8_bench.json"))
    args = ap.parse_args()

    import torch
    import bench
    import model as ours
    import sdpnet_hip as sp

    if not torch.cuda.is_available():
        raise SystemExit("mx_bench needs the GPU")
    dev = torch.device("cuda", 0)
    BF = torch.bfloat16

    def window(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def interleave(arms):
        for fn in arms.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        n = max(3, int(args.window_ms / max(window(next(iter(arms.values())), 3), 1e-3)))
        t = {k: [] for k in arms}
        for _ in range(args.windows):
            for k, fn in arms.items():
                t[k].append(window(fn, n))
        return {k: stats(v) for k, v in t.items()}, n

    out = {"tool": "tools/mx_bench.py", "device": torch.cuda.get_device_name(0), "gemm": [], "forward": []}
    parts = args.parts.split(",")
    if "gemm" in parts:
        M, C, F_ = 50176, 768, 3072
        g = torch.Generator(device="cpu").manual_seed(1)
        x = (torch.randn(M, C, generator=g) + 0.3).to(dev).to(BF)
        w_up32 = (torch.randn(F_, C, generator=g) * 0.04).to(dev)
        w_dn32 = (torch.randn(C, F_, generator=g) * 0.02).to(dev)
        gam, bet = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        b_up, b_dn = torch.randn(F_, generator=g).to(dev) * 0.1, torch.randn(C, generator=g).to(dev) * 0.1
        part = torch.empty(M, C // 64, 2, device=dev)
        sp.row_partials(sp.dense(x), M, C, part)
        st = torch.empty(M, 2, device=dev)
        sp.ln_stats(part, sp.dense(x), M, C, 1e-6, st)
        wf, colsum, cvec = sp.fold_ln_weight(w_up32, gam, bet, b_up, BF)
        wf32, _, _ = sp.fold_ln_weight(w_up32, gam, bet, b_up, torch.float32)
        w_dn = w_dn32.to(BF)
        wq_up, wq_dn = sp.mx_quant_rows(sp.dense(wf32), F_, C), sp.mx_quant_rows(sp.dense(w_dn32), C, F_)
        hid = torch.empty(M, F_, dtype=BF, device=dev)
        hid_mx = sp.mx_empty(M, F_, dev)
        xq = sp.mx_empty(M, C, dev)
        y = x.clone()
        sp.mx_quant_rows(sp.dense(x), M, C, stats=st, out=xq)

        def up_bf16():
            sp.gemm(sp.dense(x), wf, sp.dense(hid), M, F_, C, bias=cvec, act=1, ln=(st, colsum))

        def up_mx():
            sp.gemm_mx(xq, wq_up, M, F_, C, out_mx=hid_mx, bias=cvec, act=1)

        def up_quant_mx():
            sp.mx_quant_rows(sp.dense(x), M, C, stats=st, out=xq)
            up_mx()

        def dn_bf16():
            sp.gemm(sp.dense(hid), w_dn, sp.dense(y), M, C, F_, bias=b_dn, resid=sp.dense(x), part=part)

        def dn_mx():
            sp.gemm_mx(hid_mx, wq_dn, M, C, F_, y=sp.dense(y), bias=b_dn, resid=sp.dense(x), part=part)
        up_bf16()
        up_mx()
        for name, (N, K), arms in (("up 50176x3072x768", (F_, C), {"bf16": up_bf16, "mx": up_mx, "quant+mx": up_quant_mx}),
                                   ("down 50176x768x3072", (C, F_), {"bf16": dn_bf16, "mx": dn_mx})):
            t, n = interleave(arms)
            fl = 2.0 * M * N * K
            row = {"gemm": name, "launches_per_window": n, "windows": args.windows, "ms": t,
                   "tflops": {k: round(fl / (v["median"] * 1e-3) / 1e12, 1) for k, v in t.items()},
                   "speedup_mx_over_bf16": round(t["bf16"]["median"] / t["mx"]["median"], 3),
                   "resolved": resolved(t["bf16"], t["mx"])}
            out["gemm"].append(row)
            print(json.dumps(row), flush=True)
    if "forward" in parts:
        for name, cfg, B in (("SdP-Net-M", bench.M_CFG, 256), ("SdP-Net-XL", bench.XL_CFG, 512)):
            torch.manual_seed(231424314)
            m = ours.MainModel(**cfg).to(dev).eval()
            g = torch.Generator(device="cpu").manual_seed(B)
            x = torch.randn(B, 3, 224, 224, generator=g).to(dev).to(BF)

            def arm(on):
                def run():
                    m.mx_fp8 = on
                    with torch.no_grad():
                        m(x)
                return run
            t, n = interleave({"off": arm(False), "on": arm(True)})
            m.mx_fp8 = False
            y0 = m(x).float()
            m.mx_fp8 = True
            y1 = m(x).float()
            row = {"config": name, "batch": B, "forwards_per_window": n, "windows": args.windows, "ms": t,
                   "img_per_s": {k: round(B / (v["median"] * 1e-3), 1) for k, v in t.items()},
                   "speedup_on_over_off": round(t["off"]["median"] / t["on"]["median"], 3),
                   "resolved": resolved(t["off"], t["on"]),
                   "rms_logit_diff_on_vs_off": float((y1 - y0).pow(2).mean().sqrt()),
                   "rms_logit": float(y0.pow(2).mean().sqrt())}
            out["forward"].append(row)
            print(json.dumps(row), flush=True)
            del m
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
