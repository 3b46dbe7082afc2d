"""Measurements at patch grids above 16 x 16, written to profiles/highres.md and .json.

  python tools/highres_bench.py [--parts a,b,c,d] [--windows 7] [--window-ms 60] [--out profiles/highres]

Every figure is the median of ``--windows`` windows with the window min-max beside it; a window is
device events around back-to-back calls that fill about ``--window-ms``.  Two arms of a comparison
alternate window by window in one process; ``resolved`` says whether the two window ranges are
disjoint.

 a. the banded ``sdp_dw_wgrad`` at C 768, k 7, B 64 on 24 x 24, 28 x 28 and 32 x 32 (us, GB/s of the
    two operand planes, ns per pixel of the batch), and the whole-plane kernel at 25 x 25, the
    largest plane it takes;
 b. ``sdp_dwconv`` under selection 2 (dwconv2_nhwc) against selection 3 (the tiled MFMA kernel)
    at the same shapes, plain and with LayerNorm, k 3 / 5 / 7;
 c. SdP-Net-M bf16 eval forward at 384 x 384, batch 64, selection 2 against 3;
 d. SdP-Net-M bf16 training step (forward, loss, backward, fused AdamW) at 384 x 384, batch 32.

Run it on the GPU under a time limit, one part per command if the limit is short:
  timeout -k 10 900 python tools/highres_bench.py --parts a,b && timeout -k 10 900 python tools/highres_bench.py --parts c,d
Parts that are not run keep their previous entries in the .json; the .md is rewritten from it, with
the .json's free-text ``note`` under the heading.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sdp-net_amd"))

import torch  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
GRIDS = [(24, 24), (28, 28), (32, 32)]


def window(fn, n):
    """us per call over n back-to-back calls (device events)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def measure(arms, windows, window_ms):
    """arms: {name: fn}.  Warm up, size the window on the first arm, alternate the arms window by
    window.  Returns {name: {"us": median, "min": .., "max": .., "calls_per_window": n}}."""
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    est = max(window(next(iter(arms.values())), 3), 1e-2)
    n = max(3, int(window_ms * 1e3 / est))
    got = {k: [] for k in arms}
    for _ in range(windows):
        for k, fn in arms.items():
            got[k].append(window(fn, n))
    return {k: dict(us=statistics.median(v), min=min(v), max=max(v), calls_per_window=n, windows=windows)
            for k, v in got.items()}


def resolved(a, b):
    return a["max"] < b["min"] or b["max"] < a["min"]


def part_a(args):
    import sdpnet_hip as sp
    L = sp.lib()
    B, C, k = 64, 768, 7
    rows = []
    for H, W in [(25, 25)] + GRIDS:
        a = torch.randn(B * H * W, C, device=DEV).to(BF)
        dy = torch.randn(B * H * W, C, device=DEV).to(BF)
        part = torch.empty(L.sdp_dw_wgrad_chunks(B), C * k * k, dtype=torch.float32, device=DEV)
        cargs = (1, a.data_ptr(), C, 0, 0, 0, dy.data_ptr(), C, 0, 0, 0, B, H, W, C, k, part.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)

        def call():
            rc = L.sdp_dw_wgrad(*cargs)
            if rc != 0:
                raise RuntimeError(f"sdp_dw_wgrad failed with hip error code {rc}")
        r = measure({"dw_wgrad": call}, args.windows, args.window_ms)["dw_wgrad"]
        nbytes = 2 * a.numel() * 2
        r.update(B=B, H=H, W=W, C=C, k=k, kernel="dw_wgrad_k (whole plane)" if H * W <= 640 else "dw_wgrad_band_k",
                 gbps=nbytes / r["us"] * 1e-3, ns_per_pixel=r["us"] * 1e3 / (B * H * W))
        print("a", r, flush=True)
        rows.append(r)
    return rows


def part_b(args):
    import sdpnet_hip as sp
    L = sp.lib()
    B, C = 64, 768
    rows = []
    for H, W in GRIDS:
        M = B * H * W
        x = torch.randn(M, C, device=DEV).to(BF)
        y = torch.empty_like(x)
        stats = torch.empty(M, 2, device=DEV)
        sp.rowstats(sp.dense(x), 1e-6, stats, M, C)
        g, be = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        for k in (3, 5, 7):
            w = (torch.randn(C, k * k, device=DEV) * 0.1).contiguous()
            for ln in (False, True):
                kw = dict(stats=stats, ln_gamma=g, ln_beta=be) if ln else {}

                def arm(sel):
                    def call():
                        L.sdp_dwconv_set_kernel(sel)
                        sp.dwconv(sp.dense(x), w, None, sp.dense(y), B, H, W, C, k, **kw)
                    return call
                old = L.sdp_dwconv_set_kernel(3)
                try:
                    variant = L.sdp_dwconv_variant(1, H, W, C, k)
                    r = measure({"sel2": arm(2), "sel3": arm(3)}, args.windows, args.window_ms)
                finally:
                    L.sdp_dwconv_set_kernel(old)
                row = dict(B=B, H=H, W=W, C=C, k=k, ln=ln, sel3_variant=variant, sel2=r["sel2"], sel3=r["sel3"],
                           ratio=r["sel2"]["us"] / r["sel3"]["us"], resolved=resolved(r["sel2"], r["sel3"]))
                print("b", row, flush=True)
                rows.append(row)
    return rows


def _m_cfg():
    """SdP-Net-M as bench.py builds it, with position tables for a 24 x 24 grid."""
    return dict(embedding_dim=768, num_blocks=12, n_head=8, activation="gelu", embedding_activation="none",
                conv_kernel_size=7, patch_size=16, ffn_dropout=0.2, attn_dropout=0.2, output_classes=1000,
                conv_block_num=2, ff_multiplication_factor=4, max_image_size=[24, 24], max_num_registers=5,
                conv_first=True, head_output_from_register=True, simple_mlp_output=False, output_head_bias=False,
                normalize_qv=True, stochastic_depth_p=[0.0, 0.0], mixer_deptwise_bias=False, mixer_ffn_bias=False,
                conv_embedding=False, conv_embedding_kernel_size=5)


def part_c(args):
    import model as sdp
    import sdpnet_hip as sp
    L = sp.lib()
    B = 64
    torch.manual_seed(231424314)
    m = sdp.MainModel.from_dict(**_m_cfg()).to(DEV).eval()
    x = torch.randn(B, 3, 384, 384, generator=torch.Generator(device="cpu").manual_seed(1)).to(DEV)

    def arm(sel):
        def call():
            L.sdp_dwconv_set_kernel(sel)
            with torch.no_grad(), torch.autocast("cuda", dtype=BF):
                m(x)
        return call
    old = L.sdp_dwconv_set_kernel(3)
    try:
        r = measure({"sel2": arm(2), "sel3": arm(3)}, args.windows, max(args.window_ms, 400.0))
    finally:
        L.sdp_dwconv_set_kernel(old)
    row = dict(model="SdP-Net-M", image=384, grid=[24, 24], batch=B, dtype="bf16 autocast", sel2=r["sel2"],
               sel3=r["sel3"], img_s_sel2=B / r["sel2"]["us"] * 1e6, img_s_sel3=B / r["sel3"]["us"] * 1e6,
               ratio=r["sel2"]["us"] / r["sel3"]["us"], resolved=resolved(r["sel2"], r["sel3"]),
               sel3_variant=L.sdp_dwconv_variant(1, 24, 24, 768, 7))
    print("c", row, flush=True)
    return row


def part_d(args):
    import model as sdp
    import sdpnet_hip as sp
    import sdpnet_train
    B = 32
    cfg = _m_cfg()
    torch.manual_seed(231424314)
    m = sdp.MainModel.from_dict(**cfg).to(DEV).train()
    opt = sdpnet_train.AdamW(m.parameters(), lr=0.0015, weight_decay=0.05)
    g = torch.Generator(device="cpu").manual_seed(1000)
    x = torch.randn(B, 3, 384, 384, generator=g).to(DEV)
    y = torch.randint(0, cfg["output_classes"], (B,), generator=g).to(DEV)
    last = {}

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=BF):
            loss = sdpnet_train.cross_entropy(m(x), y, 0.1)
        opt.scale(loss).backward()
        opt.step(grad_scale=None, max_norm=5.0)
        last["loss"] = loss
    r = measure({"step": step}, args.windows, max(args.window_ms, 600.0))["step"]
    loss = float(last["loss"].detach())
    if not loss == loss:
        raise RuntimeError("training step produced a NaN loss")
    row = dict(model="SdP-Net-M", image=384, grid=[24, 24], batch=B, dtype="bf16 autocast", step=r,
               img_s=B / r["us"] * 1e6, last_loss=loss, dw_selection=sp.lib().sdp_dwconv_set_kernel(0),
               dw_variant=sp.lib().sdp_dwconv_variant(1, 24, 24, 768, 7))
    print("d", row, flush=True)
    return row


def rng(r, scale=1.0, fmt="{:.1f}"):
    return f"{fmt.format(r['us'] * scale)} ({fmt.format(r['min'] * scale)}-{fmt.format(r['max'] * scale)})"


def render(res):
    o = ["# Grids above 16 x 16: measurements (tools/highres_bench.py)", "",
         f"Device: {res.get('device', '?')}.  Median of the windows, window min-max in brackets; arms of a "
         "comparison alternate window by window in one process.", ""]
    if res.get("note"):
        o += [res["note"], ""]
    if "a" in res:
        o += ["## a. `sdp_dw_wgrad`, C 768, k 7, B 64, bf16", "",
              "| plane | kernel | us | GB/s (both operand planes) | ns per pixel |", "|---|---|---|---|---|"]
        for r in res["a"]:
            o.append(f"| {r['H']} x {r['W']} | {r['kernel']} | {rng(r)} | {r['gbps']:.0f} | {r['ns_per_pixel']:.2f} |")
        o.append("")
    if "b" in res:
        o += ["## b. `sdp_dwconv`, C 768, B 64, bf16: selection 2 (dwconv2_nhwc) against 3", "",
              "| plane | k | LN | selection 2 us | selection 3 us | kernel under 3 | 2 / 3 | ranges disjoint |",
              "|---|---|---|---|---|---|---|---|"]
        for r in res["b"]:
            o.append(f"| {r['H']} x {r['W']} | {r['k']} | {'yes' if r['ln'] else 'no'} | {rng(r['sel2'])} | "
                     f"{rng(r['sel3'])} | {r['sel3_variant']} | {r['ratio']:.2f} | {'yes' if r['resolved'] else 'no'} |")
        o.append("")
    if "c" in res:
        r = res["c"]
        o += ["## c. SdP-Net-M eval forward, 384 x 384 (24 x 24 grid), batch 64, bf16 autocast", "",
              "| selection | kernel at 24 x 24 | ms per forward | images/s |", "|---|---|---|---|",
              f"| 2 | 2 | {rng(r['sel2'], 1e-3, '{:.2f}')} | {r['img_s_sel2']:.0f} |",
              f"| 3 | {r['sel3_variant']} | {rng(r['sel3'], 1e-3, '{:.2f}')} | {r['img_s_sel3']:.0f} |", "",
              f"2 / 3 = {r['ratio']:.3f}; window ranges disjoint: {'yes' if r['resolved'] else 'no'}.", ""]
    if "d" in res:
        r = res["d"]
        o += ["## d. SdP-Net-M training step, 384 x 384 (24 x 24 grid), batch 32, bf16 autocast", "",
              f"Forward, label-smoothed CE, backward, fused AdamW with clipping: {rng(r['step'], 1e-3, '{:.1f}')} ms "
              f"per step, {r['img_s']:.0f} images/s (depthwise selection {r['dw_selection']}, kernel "
              f"{r['dw_variant']} at 24 x 24).  A first number: the step raised before the banded weight "
              "gradient.", ""]
    return "\n".join(o)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c,d")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=60.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "highres"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("highres_bench: no GPU; nothing is measured without one")
    res = {}
    if os.path.exists(args.out + ".json"):
        with open(args.out + ".json") as f:
            res = json.load(f)
    res["device"] = torch.cuda.get_device_name(0)
    fns = dict(a=part_a, b=part_b, c=part_c, d=part_d)
    for p in args.parts.split(","):
        res[p] = fns[p](args)
        with open(args.out + ".json", "w") as f:
            json.dump(res, f, indent=1)
        with open(args.out + ".md", "w") as f:
            f.write(render(res) + "\n")


if __name__ == "__main__":
    main()
