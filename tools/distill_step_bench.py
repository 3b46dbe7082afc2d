"""What knowledge distillation costs per training step: the SdP-Net-M bs-120 training step with an
SdP-Net-XL teacher, in three arms run alternately in one process.

  A  the fused step: bf16 autocast forward, ``cross_entropy`` (label smoothing 0.1), backward,
     ``AdamW.step`` (GradScaler unscale, clip_grad_norm_(5));
  B  A with the loss replaced by ``distillation_loss`` (soft, alpha 0.5, T 2) against the logits of
     an XL teacher run on the same batch (bf16, eval, ``torch.no_grad()``), as ``training_tools.Trainer``
     runs it with ``distill_kind="soft"``;
  A+T  A with the same teacher forward in the same place and its logits thrown away (the loss stays
     ``cross_entropy``): B - (A+T) is what the loss itself adds, (A+T) - A - teacher what running the
     teacher between the student's forward and backward costs beyond its stand-alone time.

Each arm is warmed up, then timed ``--reps`` times over ``--steps`` steps (host clock around work
that ends in a device synchronize), the arms interleaved so that drift hits both alike.  The
teacher forward alone is timed the same way in the same interleave.  ``sdp_distill_loss`` and
``sdp_ce_loss_soft`` alone are timed with device events over back-to-back launches at
(B, K) = (120, 1000) and (256, 1000), bf16 student logits, bf16 teacher logits, fp32 target rows.
The result records the numbers; it sets no pass mark.

  python tools/distill_step_bench.py [--steps 20 --reps 2 --warmup 3] [--out profiles/distill_step_bench.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "sdp-net_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=120)
    ap.add_argument("--kernel-launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("distill_step_bench needs the GPU: nothing here can be timed on the CPU")
    import bench
    import model as sdp
    import sdpnet_hip as sp
    import sdpnet_train
    B = args.batch
    dev = torch.device("cuda", 0)
    torch.manual_seed(231424314)
    m = sdp.MainModel.from_dict(**bench.M_CFG).to(dev).train()
    teacher = sdp.MainModel.from_dict(**bench.XL_CFG).to(dev).eval().requires_grad_(False)
    opt = sdpnet_train.AdamW(m.parameters(), lr=0.0015, weight_decay=0.05)
    g = torch.Generator(device="cpu").manual_seed(1000)
    x = torch.randn(B, 3, 224, 224, generator=g).to(dev)
    K = bench.M_CFG["output_classes"]
    y = torch.randint(0, K, (B,), generator=g).to(dev)

    def step(distill, run_teacher=None):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m(x)
            if distill or run_teacher:
                with torch.no_grad():
                    tl = teacher(x)
            if distill:
                loss = sdpnet_train.distillation_loss(out, tl, y, alpha=0.5, temperature=2.0, kind="soft", base="ce",
                                                      label_smoothing=0.1)
            else:
                loss = sdpnet_train.cross_entropy(out, y, 0.1)
        opt.scale(loss).backward()
        opt.step(grad_scale=None, max_norm=5.0)
        return loss

    def teacher_only():
        with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
            return teacher(x)

    arms = [("A", lambda: step(False)), ("B", lambda: step(True)), ("A+T", lambda: step(False, run_teacher=True)),
            ("teacher", teacher_only)]
    for _, fn in arms:
        for _ in range(max(1, args.warmup)):
            fn()
    tl = teacher_only()
    teacher_dtype = str(tl.dtype)
    ms = {n: [] for n, _ in arms}
    for _ in range(args.reps):
        for n, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            ms[n].append(1e3 * (time.perf_counter() - t0) / args.steps)

    # host time to enqueue the loss alone (the device is idle): what arm B adds on the host besides the teacher
    def host_ms(fn, n=20):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        el = time.perf_counter() - t0
        torch.cuda.synchronize()
        return 1e3 * el / n
    zl = torch.randn(B, K, device=dev, dtype=torch.bfloat16)
    host = dict(cross_entropy_enqueue_ms=host_ms(lambda: sdpnet_train.cross_entropy(zl, y, 0.1)),
                distillation_loss_enqueue_ms=host_ms(lambda: sdpnet_train.distillation_loss(zl, tl, y, alpha=0.5,
                                                                                            temperature=2.0)))

    # the loss kernels alone
    kern = {}
    for b in (120, 256):
        z = torch.randn(b, K, device=dev).to(torch.bfloat16)
        t = torch.randn(b, K, device=dev).to(torch.bfloat16)
        rows = torch.softmax(torch.randn(b, K, device=dev), 1)
        d = torch.empty_like(z)
        loss = torch.zeros(1, device=dev)
        parts = torch.zeros(2, device=dev)
        calls = {"sdp_ce_loss_soft": lambda: sp.ce_loss_soft(z, rows, 0.1, 1.0, d, loss),
                 "sdp_distill_loss": lambda: sp.distill_loss(z, t, rows, 0.1, 0.5, 2.0, 0, 1.0, d, loss, parts)}
        res = {}
        for name, fn in calls.items():
            for _ in range(5):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.kernel_launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name] = round(1e3 * e0.elapsed_time(e1) / args.kernel_launches, 2)
        kern[f"{b}x{K}"] = dict(us_per_launch=res)

    mean = {n: sum(v) / len(v) for n, v in ms.items()}
    spread_a = max(ms["A"]) - min(ms["A"])
    extra = mean["B"] - mean["A"] - mean["teacher"]
    out = dict(workload=f"SdP-Net-M training step bs {B} (12 blocks, d=768, patch 16), SdP-Net-XL teacher (17 blocks, "
                        "patch 14), soft distillation alpha 0.5 T 2",
               batch=B, steps_per_window=args.steps, reps=args.reps, warmup=args.warmup,
               ms_per_step={n: [round(v, 3) for v in vs] for n, vs in ms.items()},
               mean_ms_per_step={n: round(v, 3) for n, v in mean.items()},
               images_per_s={n: round(1e3 * B / v, 1) for n, v in mean.items()},
               b_minus_a_ms=round(mean["B"] - mean["A"], 3), teacher_alone_ms=round(mean["teacher"], 3),
               b_minus_a_minus_teacher_ms=round(extra, 3), spread_between_a_windows_ms=round(spread_a, 3),
               loss_alone_b_minus_at_ms=round(mean["B"] - mean["A+T"], 3),
               interleaving_at_minus_a_minus_teacher_ms=round(mean["A+T"] - mean["A"] - mean["teacher"], 3),
               teacher_logits_dtype=teacher_dtype, host={k: round(v, 3) for k, v in host.items()}, loss_kernels=kern,
               timing="host clock around N steps ending in torch.cuda.synchronize(); kernels: device events over "
                      f"{args.kernel_launches} back-to-back launches")
    line = json.dumps(out)
    print(line, flush=True)
    print("arm      " + "  ".join(f"rep{i + 1} ms/step" for i in range(args.reps)))
    for n, vs in ms.items():
        print(f"{n:8s} " + "  ".join(f"{v:12.2f}" for v in vs))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
