"""What the weight average costs per training step: the SdP-Net-XL bs-120 step of
``bench.py --config xl_train`` (same configuration and seeds) in three arms, run alternately in
one process.

  A  the fused step alone (forward, CE, backward, AdamW.step);
  B  A + the reference's EMA update (training_tools.py:291-297) in per-entry torch ops, behind the
     per-batch ``torch.cuda.synchronize()`` of the reference's epoch loop (:115-119);
  C  A + ``EMA.update_parameters`` (one ``sdp_ema_update`` launch, no synchronize), as
     ``training_tools.Trainer`` runs it.

Each arm is warmed up, then timed ``--reps`` times over ``--steps`` steps (host clock around work
that ends in a device synchronize), the arms interleaved so that drift hits all three alike.  The
EMA kernel alone is timed with device events over back-to-back launches; its bytes/s count
3 x 4 B x elements (two operand reads and one write per element), the algorithmic traffic of the
running-average form.

  python tools/trainer_step_bench.py [--steps 20 --reps 2 --warmup 3] [--out profiles/trainer_step_bench.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "sdp-net_amd"))

HBM_PEAK_TBS = 8.0  # MI355X HBM3E specification


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-launches", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("trainer_step_bench needs the GPU: nothing here can be timed on the CPU")
    import bench
    import model as sdp
    import sdpnet_hip as sp
    import sdpnet_train
    C = bench.CONFIGS["xl_train"]
    cfg, B = C["cfg"], C["batch"]
    dev = torch.device("cuda", 0)
    torch.manual_seed(231424314)
    m = sdp.MainModel.from_dict(**cfg).to(dev).train()
    opt = sdpnet_train.AdamW(m.parameters(), lr=0.0015, weight_decay=0.05)
    g = torch.Generator(device="cpu").manual_seed(1000)
    x = torch.randn(B, 3, 224, 224, generator=g).to(dev)
    y = torch.randint(0, cfg["output_classes"], (B,), generator=g).to(dev)

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = sdpnet_train.cross_entropy(m(x), y, 0.1)
        opt.scale(loss).backward()
        opt.step(grad_scale=None, max_norm=5.0)
        return loss

    decay = 0.999
    ref_ema = {k: v.clone().detach() for k, v in m.state_dict().items()}
    ema = sdpnet_train.EMA(m, decay=decay, reference_quirks=True)

    def ref_update():  # training_tools.py:291-297 as written
        with torch.no_grad():
            for keys, values in m.state_dict().items():
                if "num_batches_tracked" or "running" in keys:
                    ref_ema[keys].copy_(values)
                ref_ema[keys] = decay * ref_ema[keys] + (1 - decay) * values.detach()

    def arm_a():
        step()

    def arm_b():
        step()
        torch.cuda.synchronize()
        ref_update()

    def arm_c():
        step()
        ema.update_parameters(m)

    arms = [("A", arm_a), ("B", arm_b), ("C", arm_c)]
    for _, fn in arms:
        for _ in range(max(1, args.warmup)):
            fn()
    # on the same weights the kernel's state equals the torch loop's, bit for bit
    ref_update()
    ema.update_parameters(m)
    torch.cuda.synchronize()
    same = all(v.dtype == ema.state_dict()[k].dtype and torch.equal(ema.state_dict()[k], v) for k, v in ref_ema.items())
    ms = {n: [] for n, _ in arms}
    for _ in range(args.reps):
        for n, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            ms[n].append(1e3 * (time.perf_counter() - t0) / args.steps)

    # host time of the two updates alone (enqueue only; the device is idle)
    def host_ms(fn, n=5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        el = time.perf_counter() - t0
        torch.cuda.synchronize()
        return 1e3 * el / n
    host = dict(reference_loop_enqueue_ms=host_ms(ref_update), ema_update_parameters_enqueue_ms=host_ms(lambda: ema.update_parameters(m)))

    # the kernel alone, both forms
    sd = m.state_dict()
    n_entries = len(sd)
    n_fp32 = sum(1 for v in sd.values() if v.dtype == torch.float32)
    elems = sum(v.numel() for v in sd.values() if v.dtype == torch.float32)
    kern = {}
    for name, quirks in (("running_average", False), ("reference_form", True)):
        e = sdpnet_train.EMA(m, decay=decay, reference_quirks=quirks)
        for _ in range(3):
            e.update_parameters(m)
        t = e._tab
        a = t["w"] if quirks else t["e"]
        a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a0.record()
        for _ in range(args.kernel_launches):
            sp.ema_update(t["e"], a, t["w"], t["sizes"], t["blocks"], t["nblocks"], decay, 1 - decay)
        a1.record()
        torch.cuda.synchronize()
        us = 1e3 * a0.elapsed_time(a1) / args.kernel_launches
        streams = 2 if quirks else 3  # a == b: each element is read once
        kern[name] = dict(us_per_launch=round(us, 1), bytes_moved=streams * 4 * elems,
                          tb_per_s=round(streams * 4 * elems / (us * 1e-6) / 1e12, 3),
                          share_of_hbm_peak=round(streams * 4 * elems / (us * 1e-6) / 1e12 / HBM_PEAK_TBS, 3),
                          algorithmic_bytes_3x4xelements=3 * 4 * elems,
                          tb_per_s_at_3x4xelements=round(3 * 4 * elems / (us * 1e-6) / 1e12, 3))
    out = dict(workload=C["desc"], batch=B, steps_per_window=args.steps, reps=args.reps, warmup=args.warmup,
               ms_per_step={n: [round(v, 3) for v in vs] for n, vs in ms.items()},
               state_dict_entries=n_entries, fp32_entries=n_fp32, fp32_elements=elems, blocks=ema._tab["nblocks"],
               kernel_state_equals_torch_loop=bool(same), host={k: round(v, 3) for k, v in host.items()},
               ema_kernel=kern, timing="host clock around N steps ending in torch.cuda.synchronize(); kernel: device "
               f"events over {args.kernel_launches} back-to-back launches", hbm_peak_tb_per_s=HBM_PEAK_TBS)
    line = json.dumps(out)
    print(line, flush=True)
    print("arm  " + "  ".join(f"rep{i + 1} ms/step" for i in range(args.reps)))
    for n, vs in ms.items():
        print(f"{n}    " + "  ".join(f"{v:12.2f}" for v in vs))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
