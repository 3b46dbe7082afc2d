"""Device-side training batch augmentation against its two yardsticks.

  python tools/aug_bench.py [--batch 120] [--hw 224,224] [--reps 200] [--repeats 7]
                            [--out profiles/train_aug_bench.json]

* sdp_train_batch_aug on a device-resident uint8 batch, fp32 and bf16 output, modes none / MixUp /
  CutMix: device time over events after warm-up, median / min / max over ``--repeats`` windows of
  ``--reps`` launches (captured into a graph and replayed, so that the host's enqueue rate does
  not bound the window), next to the kernel's algorithmic bytes (source pixels read once per use,
  output and target rows written once) as a rate and as a fraction of the HBM peak.  The launches
  rotate through enough buffer sets that a window streams more than the 256 MiB Infinity Cache,
  so the rate is a memory rate and not a cache rate.
* Host yardstick: the same batch through the torch restatement of the reference's collate
  (tests/augment_oracle.py: normalise, erase, CutMix / MixUp, one-hot mixing; fp32 on the CPU),
  limited to 16 threads, wall time.
* Copy yardstick: the pinned host-to-device copy of the fp32 batch plus its dense targets (what the
  reference's loader ships) against the uint8 batch plus labels and plan (what this path ships).

No threshold is attached: the numbers go into DESIGN.md.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sdp-net_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

import augment_oracle as ao  # noqa: E402
import preprocess as pp  # noqa: E402
import sdpnet_hip as sp  # noqa: E402

HBM_PEAK_GBS = 8000.0
L3_BYTES = 256 << 20
MODES = {0: "none", 1: "mixup", 2: "cutmix"}


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def plan_for(mode, B, H, W, seed=0):
    """A sampled per-image plan (erase p = 0.25) with the batch mode forced; CutMix at lam = 0.5
    (the mean of Beta(1, 1)), centred, so its box covers half of the image area."""
    p = pp.AugPlan.sample(B, H, W, torch.Generator().manual_seed(seed), mix=None)
    if mode == 1:
        p.with_mixup(0.5)
    elif mode == 2:
        p.with_cutmix(0.5, W // 2, H // 2)
    return p


def algorithmic_bytes(plan, K, out_es):
    B, H, W = plan.B, plan.H, plan.W
    px = B * 3 * H * W
    read = px
    if plan.mode == 1:
        read += px
    elif plan.mode == 2:
        x1, y1, x2, y2 = plan.box
        read += B * 3 * (y2 - y1) * (x2 - x1)
    targets = B * K * 4 if plan.mode else 0
    return read + px * out_es + targets


def device_times(B, H, W, K, reps, repeats):
    dev = torch.device("cuda")
    lut = pp.normalize_lut().to(dev)
    g = torch.Generator().manual_seed(0)
    per_set = B * 3 * H * W * 5
    nset = max(2, -(-2 * L3_BYTES // per_set))
    imgs = [torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8).to(dev) for _ in range(nset)]
    labels = torch.randint(0, K, (B,), generator=g).to(dev)
    rows = []
    for dtype in (torch.float32, torch.bfloat16):
        for mode, name in MODES.items():
            plan = plan_for(mode, B, H, W)
            plan_d = torch.from_numpy(plan.pack()).to(dev)
            tg = [torch.empty(B, K, device=dev) for _ in range(nset)] if mode else [None] * nset
            outs = [torch.empty(B, 3, H, W, dtype=dtype, device=dev) for _ in range(nset)]

            def run(i):
                return sp.train_batch_aug(imgs[i % nset], labels, lut, plan_d, K, dtype, mode != 0,
                                          targets=tg[i % nset], out=outs[i % nset])
            for i in range(nset + 3):
                run(i)
            torch.cuda.synchronize()
            # The kernel takes tens of microseconds, less than the binding needs to enqueue it, so
            # a window of eager launches would time the host.  The window is captured once and
            # replayed: the events then bracket back-to-back device work (launch gaps included).
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for i in range(reps):
                    run(i)
            graph.replay()
            torch.cuda.synchronize()
            us = []
            for _ in range(repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graph.replay()
                e1.record()
                torch.cuda.synchronize()
                us.append(1e3 * e0.elapsed_time(e1) / reps)
            eager = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                for i in range(reps):
                    run(i)
                torch.cuda.synchronize()
                eager.append(1e6 * (time.perf_counter() - t0) / reps)
            nbytes = algorithmic_bytes(plan, K, 4 if dtype == torch.float32 else 2)
            med = statistics.median(us)
            gbs = nbytes / (med * 1e-6) / 1e9
            rows.append({"out_dtype": str(dtype).replace("torch.", ""), "mode": name, "us_per_batch": spread(us),
                         "eager_us_per_call_host_bound": spread(eager),
                         "algorithmic_bytes": nbytes, "achieved_GBs": round(gbs, 1),
                         "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
                         "images_per_s": round(B / (med * 1e-6), 1)})
    return rows, nset


def host_times(B, H, W, K, repeats, threads):
    torch.set_num_threads(threads)
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, K, (B,), generator=g)
    rows = []
    for mode, name in MODES.items():
        plan = plan_for(mode, B, H, W)
        ao.apply(img, labels, plan, K)
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            ao.apply(img, labels, plan, K)
            ms.append(1e3 * (time.perf_counter() - t0))
        rows.append({"mode": name, "ms_per_batch": spread(ms), "threads": threads,
                     "images_per_s": round(B / (statistics.median(ms) * 1e-3), 1)})
    return rows


def copy_times(B, H, W, K, reps, repeats):
    dev = torch.device("cuda")
    out = {}
    for name, nbytes in (("fp32_batch_and_targets", B * 3 * H * W * 4 + B * K * 4),
                         ("uint8_batch_labels_plan", B * 3 * H * W + B * 8 + 4 * (8 + 8 * B))):
        host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        host.random_(0, 256)
        dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        for _ in range(3):
            dst.copy_(host, non_blocking=True)
        torch.cuda.synchronize()
        us = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                dst.copy_(host, non_blocking=True)
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / reps)
        out[name] = {"bytes": nbytes, "us_per_copy": spread(us),
                     "GBs": round(nbytes / (statistics.median(us) * 1e-6) / 1e9, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=120)
    ap.add_argument("--hw", default="224,224")
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--device-only", action="store_true", help="skip the host and copy yardsticks")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train_aug_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aug_bench.py measures on the GPU; no device found")
    H, W = (int(v) for v in args.hw.split(","))
    B, K = args.batch, args.classes
    dev_rows, nset = device_times(B, H, W, K, args.reps, args.repeats)
    res = {"op": "sdp_train_batch_aug", "device": torch.cuda.get_device_name(0), "batch": B, "image_hw": [H, W],
           "classes": K, "reps_per_window": args.reps, "windows": args.repeats, "buffer_sets": nset,
           "hbm_peak_GBs": HBM_PEAK_GBS, "device_kernel": dev_rows}
    if not args.device_only:
        res["host_collate_torch_ops"] = host_times(B, H, W, K, args.repeats, args.host_threads)
        res["h2d_pinned"] = copy_times(B, H, W, K, args.reps, args.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
