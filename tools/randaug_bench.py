"""Device-side RandomResizedCrop + flip + RandAugment against the PIL pipeline it replaces.

  python tools/randaug_bench.py [--batch 120] [--reps 20] [--repeats 7] [--step-ms MS]
                                [--out profiles/device_randaug.json]

For one batch of synthetic decoded images (random pixels, about 500 x 375; no JPEGs: decode is not
part of either side) and one sampled plan:

* device time of sdp_resized_crop, sdp_randaugment and sdp_train_batch_aug, each over events around
  ``--reps`` back-to-back launches on device-resident operands;
* the pinned host-to-device copy of what ``TrainImageTransform`` uploads (rows under the crop boxes,
  plans, image table, labels), its size, and the size of whole images for comparison;
* the host wall time of ``TrainImageTransform.__call__`` (packing included, ending in a device
  synchronise);
* one core running the same three steps through Pillow with the same plan (crop().resize(BICUBIC),
  flip, two RandAugment ops), its output checked against the device's uint8 batch.

The windows of the four measurements alternate ``--repeats`` times in one process; median and
min-max are reported.  ``--step-ms``: a training step time measured on the same box (bench.py
--config xl_train), recorded next to the device time.  No threshold is attached.
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
sys.path.insert(0, os.path.join(REPO, "oracle"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import preprocess as pp  # noqa: E402
import sdpnet_hip as sp  # noqa: E402
from test_randaug_host import pil_op  # noqa: E402

OUT = (224, 224)


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def pil_pipeline(images, crop):
    out = []
    for a, (top, left, h, w), f, ops in zip(images, crop.boxes.tolist(), crop.flip.tolist(), crop.ops):
        im = Image.fromarray(a).crop((left, top, left + w, top + h)).resize((OUT[1], OUT[0]), Image.Resampling.BICUBIC)
        if f:
            im = im.transpose(Image.Transpose.FLIP_LEFT_RIGHT)
        x = np.asarray(im)
        for name, m in ops:
            x = pil_op(x, name, m)
        out.append(x)
    return np.stack(out)


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=120)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step-ms", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "device_randaug.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("randaug_bench.py measures on the GPU; no device found")
    dev = torch.device("cuda")
    B = args.batch
    rng = np.random.default_rng(0)
    sizes = [(int(rng.integers(333, 501)), int(rng.integers(375, 501))) for _ in range(B)]
    sizes = [(h, w) if i % 2 else (w, h) for i, (h, w) in enumerate(sizes)]
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    labels = torch.from_numpy(rng.integers(0, 1000, B))
    g = torch.Generator().manual_seed(0)
    t = pp.TrainImageTransform(OUT, device=dev, dtype=torch.bfloat16, generator=g)
    crop, plan = t.sample(sizes)

    # device-resident operands of the three kernels (whole images; the boxes address into them)
    nbytes = np.array([a.size for a in images], np.int64)
    offs = np.zeros(B, np.int64)
    offs[1:] = np.cumsum(nbytes)[:-1]
    pix = torch.from_numpy(np.concatenate([a.reshape(-1) for a in images])).to(dev)
    offs_d, hw_d = torch.from_numpy(offs).to(dev), torch.tensor(sizes, dtype=torch.int32, device=dev)
    words = crop.pack()
    n_box = sp.CROP_PLAN_PER_IMAGE * B
    crop_d, ra_d = torch.from_numpy(words[:n_box].copy()).to(dev), torch.from_numpy(words[n_box:].copy()).to(dev)
    plan_d = torch.from_numpy(plan.pack()).to(dev)
    labels_d = labels.to(dev)
    kmax, max_h, max_w = crop.kmax(), int(crop.boxes[:, 2].max()), int(crop.boxes[:, 3].max())
    ws = torch.empty(sp.resized_crop_ws_words(B, OUT, kmax), dtype=torch.int32, device=dev)
    tmp = torch.empty(B * max_h * OUT[1] * 4, dtype=torch.uint8, device=dev)
    u8 = torch.empty(B, *OUT, 3, dtype=torch.uint8, device=dev)
    aug = torch.empty_like(u8)
    scratch = torch.empty(u8.numel(), dtype=torch.uint8, device=dev)
    out = torch.empty(B, 3, *OUT, dtype=torch.bfloat16, device=dev)
    targets = torch.empty(B, 1000, device=dev) if plan.mode else None

    def k_crop():
        sp.resized_crop(pix, offs_d, hw_d, crop_d, OUT, kmax, max_h, max_w, ws=ws, tmp=tmp, out=u8)

    def k_ra():
        sp.randaugment(u8, ra_d, crop.num_ops, scratch=scratch, out=aug)

    def k_batch():
        sp.train_batch_aug(aug, labels_d, t.lut, plan_d, 1000, torch.bfloat16, plan.mode != 0, channels_last=True,
                           targets=targets, out=out)

    # what TrainImageTransform uploads: the rows under the boxes + plans + table + labels
    up_bytes = int((crop.boxes[:, 2] * np.array(sizes)[:, 1] * 3).sum()) + 4 * crop.words() + 4 * plan.words() + 24 * B
    host = torch.empty(up_bytes, dtype=torch.uint8, pin_memory=True)
    host.random_(0, 256)
    dst = torch.empty(up_bytes, dtype=torch.uint8, device=dev)

    def k_copy():
        dst.copy_(host, non_blocking=True)

    def e2e():
        t0 = time.perf_counter()
        t(images, labels, crop_plan=crop, plan=plan)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for fn in (k_crop, k_ra, k_batch, k_copy):
        for _ in range(3):
            fn()
    for _ in range(3):
        e2e()
    torch.cuda.synchronize()
    same = bool(np.array_equal(aug.cpu().numpy(), pil_pipeline(images, crop)))

    us = {"sdp_resized_crop": [], "sdp_randaugment": [], "sdp_train_batch_aug": [], "h2d_copy": []}
    e2e_ms, pil_ms = [], []
    for _ in range(args.repeats):
        us["sdp_resized_crop"].append(events(k_crop, args.reps))
        us["sdp_randaugment"].append(events(k_ra, args.reps))
        us["sdp_train_batch_aug"].append(events(k_batch, args.reps))
        us["h2d_copy"].append(events(k_copy, args.reps))
        e2e_ms.append(e2e())
        t0 = time.perf_counter()
        pil_pipeline(images, crop)
        pil_ms.append(1e3 * (time.perf_counter() - t0))
    dev_us = sum(statistics.median(us[k]) for k in ("sdp_resized_crop", "sdp_randaugment", "sdp_train_batch_aug"))
    pil_med = statistics.median(pil_ms)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "out_size": list(OUT), "out_dtype": "bfloat16",
           "mean_image_hw": [round(float(np.mean([s[0] for s in sizes])), 1), round(float(np.mean([s[1] for s in sizes])), 1)],
           "num_ops": crop.num_ops, "batch_mode": int(plan.mode), "reps_per_window": args.reps, "windows": args.repeats,
           "device_equals_pillow_u8": same,
           "device_us_per_batch": {k: spread(v) for k, v in us.items() if k != "h2d_copy"},
           "device_us_three_kernels": round(dev_us, 1),
           "device_images_per_s_three_kernels": round(B / (dev_us * 1e-6), 1),
           "upload": {"bytes": up_bytes, "whole_images_bytes": int(nbytes.sum()), "us_per_copy": spread(us["h2d_copy"]),
                      "GBs": round(up_bytes / (statistics.median(us["h2d_copy"]) * 1e-6) / 1e9, 1)},
           "transform_call_ms_host_wall": spread(e2e_ms),
           "transform_call_images_per_s": round(B / (statistics.median(e2e_ms) * 1e-3), 1),
           "pil_one_core_ms_per_batch": spread(pil_ms),
           "pil_one_core_images_per_s": round(B / (pil_med * 1e-3), 1),
           "pil_16_cores_images_per_s_if_linear": round(16 * B / (pil_med * 1e-3), 1),
           "not_included": "JPEG decode; end-to-end training throughput (not measured); the torchvision parameter "
                           "mapping is unverified against torchvision itself"}
    if args.step_ms > 0:
        res["xl_train_bs120_step_ms_same_box"] = args.step_ms
        res["device_three_kernels_share_of_step"] = round(dev_us * 1e-3 / args.step_ms, 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
