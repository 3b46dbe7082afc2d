"""Measurements of the hybrid JPEG decoder (profiles/device_jpeg.md).

  python tools/jpeg_bench.py [--images 256] [--threads 8,16] [--out FILE.json] [--host-only]

Set: synthetic 500 x 375 photos (gradients, edges, noise), quality 90, 4:2:0, about 83 kB each.
Baseline everywhere: Pillow's full decode (Image.open(...).convert("RGB") -> np.asarray),
``_as_rgb_u8`` and the upload of the pixels, which is what the transforms did before.

* host, one core: ms per image of sdp_jpeg_entropy_decode against Pillow's full decode, in
  interleaved windows (min - max over the windows); then both on a thread pool of 1 / 4 / 8 / 16;
* device: event time of sdp_jpeg_reconstruct for the batch, its HBM bytes (coefficients read,
  planar samples written and read again, pixels written) against the memory roofline;
* upload: bytes and time of the coefficient upload against the upload of decoded pixels;
* end to end: images/s of preprocess.batches -> SdP-Net-M bf16 forward from JPEG bytes against
  the same from Pillow-decoded images, the decode on the same number of threads.
The GPU sections need a GPU (``--host-only`` leaves them out; it does not estimate them)."""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sdp-net_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402
from PIL import Image  # noqa: E402
import PIL  # noqa: E402

import preprocess  # noqa: E402
import sdpnet_hip as sp  # noqa: E402

HBM_PEAK_GBS = 8000.0
H, W = 375, 500


def synth_photo(seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ch = []
    for k in range(3):
        a = 127 + 70 * np.sin(xx * (0.021 + 0.01 * k) + yy * (0.017 + 0.006 * k) + seed + k)
        a += 40 * np.cos(xx * 0.09 - yy * 0.05 * (k + 1))
        a += 50 * ((xx + 2 * yy + 5 * k + seed * 7) % 61 < 23)
        a += rng.normal(0, 8.0, (H, W))
        ch.append(np.clip(a, 0, 255))
    return np.stack(ch, axis=2).astype(np.uint8)


def make_set(n: int, distinct: int = 32):
    files = []
    for k in range(min(n, distinct)):
        buf = io.BytesIO()
        Image.fromarray(synth_photo(k)).save(buf, "JPEG", quality=90, subsampling=2)
        files.append(buf.getvalue())
    return [files[k % len(files)] for k in range(n)]


def pillow_decode(data) -> np.ndarray:
    return preprocess._as_rgb_u8(Image.open(io.BytesIO(data)))


def span(v):
    return {"min": round(min(v), 4), "max": round(max(v), 4), "windows": len(v)}


def host_one_core(files, windows=6, per_window=48):
    n = int(sp.jpeg_probe(files[0])[1][10])
    coef = np.zeros(n, np.int16)
    qt = np.zeros(192, np.uint8)
    sub = files[:per_window]
    ours, pil = [], []
    for f in sub[:8]:
        sp.jpeg_entropy_decode(f, coef, qt)
        pillow_decode(f)
    for _ in range(windows):
        t = time.perf_counter()
        for f in sub:
            assert sp.jpeg_entropy_decode(f, coef, qt)[0] == 0
        ours.append((time.perf_counter() - t) / len(sub) * 1e3)
        t = time.perf_counter()
        for f in sub:
            pillow_decode(f)
        pil.append((time.perf_counter() - t) / len(sub) * 1e3)
    return {"entropy_decode_ms_per_image": span(ours), "pillow_full_decode_ms_per_image": span(pil)}


def host_pool(files, windows=5):
    n = int(sp.jpeg_probe(files[0])[1][10])
    out = {}
    for threads in (1, 4, 8, 16):
        bufs = [(np.zeros(n, np.int16), np.zeros(192, np.uint8)) for _ in files]
        ours, pil = [], []
        with ThreadPoolExecutor(threads) as pool:
            for _ in range(windows):
                t = time.perf_counter()
                rcs = list(pool.map(lambda k: sp.jpeg_entropy_decode(files[k], *bufs[k])[0], range(len(files))))
                ours.append(len(files) / (time.perf_counter() - t))
                assert not any(rcs)
                t = time.perf_counter()
                list(pool.map(pillow_decode, files))
                pil.append(len(files) / (time.perf_counter() - t))
        out[str(threads)] = {"entropy_decode_images_per_s": span(ours), "pillow_full_decode_images_per_s": span(pil)}
    return out


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def device_sections(files, threads):
    dev = torch.device("cuda")
    B = len(files)
    infos = [sp.jpeg_probe(f)[1] for f in files]
    n = np.array([int(i[10]) for i in infos], np.int64)
    off = np.zeros(B, np.int64)
    off[1:] = np.cumsum(n)[:-1]
    n_coef, n_pix = int(n.sum()), B * H * W * 3
    Wd = sp.JPEG_DESC_WORDS
    desc = np.zeros(B * Wd, np.int32)
    host = torch.empty(2 * n_coef, dtype=torch.uint8, pin_memory=True)
    coef = host.numpy().view(np.int16)
    for k, f in enumerate(files):
        q = desc[k * Wd:(k + 1) * Wd]
        assert sp.jpeg_entropy_decode(f, coef[off[k]:off[k] + n[k]], q[sp.JPEG_DESC_QT:].view(np.uint8))[0] == 0
        sp.jpeg_fill_desc(q, infos[k], off[k], off[k], k * H * W * 3)
    coef_d = host.to(dev).view(torch.int16)
    desc_d = torch.from_numpy(desc).to(dev)
    ws = torch.empty(n_coef, dtype=torch.uint8, device=dev)
    pix = torch.empty(n_pix, dtype=torch.uint8, device=dev)

    def run():
        sp.jpeg_reconstruct(coef_d, desc, desc_d, B, ws, pix)

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = [event_ms(run, 20) for _ in range(5)]
    want = np.concatenate([pillow_decode(f).reshape(-1) for f in files[:8]])
    assert np.array_equal(pix[:want.size].cpu().numpy(), want), "reconstruct differs from Pillow"
    hbm = 2 * n_coef + 2 * n_coef + n_pix   # coefficients read; samples written and read; pixels written
    best = min(ms)
    rec = {"batch": B, "reconstruct_ms": span(ms), "hbm_bytes": hbm,
           "achieved_GBs_at_min": round(hbm / (best * 1e-3) / 1e9, 1), "hbm_peak_GBs": HBM_PEAK_GBS,
           "frac_of_memory_roofline_at_min": round(hbm / (best * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
           "images_per_s_at_min": round(B / (best * 1e-3), 1)}

    pixels_host = torch.empty(n_pix, dtype=torch.uint8, pin_memory=True)
    up_c = [event_ms(lambda: host.to(dev, non_blocking=True), 5) for _ in range(5)]
    up_p = [event_ms(lambda: pixels_host.to(dev, non_blocking=True), 5) for _ in range(5)]
    upload = {"coefficient_bytes": 2 * n_coef, "pixel_bytes": n_pix, "coefficient_upload_ms": span(up_c),
              "pixel_upload_ms": span(up_p)}

    # end to end: batches -> SdP-Net-M bf16 forward
    import bench
    import model as sdp
    torch.manual_seed(231424314)
    m = sdp.MainModel.from_dict(**bench.CONFIGS["m"]["cfg"]).eval().to(dev)
    t_jpeg = preprocess.val_transforms(device=dev)
    t_pil = preprocess.val_transforms(device=dev)
    data = files * 8
    pool = None

    def from_bytes():
        return ((f, 0) for f in data)

    def from_pillow():   # the decode on the same number of threads, a batch ahead at most
        for s in range(0, len(data), B):
            for a in pool.map(pillow_decode, data[s:s + B]):
                yield a, 0

    def epoch(source, t):
        t0 = time.perf_counter()
        seen = 0
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            for x, _ in preprocess.batches(source(), t, batch_size=B):
                y = m(x)
                seen += x.shape[0]
        torch.cuda.synchronize()
        assert torch.isfinite(y).all().item()
        return seen / (time.perf_counter() - t0)

    e2e = []
    for n_threads in threads:
        t_jpeg.jpeg_decoder = preprocess.JpegDecoder(dev, num_threads=n_threads)
        pool = ThreadPoolExecutor(n_threads)
        epoch(from_bytes, t_jpeg), epoch(from_pillow, t_pil)   # warm-up
        a, b = [], []
        for _ in range(5):
            a.append(epoch(from_bytes, t_jpeg))
            b.append(epoch(from_pillow, t_pil))
        pool.shutdown()
        e2e.append({"threads": n_threads, "images_per_epoch": len(data), "from_jpeg_bytes_images_per_s": span(a),
                    "from_pillow_images_images_per_s": span(b)})
    return {"reconstruct": rec, "upload": upload, "end_to_end_m_bf16": e2e}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--threads", default="8,16", help="decode threads of the end-to-end runs, comma-separated")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    files = make_set(args.images)
    res = {"pillow": PIL.__version__, "images": len(files), "image_wh": [W, H],
           "mean_file_bytes": int(np.mean([len(f) for f in files])), "cpus_used": len(os.sched_getaffinity(0)),
           "host_one_core": host_one_core(files), "host_pool": host_pool(files)}
    if not args.host_only:
        if not torch.cuda.is_available():
            raise SystemExit("jpeg_bench: the device sections need a GPU (--host-only leaves them out)")
        res.update(device_sections(files, [int(v) for v in args.threads.split(",")]))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
