"""SdP-Net forward benchmark on MI355X (BASELINE.json metric).

  python bench.py [--gpus N --steps K --warmup W] [--config m|xl|xl_train] [--dump-outputs DIR] [--full]

A plain run does what the headline figure needs and no more: set up, W warmup steps,
K timed steps, the outputs if asked for, one JSON line (metric, value, unit,
higher_is_better, dtype, ms_per_step = milliseconds per timed step, ...).  --full adds
the roofline, secondary and cpu_baseline measurements described at the end.

--dump-outputs DIR writes what the timed path returned in its last timed step as
float32 DIR/<name>.npy (forward: logits; xl_train: logits and loss; <name>_rank<r> when
N > 1; a fixed seeded sample when an array would pass 64 MB in all).  Weights and inputs
are seeded, so the same arguments give the same inputs in every run and two builds can
be compared output for output.

--gpus N > 1 started outside torch.distributed.run re-launches itself as a CHILD
`python -m torch.distributed.run --nproc-per-node N ... bench.py ...` (before any
GPU call in the parent) and exits with its code; under torch.distributed.run each
rank checks WORLD_SIZE == --gpus and rank 0 reports the RCCL world size and the
per-rank devices.  --dry-run runs the same launch / barrier / max-over-ranks
timing path on CPU with gloo and a trivial step (launcher test; no model).

Workload (BASELINE.json configs[1]): SdP-Net-M (12 blocks, d=768, patch 16,
canonical config SURVEY.md §0) bf16 eval forward in the reference's form --
an fp32 batch under torch.autocast("cuda", bfloat16) (training_tools.py:85) --
256 synthetic N(0,1) 224x224 images per GPU, random-init weights (reference
init), inputs resident in HBM before timing.  A step = one full forward of one
batch (logits), replayed from a HIP graph captured after warmup.  Multi-GPU: one
process per GPU, each its own independent batch shard (weak scaling), no
data-path collective; barrier + max-over-ranks timing only.

Integrity: the bench times the product library only.  It refuses a diagnostic
build (sdp_build_info() != 0: kernel-skip or stamp code compiled in) and a
non-zero kernel-skip mask, and records every SDPNET_* environment variable
(`config.knobs`, empty in a default run) and the loaded library's md5.

With --full, also reported on the same JSON line (each takes GPU or CPU runs of its own
after the headline's timed region):
  roofline     — dominant kernel (the bf16 fast GEMM, ~98 % of FLOPs): algorithmic
                 FLOPs per step / the union of its launch intervals in a replay of
                 the timed schedule, vs the dense bf16 MFMA peak.
  secondary    — (N=1, --no-secondary skips it) the other single-GPU BASELINE configs timed in the
                 same process after the headline: configs[2] XL bs512 forward and
                 configs[4]'s per-GPU XL training step (bs 120).
  cpu_baseline — the oracle (the reference's math in stock PyTorch CPU ops,
                 oracle/sdpnet_oracle.py) on this host's cores, bounded samples of
                 M bs16, configs[0] XXS bs4 and XL bs16, rank 0 at N=1 only
                 (--no-cpu-baseline skips it).
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "sdp-net_amd"))

METRIC = "images/sec fwd SdP-Net-M 224×224 bs=256 @1 GPU; scaling 1/2/4/8"
MFMA_BF16_PEAK_TFLOPS = 2516.6   # 256 CU x 2.4 GHz x 4096 FLOP/clk/CU (dense)
FAST_GEMM_NAMES = {9: "gemm_bf16_8ph", 14: "gemm_bf16_8ph"}

M_CFG = dict(embedding_dim=768, num_blocks=12, n_head=8, activation="gelu", embedding_activation="none",
             conv_kernel_size=7, patch_size=16, ffn_dropout=0.2, attn_dropout=0.2, output_classes=1000,
             conv_block_num=2, ff_multiplication_factor=4, max_image_size=[16, 16], max_num_registers=5,
             conv_first=True, head_output_from_register=True, simple_mlp_output=False, output_head_bias=False,
             normalize_qv=True, stochastic_depth_p=[0.0, 0.0], mixer_deptwise_bias=False, mixer_ffn_bias=False,
             conv_embedding=False, conv_embedding_kernel_size=5)


# BASELINE.json configs[2]: SdP-Net-XL (17 blocks, d=768, patch 14, 256 patches + 4 registers)
XL_CFG = dict(M_CFG, num_blocks=17, patch_size=14)
CONFIGS = {
    "m": dict(cfg=M_CFG, batch=256, name="SdP-Net-M", metric=METRIC,
              desc="SdP-Net-M eval forward (12 blocks, d=768, patch 16, 200 tokens)"),
    # BASELINE.json configs[4]: XL training step, 120 images per GPU (global 960 at DP=8)
    "xl_train": dict(cfg=dict(XL_CFG), batch=120, name="SdP-Net-XL", train=True,
                     metric="images/sec train step (fwd+bwd+AdamW) SdP-Net-XL 224x224 bs=120/GPU (BASELINE.json configs[4])",
                     desc="SdP-Net-XL training step (17 blocks, d=768, patch 14, 260 tokens): bf16 autocast forward, "
                          "label-smoothed CE, backward, GradScaler unscale + clip_grad_norm_(5) + AdamW"),
    "xl": dict(cfg=XL_CFG, batch=512, name="SdP-Net-XL",
               metric="images/sec fwd SdP-Net-XL 224×224 bs=512 @1 GPU (BASELINE.json configs[2])",
               desc="SdP-Net-XL eval forward (17 blocks, d=768, patch 14, 260 tokens)"),
}


def flops_per_image(cfg, img=224, num_registers=3):
    """2*MAC over every conv (incl. depthwise), GEMM and attention QK^T + PV
    (M = 88.933 GF)."""
    C, p, k = cfg["embedding_dim"], cfg["patch_size"], cfg["conv_kernel_size"]
    P = (img // p) ** 2
    R = min(num_registers + 1, cfg["max_num_registers"])
    N = R + P
    mf = cfg["ff_multiplication_factor"]
    patch = 2 * P * C * 3 * p * p
    mixer = 2 * P * C * k * k + 2 * P * C * C + 2 * 2 * P * C * 4 * C
    enc = 2 * N * C * 3 * C + 2 * N * C * C + 2 * 2 * N * C * mf * C + 2 * 2 * N * N * C
    ncls = cfg["output_classes"]
    head = 2 * C * ncls + 2 * ncls * ncls
    return patch + cfg["num_blocks"] * (cfg["conv_block_num"] * mixer + enc) + enc + head


def measured_traffic(kernel, config="m"):
    """HBM bytes per launch of `kernel` from the newest committed PMC summary
    (profiles/r*_gemm_traffic.json, written by tools/prof_summary.py from separate
    rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this same bench command,
    gfx950 correction bytes = (2*FETCH_SIZE + WRITE_SIZE) * 1024).  PMC counters
    cannot be read live without the profiler, hence the file."""
    import glob
    for f in sorted(glob.glob(os.path.join(REPO, "profiles", "r*_gemm_traffic.json")), reverse=True):
        try:
            d = json.load(open(f))
        except (OSError, ValueError):
            continue
        if d.get("kernel") == kernel and d.get("config", "m") == config:
            return int(d["hbm_bytes_per_launch"]), os.path.relpath(f, REPO), traffic_staleness(d)
    return None, None, None


def gemm_source_sha16():
    """Hash of the sources the fast GEMM is built from (its kernel file and the shared header)."""
    import hashlib
    h = hashlib.sha256()
    for rel in ("sdp-net_amd/csrc/gemm.hip", "sdp-net_amd/csrc/common.h"):
        with open(os.path.join(REPO, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def traffic_staleness(d):
    """Ties a committed PMC traffic summary to the build it describes (VERDICT r05 'what's weak' 7):
    the summary records the GEMM source hash and the library md5 it was measured with.  True when
    the GEMM source differs from the one built here, False when it matches, None for a summary
    that predates the record (unknown)."""
    src = d.get("gemm_src_sha16")
    if not src:
        return None
    return src != gemm_source_sha16()


XXS_CFG = dict(M_CFG, embedding_dim=128, num_blocks=7)   # BASELINE.json configs[0]


def cpu_baseline(cpu_sds, headline="SdP-Net-M", seconds=10.0):
    """The oracle's fp32 eval forward on this host's cores: M bs16 for ~`seconds`
    (the headline's CPU counterpart), configs[0] XXS bs4 for ~5 s, XL bs16 for one batch.
    cpu_sds: {name: (state_dict, cfg)} built from the same seeded models as the GPU runs."""
    import torch
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import sdpnet_oracle as orc
    threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or len(os.sched_getaffinity(0))
    threads = max(1, min(threads, len(os.sched_getaffinity(0))))
    torch.set_num_threads(threads)

    def timed(sd, cfg, bs, secs, min_batches=1):
        x = torch.randn(bs, 3, 224, 224, generator=torch.Generator().manual_seed(7))
        orc.forward(x[:1], sd, cfg)  # warm
        n, t0 = 0, time.perf_counter()
        while True:
            orc.forward(x, sd, cfg)
            n += bs
            if n >= min_batches * bs and time.perf_counter() - t0 >= secs:
                break
        return n, time.perf_counter() - t0

    import glob
    ratio = None  # oracle speed / the reference's own CPU forward, measured in the build container
    for f in sorted(glob.glob(os.path.join(REPO, "profiles", "r*_cpu_ratio.json")), reverse=True):
        try:
            ratio = json.load(open(f))
            ratio["source"] = os.path.relpath(f, REPO)
            break
        except (OSError, ValueError):
            continue
    plan = [("SdP-Net-M", 16, 0.0), ("SdP-Net-XXS", 4, 5.0), ("SdP-Net-XL", 16, 0.0)]
    plan = [(nm, bs, seconds if nm == headline else secs) for nm, bs, secs in plan]
    res = {}
    for name, bs, secs in plan:
        if name not in cpu_sds:
            continue
        sd, cfg = cpu_sds[name]
        n, dt = timed(sd, cfg, bs, secs)
        res[name] = {"value": round(n / dt, 3), "unit": "images/sec", "batch": bs, "images": n,
                     "seconds": round(dt, 2)}
    m = res.get(headline)
    return {"value": m["value"] if m else None, "unit": "images/sec", "cores": threads, "kind": "port",
            "port_vs_reference": ratio, "per_config": res,
            "sample": "fp32 eval forward of the oracle (oracle/sdpnet_oracle.py: the reference math in stock torch "
                      "CPU ops) on this host's cores: %s in batches of 16 for ~%.0f s (value); per_config: configs[0] "
                      "XXS bs4 for ~5 s, M / XL one batch of 16 unless headline" % (headline, seconds)}


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n):
    """Parent side of --gpus N: run N ranks under torch.distributed.run as a child
    process (model_train.py:33-42 is the reference's rank setup: one process per GPU,
    LOCAL_RANK from the launcher).  No GPU call happens in this process."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def dry_run(args, world, rank):
    """CPU/gloo rehearsal of the multi-rank timing path (no model, no GPU)."""
    import torch
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(REPO, "sdp-net_amd"))
    import sharding
    if world > 1:
        dist.init_process_group("gloo")
    lo, hi = sharding.shard_bounds(args.batch * world, world, rank)
    x = torch.randn(hi - lo, 64)
    w = torch.randn(64, 64)
    for _ in range(args.warmup):
        x @ w
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        x @ w
    if world > 1:
        dist.barrier()
    el = sharding.max_over_ranks(time.perf_counter() - t0)
    total = int(sharding.sum_over_ranks((hi - lo) * args.steps))
    ranks = [None] * world
    if world > 1:
        dist.all_gather_object(ranks, {"rank": rank, "pid": os.getpid(), "shard": [lo, hi]})
    else:
        ranks = [{"rank": 0, "pid": os.getpid(), "shard": [lo, hi]}]
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": world, "steps": args.steps, "value": round(total / el, 2),
                          "comm_world": dist.get_world_size() if world > 1 else 1,
                          "backend": dist.get_backend() if world > 1 else None,
                          "global_batch": args.batch * world, "ranks": ranks}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def check_library(L, env):
    """The integrity gate (VERDICT r04 'what's weak' 6): returns the SDPNET_* knobs of this run; refuses
    (SystemExit) a diagnostic library or a non-zero kernel-skip mask, either of which could leave work
    out of the timed region.  L: the loaded ctypes library (sdpnet_hip.lib()); env: os.environ."""
    knobs = {k: v for k, v in sorted(env.items()) if k.startswith("SDPNET_")}
    flags = int(L.sdp_build_info())
    if flags:
        raise SystemExit(f"bench.py: refusing to time a diagnostic library (sdp_build_info() = {flags}: "
                         "kernel-skip / stamp code compiled in); build the product library (make -C sdp-net_amd/csrc)")
    mask = int(L.sdp_debug_skip(0))
    if mask or knobs.get("SDPNET_DEBUG_SKIP", "0").strip() not in ("", "0"):
        raise SystemExit(f"bench.py: refusing to time with a kernel-skip mask (library mask {mask}, "
                         f"SDPNET_DEBUG_SKIP={knobs.get('SDPNET_DEBUG_SKIP')!r}): results would be wrong")
    return knobs


def library_record(env=os.environ):
    import hashlib
    import sdpnet_hip as sp
    knobs = check_library(sp.lib(), env)
    with open(sp.LIB_PATH, "rb") as f:
        md5 = hashlib.md5(f.read()).hexdigest()
    return {"knobs": knobs, "lib": os.path.relpath(os.path.realpath(sp.LIB_PATH), REPO), "lib_md5": md5}


def _progress(rank, msg):
    """One progress line on stderr (rank 0): long profiled runs print as they go."""
    if rank == 0:
        print(f"[bench] {time.strftime('%H:%M:%S')} {msg}", file=sys.stderr, flush=True)


DUMP_LIMIT_BYTES = 60 * 10 ** 6   # array data; with the .npy headers the files stay under 64 MB


def dump_outputs(path, arrays, world, rank):
    """--dump-outputs: each tensor of `arrays` as float32 `path`/<name>.npy (<name>_rank<r> at N > 1).
    Together they stay under DUMP_LIMIT_BYTES: an array above its share is cut to a fixed, seeded
    sample of its elements (flattened, in index order), the same in every run."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    share = DUMP_LIMIT_BYTES // (4 * max(1, len(arrays)))
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        if a.size > share:
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, share, replace=False))]
        np.save(os.path.join(path, name + (f"_rank{rank}" if world > 1 else "") + ".npy"), a)


def train_step_bench(C, B, steps, warmup, dev, world, rank, local, global_batch, dump=None):
    """BASELINE.json configs[4]: one training step = bf16-autocast forward + label-smoothed CE
    (training_tools.py:85-88) + backward (DDP bucketed gradient all-reduce over RCCL when
    N > 1, training_tools.py:36, :91) + GradScaler unscale / clip_grad_norm_(5) / AdamW
    (training_tools.py:94-99, fused into one HIP kernel) on each rank's B synthetic images.
    Returns the line's fields (timing = barrier + synchronize on both sides, max over ranks)."""
    import torch
    import torch.distributed as dist
    import model as sdp
    import sdpnet_train
    import sharding
    cfg = C["cfg"]
    torch.manual_seed(231424314)  # model_train.py:61
    m = sdp.MainModel.from_dict(**cfg).to(dev).train()
    net = m
    if world > 1:
        net = torch.nn.parallel.DistributedDataParallel(m, device_ids=[local])
    opt = sdpnet_train.AdamW(m.parameters(), lr=0.0015, weight_decay=0.05)   # model_config_vit.yaml:49-51
    g = torch.Generator(device="cpu").manual_seed(1000 + rank)
    x = torch.randn(B, 3, 224, 224, generator=g).to(dev)
    y = torch.randint(0, cfg["output_classes"], (B,), generator=g).to(dev)

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = net(x)
            loss = sdpnet_train.cross_entropy(out, y, 0.1)
        opt.scale(loss).backward()              # GradScaler.scale on the device scale (no sync)
        opt.step(grad_scale=None, max_norm=5.0)  # unscale / inf check / clip / AdamW / scale update
        return loss, out

    _progress(rank, f"{C['name']} training bs {B}: model built, {max(1, warmup)} warmup steps")
    for _ in range(max(1, warmup)):
        loss, logits = step()
    torch.cuda.synchronize()
    _progress(rank, "warmup done")
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    taken0 = float(opt._steps[0])
    t0 = time.perf_counter()
    for _ in range(steps):
        loss, logits = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    el = sharding.max_over_ranks(time.perf_counter() - t0, device=dev)
    total = int(sharding.sum_over_ranks(B * steps, device=dev))
    assert torch.isfinite(loss).all()
    # GradScaler skips (inf/nan grads) did no optimizer work: count them, none expected
    skipped = int(steps - (float(opt._steps[0]) - taken0))
    assert skipped == 0, f"{skipped} optimizer steps skipped by the GradScaler inside the timed region"
    if dump:
        dump_outputs(dump, {"logits": logits, "loss": loss}, world, rank)
    gf = 3 * flops_per_image(cfg) / 1e9   # forward + dX + dW GEMMs (3x forward)
    value = total / el
    out = {
        "metric": C["metric"], "value": round(value, 2), "unit": "images/sec", "n_gpus": world,
        "steps": steps, "warmup": warmup, "ms_per_step": round(1e3 * el / steps, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
        "data": "synthetic N(0,1) 224x224 images + random labels resident in HBM; random-init weights",
        "config": {"workload": C["desc"], "global_batch": global_batch, "per_gpu_batch": B,
                   "parallelism": f"dp{world}" + (" DDP bucketed grad all-reduce over RCCL" if world > 1 else "")},
        "model_flops_per_image_gf": round(gf, 3),
        "model_mfma_frac": round(value * gf * 1e9 / (world * MFMA_BF16_PEAK_TFLOPS * 1e12), 4),
        "skipped_steps": skipped, "grad_scale": float(opt.scaler[0]),
        "loss": round(float(loss.detach()), 4), "peak_mem_gb": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 1),
    }
    del m, net, opt, x, y, logits
    return out


def train_bench(args, C, world, rank, local):
    import torch
    import torch.distributed as dist
    import sharding
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)
    rec = library_record()
    lo, hi = sharding.shard_bounds(args.batch * world, world, rank)
    out = train_step_bench(C, hi - lo, args.steps, args.warmup, dev, world, rank, local, args.batch * world,
                           dump=args.dump_outputs)
    out["config"].update(rec)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def forward_bench(C, B, steps, warmup, dev, world, rank, streams=0, graph=True, roofline=True, config="m",
                  keep_cpu_sd=True, dump=None):
    """One config's eval forward: an fp32 batch resident in HBM under torch.autocast("cuda", bf16)
    (the reference's bf16 forward, training_tools.py:85; the patch kernel reads the fp32 image),
    W warmup forwards, a HIP graph of one forward (both sub-batch streams), K timed replays
    bracketed by barrier + synchronize, max over ranks.  Returns (fields, cpu state_dict or None)."""
    import torch
    import torch.distributed as dist
    import model as sdp
    import sdpnet_hip as sp
    import sharding
    cfg = C["cfg"]
    torch.manual_seed(231424314)  # model_train.py:61
    m = sdp.MainModel.from_dict(**cfg).eval()
    if streams > 0:
        m.num_streams = streams
    cpu_sd = {k: v.detach().clone() for k, v in m.state_dict().items()} if keep_cpu_sd and rank == 0 and world == 1 else None
    m = m.to(dev)
    g = torch.Generator(device="cpu").manual_seed(1000 + rank)
    x = torch.randn(B, 3, 224, 224, generator=g).to(dev)   # fp32, resident in HBM

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return m(x)

    _progress(rank, f"{C['name']} bs {B}: model built, {max(1, warmup)} warmup forwards")
    for _ in range(max(1, warmup)):
        y = step()
    torch.cuda.synchronize()
    _progress(rank, "warmup done")
    pgraph = None
    if graph:
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()
        torch.cuda.current_stream().wait_stream(s)
        pgraph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(pgraph):
            y = step()
        pgraph.replay()
        torch.cuda.synchronize()
    run = pgraph.replay if pgraph is not None else step

    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        r = run()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    el = sharding.max_over_ranks(time.perf_counter() - t0, device=dev)
    total_imgs = int(sharding.sum_over_ranks(B * steps, device=dev))
    if pgraph is None:
        y = r   # eager: the last timed step's own result (a replay writes into y)
    assert y.dtype == torch.bfloat16 and torch.isfinite(y.float()).all()
    value = total_imgs / el
    ms_step = 1e3 * el / steps
    gf = flops_per_image(cfg) / 1e9
    tokens = (224 // cfg["patch_size"]) ** 2 + min(4, cfg["max_num_registers"])
    out = {
        "metric": C["metric"], "value": round(value, 2), "unit": "images/sec", "n_gpus": world,
        "steps": steps, "warmup": warmup, "ms_per_step": round(ms_step, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
        "data": "synthetic N(0,1) 224x224 fp32 images resident in HBM, bf16 autocast; random-init weights "
                "(reference init)",
        "config": {"workload": C["desc"] + ", torch.autocast bf16 (bf16 storage / fp32 accumulate)"
                               + (", eager launches" if not graph else ", HIP-graph replay"),
                   "streams_per_gpu": m._num_streams(B), "per_gpu_batch": B, "image": 224, "tokens": tokens},
        "model_flops_per_image_gf": round(gf, 3),
        "model_mfma_frac": round(value * gf * 1e9 / (world * MFMA_BF16_PEAK_TFLOPS * 1e12), 4),
    }
    _progress(rank, f"{steps} timed forwards: {value:.1f} img/s")
    if dump:
        dump_outputs(dump, {"logits": y}, world, rank)
    if roofline:
        out["roofline"] = gemm_roofline(step, dev, ms_step, config)
        _progress(rank, "roofline replays done")
    del pgraph, m, x, y, r
    return out, cpu_sd


def gemm_roofline(step, dev, ms_step, config, prof_steps=1):
    """Dominant-kernel roofline, measured on the timed schedule itself.  A second graph of the same
    step (same sub-batch streams, same kernels) is captured with the library's launch timeline on:
    every fast-GEMM launch folds its first-workgroup start and last-workgroup end (device clock,
    s_memrealtime at 100 MHz) into its own slot, which works inside a replayed graph where HIP
    events cannot be recorded.  Per replay: the launch intervals, their UNION (the wall time the
    GEMMs occupy in this schedule; two sub-batch streams overlap GEMMs with each other and with the
    other kernels) and the replay's own device-time span.  The timed graph itself has no timeline."""
    import torch
    import sdpnet_hip as sp
    tl = torch.empty(2 * 4096, dtype=torch.int64, device=dev)
    sp.gemm_timeline_begin(tl)
    try:
        pg = torch.cuda.CUDAGraph()
        s2 = torch.cuda.Stream(device=dev)
        s2.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s2):
            with torch.cuda.graph(pg):
                for _ in range(prof_steps):
                    step()
    finally:
        launches = sp.gemm_timeline_end()
    torch.cuda.current_stream().wait_stream(s2)
    tick_ms = sp.TIMELINE_TICK_NS * 1e-6
    samples = []
    for _ in range(5):
        tl[0::2].fill_(-1)   # UINT64_MAX: atomicMin start
        tl[1::2].fill_(0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pg.replay()
        e1.record()
        torch.cuda.synchronize()
        v = tl[:2 * len(launches)].view(-1, 2).cpu().numpy().astype("uint64")
        iv = [(int(v[i, 0]), int(v[i, 1])) for i, *_ in launches]
        assert all(a_ < b_ for a_, b_ in iv), "a timed GEMM launch recorded no interval"
        big = [(a_, b_) for (a_, b_), (_, M_, *_r) in zip(iv, launches) if M_ >= 1024]
        big.sort()
        union, cur = 0, None
        for a_, b_ in big:
            if cur is None or a_ > cur[1]:
                if cur is not None:
                    union += cur[1] - cur[0]
                cur = [a_, b_]
            else:
                cur[1] = max(cur[1], b_)
        if cur is not None:
            union += cur[1] - cur[0]
        samples.append(dict(union_ms=union * tick_ms / prof_steps, replay_ms=e0.elapsed_time(e1) / prof_steps,
                            durs=[(b_ - a_) * tick_ms for a_, b_ in iv]))
    samples.sort(key=lambda d: d["union_ms"])
    med = samples[len(samples) // 2]
    del pg
    fast_fl = sum(f for _, M_, _n, _k, f, _b in launches if M_ >= 1024) / prof_steps
    fast_by = sum(b_ for _, M_, _n, _k, _f, b_ in launches if M_ >= 1024) / prof_steps
    fast_n = sum(1 for _, M_, *_r in launches if M_ >= 1024) // prof_steps
    fast_ms = sum(d for d, (_, M_, *_r) in zip(med["durs"], launches) if M_ >= 1024) / prof_steps
    per_shape = {}
    for d, (_, M_, N_, K_, f, _b) in zip(med["durs"], launches):
        e = per_shape.setdefault(f"{M_}x{N_}x{K_}", dict(launches=0, ms=0.0, fl=0.0))
        e["launches"] += 1
        e["ms"] += d
        e["fl"] += f
    per_shape = {k: dict(launches=e["launches"], avg_us=round(1e3 * e["ms"] / e["launches"], 2),
                         tflops_co_running=round(e["fl"] / (e["ms"] * 1e-3) / 1e12, 1))
                 for k, e in per_shape.items()}
    union_ms_step = med["union_ms"]
    # the GEMM union is measured on a replay of the timed schedule; when that replay runs slower than
    # the timed steps (the union exceeds the step, e.g. at 4 sub-batch streams) the step itself is the
    # denominator, i.e. the no-overlap lower bound
    union_ok = union_ms_step <= ms_step * 1.02
    achieved = fast_fl / ((union_ms_step if union_ok else ms_step) * 1e-3) / 1e12
    per_launch_tf = fast_fl / (fast_ms * 1e-3) / 1e12 if fast_ms else 0.0
    kname = FAST_GEMM_NAMES.get(sp.lib().sdp_gemm_set_fast_kernel(0), "?")
    traffic, traffic_src, stale = measured_traffic(kname, config) if config in ("m", "xl") else (None, None, None)
    return {"bound": "mfma", "kernel": kname,
            "achieved": round(achieved, 1), "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
            "achieved_basis": ("GEMM FLOPs per step / union of the GEMM launch intervals per step, "
                               "measured in a graph replay of the timed schedule (same sub-batch streams "
                               "and kernels; device-clock launch timeline, median of 5 replays)") if union_ok
                              else ("GEMM FLOPs per step / ms_per_step (the profiled replay's GEMM union "
                                    "exceeded the timed step by > 2 %, so the lower bound is reported)"),
            "gemm_union_ms_per_step": round(union_ms_step, 3),
            "ms_per_step": round(ms_step, 3),
            "union_le_step": bool(union_ms_step <= ms_step),
            "profiled_replay_ms": round(med["replay_ms"], 3),
            "lower_bound_tflops": round(fast_fl / (ms_step * 1e-3) / 1e12, 1),
            "lower_bound_basis": "GEMM FLOPs per step / ms_per_step (no overlap assumption)",
            "per_launch_tflops": round(per_launch_tf, 1),
            "frac": round(achieved / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": traffic,
            "traffic_unit": "bytes per launch, L2-to-fabric (PMC 2*FETCH_SIZE+WRITE_SIZE; Infinity Cache hits "
                            "included)", "traffic_source": traffic_src,
            "traffic_stale": stale,
            "algorithmic_bytes_per_launch": int(fast_by / max(1, fast_n)),
            "launches_per_step": fast_n,
            "avg_launch_us": round(1e3 * fast_ms / max(1, fast_n), 2),
            "avg_launch_basis": "device-clock launch durations in the 2-stream graph replay (co-running "
                                "launches overlap, so these are not solo times)",
            "algorithmic_gflop_per_launch": round(fast_fl / max(1, fast_n) / 1e9, 3),
            "per_shape": per_shape}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", choices=sorted(CONFIGS), default="m",
                    help="m = the BASELINE metric's workload (default); xl = configs[2]; xl_train = configs[4]")
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (0 = the config's: M 256, XL 512)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as float32 DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also measure the GEMM roofline, the secondary configs and the CPU baseline")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true",
                    help="with --full: skip the XL forward / XL training lines timed after the headline at N=1")
    ap.add_argument("--secondary-steps", type=int, default=20)
    ap.add_argument("--prof-steps", type=int, default=1, help="forwards per profiled graph replay (roofline)")
    ap.add_argument("--streams", type=int, default=0, help="sub-batch streams per GPU (0 = model default)")
    ap.add_argument("--dry-run", action="store_true", help="CPU/gloo rehearsal of the launch + timing path")
    args = ap.parse_args()
    C = CONFIGS[args.config]
    cfg = C["cfg"]
    if args.batch <= 0:
        args.batch = C["batch"]
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: WORLD_SIZE={world} but --gpus {args.gpus}: launch N ranks with --gpus N")
    if args.dry_run:
        return dry_run(args, world, rank)
    if C.get("train"):
        return train_bench(args, C, world, rank, local)

    import torch
    import torch.distributed as dist
    import sharding

    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)
    comm_world = dist.get_world_size() if world > 1 else 1
    if comm_world != world:
        raise SystemExit(f"bench.py: RCCL world size {comm_world} != {world}")
    if world > 1:
        devs = [None] * world
        dist.all_gather_object(devs, f"rank{rank}:cuda:{local}:{torch.cuda.get_device_name(dev)}")
    else:
        devs = [f"rank0:cuda:{local}:{torch.cuda.get_device_name(dev)}"]
    rec = library_record()

    # weak scaling: the global batch is world x per-GPU batch, each rank owns one
    # contiguous shard (images are independent, no collective on the data path)
    lo, hi = sharding.shard_bounds(args.batch * world, world, rank)
    out, cpu_sd = forward_bench(C, hi - lo, args.steps, args.warmup, dev, world, rank, streams=args.streams,
                                graph=not args.no_graph, roofline=args.full, config=args.config,
                                keep_cpu_sd=args.full and not args.no_cpu_baseline, dump=args.dump_outputs)
    out["config"].update({"global_batch": args.batch * world,
                          "parallelism": f"dp{world} independent batch shards (no collective)",
                          "comm_world": comm_world, "comm_backend": "nccl (RCCL)" if world > 1 else None,
                          "devices": devs, **rec})
    out["cpu_baseline"] = None
    cpu_sds = {}
    if cpu_sd is not None:
        cpu_sds[C["name"]] = (cpu_sd, cfg)
    if args.full and world == 1 and not args.no_secondary and args.config == "m":
        # configs[2] and configs[4] under the same clock, after the headline's timed region
        sec = {}
        ks = max(1, min(args.secondary_steps, args.steps))
        torch.cuda.empty_cache()
        xl, xl_sd = forward_bench(CONFIGS["xl"], CONFIGS["xl"]["batch"], ks, min(args.warmup, 3), dev, 1, rank,
                                  graph=not args.no_graph, roofline=True, config="xl")
        sec["xl_fwd"] = {k: xl[k] for k in ("metric", "value", "unit", "ms_per_step", "steps", "model_mfma_frac",
                                           "model_flops_per_image_gf", "roofline")}
        sec["xl_fwd"]["per_gpu_batch"] = CONFIGS["xl"]["batch"]
        if xl_sd is not None:
            cpu_sds["SdP-Net-XL"] = (xl_sd, XL_CFG)
        torch.cuda.empty_cache()
        tr = train_step_bench(CONFIGS["xl_train"], CONFIGS["xl_train"]["batch"], ks, min(args.warmup, 3), dev, 1, rank,
                              local, CONFIGS["xl_train"]["batch"])
        sec["xl_train"] = {k: tr[k] for k in ("metric", "value", "unit", "ms_per_step", "steps", "model_mfma_frac",
                                             "model_flops_per_image_gf", "skipped_steps", "peak_mem_gb")}
        sec["xl_train"]["per_gpu_batch"] = CONFIGS["xl_train"]["batch"]
        out["secondary"] = sec
        torch.cuda.empty_cache()
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and cpu_sds:
        if args.config == "m":
            torch.manual_seed(231424314)
            import model as sdp
            cpu_sds["SdP-Net-XXS"] = (sdp.MainModel.from_dict(**XXS_CFG).state_dict(), XXS_CFG)
        out["cpu_baseline"] = cpu_baseline(cpu_sds, headline=C["name"])
        cb = out["cpu_baseline"]["value"]
        out["gpu_over_cpu"] = round(out["value"] / cb, 1) if cb else None
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
