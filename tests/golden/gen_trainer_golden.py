"""Generate tests/golden/trainer_ref.npz — CONTAINER-ONLY tool.

Imports the reference (/root/reference, read-only) the way gen_golden.py does (empty ``wandb``
stub) plus its ``training_tools`` module, and records data only:

  (a) ``bce/...``  the reference's ``BCEWithLogitsLoss(num_classes=K, label_smoothing)``
      (training_utilities.py:95-107) loss and autograd dlogits on seeded fp32 logits, B 5,
      K 10 and K 1000, hard labels and MixUp-style soft targets, label smoothing 0 and 0.1;
  (b) ``ema/<key>``  the state of the reference's ``EMA_model`` (training_tools.py:282-302,
      decay 0.999) after two ``update_parameters`` calls on the ``train_cf`` model, every
      floating entry of the model perturbed by ``perturbation(key, shape, call)`` before each call;
  (c) ``lr``  the learning rate of ``return_scheduler_optimizer`` (training_tools.py:230-259)
      at epochs 0..12: lr 0.0015, ConstantLR(0.001, 2), LinearLR(0.001, 5),
      CosineAnnealingWarmRestarts(T_0=4, eta_min=1e-5).

The reference's ``training_tools`` / ``training_utilities`` share their module names with this
project's: never put ``sdp-net_amd/`` on ``sys.path`` in this process.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_trainer_golden.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))

import synth  # noqa: E402
from gen_golden import REF, WSEED, import_reference  # noqa: E402
from gen_train_golden import CASES  # noqa: E402

BCE_B, BCE_KS, BCE_EPS, BCE_SEED = 5, (10, 1000), (0.0, 0.1), 41
EMA_DECAY, EMA_SEED, EMA_CALLS = 0.999, 43, 2
SCHED = dict(optimizer_config=dict(lr=0.0015),
             scheduler_config=dict(constant_scheduler=dict(factor=0.001, total_iters=2),
                                   linear_scheduler=dict(start_factor=0.001, total_iters=5),
                                   cosine=dict(T_0=4, eta_min=1e-5)))
SCHED_EPOCHS = 12


def bce_inputs(K: int):
    """(logits [B, K] fp32, labels [B] int64, soft targets [B, K] fp32) from the portable PRNG."""
    B = BCE_B
    logits = torch.from_numpy((3.0 * synth.normal(synth.key_seed(BCE_SEED, f"logits{K}"), B * K))
                              .astype(np.float32).reshape(B, K))
    u = synth.uniform(synth.key_seed(BCE_SEED, f"labels{K}"), 3 * B)
    a = torch.from_numpy((u[:B] * K).astype(np.int64))
    b = torch.from_numpy((u[B:2 * B] * K).astype(np.int64))
    lam = torch.from_numpy(u[2 * B:].astype(np.float32)).view(B, 1)
    soft = lam * F.one_hot(a, K).float() + (1 - lam) * F.one_hot(b, K).float()
    return logits, a, soft


def perturbation(key: str, shape, call: int) -> torch.Tensor:
    """The seeded delta added to the floating entry ``key`` before EMA update number ``call``."""
    n = int(np.prod(shape)) if len(shape) else 1
    v = 1e-3 * synth.normal(synth.key_seed(EMA_SEED + call, key), n)
    return torch.from_numpy(v.astype(np.float32).reshape(tuple(shape)))


def main():
    ref_model, _, ref_tu = import_reference()
    sys.path.insert(0, REF)
    import training_tools as ref_tt  # noqa: E402  (binds the reference's training_utilities, already imported)
    sys.path.remove(REF)
    assert os.path.dirname(os.path.abspath(ref_tt.__file__)) == REF
    torch.set_num_threads(8)
    rec = {}

    # (a) the reference's BCE loss and its autograd gradient
    for K in BCE_KS:
        logits, labels, soft = bce_inputs(K)
        rec[f"bce/K{K}/logits"] = logits.numpy()
        rec[f"bce/K{K}/labels"] = labels.numpy()
        rec[f"bce/K{K}/soft"] = soft.numpy()
        for eps in BCE_EPS:
            fn = ref_tu.BCEWithLogitsLoss(num_classes=K, label_smoothing=eps)
            for kind, tgt in (("hard", labels), ("soft", soft)):
                x = logits.clone().requires_grad_(True)
                loss = fn(x, tgt)
                (g,) = torch.autograd.grad(loss, x)
                rec[f"bce/K{K}/{kind}/eps{eps}/loss"] = np.float32(loss.item())
                rec[f"bce/K{K}/{kind}/eps{eps}/dlogits"] = g.numpy()

    # (b) the reference's EMA state after two updates of the train_cf model
    cfg = CASES["train_cf"][0]
    torch.manual_seed(0)
    m = ref_model.MainModel.from_dict(**cfg)
    m.load_state_dict(synth.synth_state_dict(m, WSEED))
    ema = ref_tt.EMA_model(m, decay=EMA_DECAY)
    for call in range(1, EMA_CALLS + 1):
        with torch.no_grad():
            for k, v in m.state_dict().items():
                if v.is_floating_point():
                    v.add_(perturbation(k, v.shape, call))
        ema.update_parameters(m)
    ema_keys = []
    for k, v in ema.state_dict().items():
        rec["ema/" + k] = v.numpy()
        ema_keys.append([k, str(v.dtype)])

    # (c) the schedule of return_scheduler_optimizer
    lin = torch.nn.Linear(2, 2)
    _, sched = ref_tt.return_scheduler_optimizer(lin, **SCHED)
    lrs = [sched.get_last_lr()[0]]
    for _ in range(SCHED_EPOCHS):
        sched.optimizer.step()
        sched.step()
        lrs.append(sched.get_last_lr()[0])
    rec["lr"] = np.asarray(lrs, dtype=np.float64)

    meta = dict(bce=dict(B=BCE_B, K=list(BCE_KS), eps=list(BCE_EPS), seed=BCE_SEED),
                ema=dict(case="train_cf", config=cfg, wseed=WSEED, decay=EMA_DECAY, seed=EMA_SEED, calls=EMA_CALLS,
                         delta="1e-3 * synth.normal(synth.key_seed(seed + call, key), n) as fp32, call = 1, 2",
                         keys=ema_keys),
                schedule=dict(SCHED, epochs=SCHED_EPOCHS))
    out = os.path.join(HERE, "trainer_ref.npz")
    np.savez_compressed(out, meta=json.dumps(meta), **rec)
    print(f"wrote {out}: {os.path.getsize(out)} bytes, {len(rec)} arrays; ema dtypes "
          f"{sorted(set(d for _, d in ema_keys))}; lr {lrs[:3]} ... {lrs[-1]}")


if __name__ == "__main__":
    main()
