"""Per-tensor judgement of training gradients (test infrastructure; a plain module, not a conftest).

Every rule here compares ONE parameter tensor's gradient with that tensor's own reference:
there is no model-wide floor.  With the synthetic weights the largest gradient of a model is
the head weight and early-layer gradients are 1e-5 to 1e-8 of it, so a floor tied to the
largest gradient lets whole tensors be wrong (an all-zero conv-block LayerNorm gradient
passes it) -- tests/test_grad_judge_selfcheck.py shows that on the oracle itself.

fp32 rule    max|got - ref| <= 1e-4 * max|ref| of that tensor.  The only exemption is by
             name: ``*k_norm.bias``.  A bias added to every key shifts all scores of a query
             equally and softmax ignores it, so its exact gradient is zero (1e-19 of the
             model's largest gradient in fp64) and any finite-precision value is rounding
             noise.  It is judged absolutely against 1e-4 * max|ref gradient of the same
             layer's k_norm.weight|, and the number of exempted tensors must equal the number
             of encoder layers with normalize_qv.

bf16 rule    max|got - ref64| <= 4 * max|g_ac - ref64| per tensor, g_ac being the oracle's own
             CPU-autocast-bf16 gradient on the same inputs: a ratio of two absolute errors of
             the same tensor, so independent of its scale.  The one allowed fallback for a
             tensor that misses it on a single batch is the statistical form (``statistical``):
             over 8 fresh batches the median of the per-batch error ratios <= 1.5 and the
             ratio of the mean errors <= 2.0.

``oracle_grads`` is the reference both rules are fed from: autograd through the committed CPU
oracle (oracle/sdpnet_oracle.py, pinned to the reference's own gradients by the train
fixtures), in fp64, fp32 or under CPU autocast.
"""
import numpy as np
import torch
import torch.nn.functional as F

import sdpnet_oracle as orc

FP32_TOL = 1e-4
BF16_FACTOR = 4.0
STAT_MEDIAN, STAT_MEAN, STAT_BATCHES = 1.5, 2.0, 8
EXEMPT_SUFFIX = "k_norm.bias"


def _np(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def amax(t) -> float:
    return float(np.abs(_np(t)).max())


def err(a, b) -> float:
    return float(np.abs(_np(a) - _np(b)).max())


def qv_layers(cfg: dict) -> int:
    """Encoder layers with a q/k head LayerNorm: one per block and the final block."""
    cfg = orc.full_config(cfg)
    return cfg["num_blocks"] + 1 if cfg["normalize_qv"] else 0


def oracle_grads(cfg, sd, x, y, num_registers=3, label_smoothing=0.1, dtype=torch.float32, autocast=False):
    """(loss, {name: gradient}) of cross_entropy(oracle(x), y): autograd through the CPU oracle with
    weights and images in ``dtype`` (fp64 is the reference of both rules), or fp32 under CPU
    autocast to bf16 (``autocast=True``, the denominator of the bf16 rule)."""
    osd = {k: (v.detach().to(dtype).clone().requires_grad_(True) if v.is_floating_point() else v.clone())
           for k, v in sd.items()}
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        logits = orc.forward.__wrapped__(x.to(dtype), osd, cfg, num_registers=num_registers)
        loss = F.cross_entropy(logits, y, label_smoothing=label_smoothing)
    loss.backward()
    grads = {k: v.grad.detach().to(torch.float64).numpy() for k, v in osd.items()
             if v.is_floating_point() and v.grad is not None}
    return float(loss.detach()), grads


def fp32_report(got: dict, ref: dict, names=None, tol: float = FP32_TOL):
    """[(error / allowed, error, allowed, name)] worst first, and the exempted names.  ``got`` and
    ``ref`` map parameter names to gradients; ``names`` defaults to every key of ``got``."""
    rows, exempt = [], []
    for k in (list(got) if names is None else names):
        e = err(got[k], ref[k])
        if k.endswith(EXEMPT_SUFFIX):
            exempt.append(k)
            allowed = tol * amax(ref[k[: -len("bias")] + "weight"])
        else:
            allowed = tol * amax(ref[k])
        rows.append((e / allowed if allowed > 0 else (0.0 if e == 0 else float("inf")), e, allowed, k))
    rows.sort(reverse=True)
    return rows, exempt


def fp32_failures(got: dict, ref: dict, n_qv_layers: int, names=None, tol: float = FP32_TOL):
    """The tensors that miss the fp32 rule (empty: pass).  Asserts that exactly the expected
    number of tensors took the k_norm.bias exemption."""
    rows, exempt = fp32_report(got, ref, names, tol)
    assert len(exempt) == n_qv_layers, (exempt, n_qv_layers)
    return [r for r in rows if not r[0] <= 1.0]


def assert_fp32(got: dict, ref: dict, n_qv_layers: int, names=None, what: str = ""):
    bad = fp32_failures(got, ref, n_qv_layers, names)
    assert not bad, (what, len(bad), bad[:4])


def bf16_report(got: dict, ref64: dict, g_ac: dict, names=None, factor: float = BF16_FACTOR, ac_ref=None):
    """[(error / allowed, error, autocast's error, name)] worst first.  ``ac_ref``: the reference
    g_ac's own error is taken against, when it is not ``ref64`` (the denominator of another run)."""
    rows = []
    for k in (list(got) if names is None else names):
        e, eac = err(got[k], ref64[k]), err(g_ac[k], (ref64 if ac_ref is None else ac_ref)[k])
        rows.append((e / (factor * eac) if eac > 0 else (0.0 if e == 0 else float("inf")), e, eac, k))
    rows.sort(reverse=True)
    return rows


def bf16_failures(got: dict, ref64: dict, g_ac: dict, names=None):
    return [r for r in bf16_report(got, ref64, g_ac, names) if not r[0] <= 1.0]


def assert_bf16(got: dict, ref64: dict, g_ac: dict, names=None, what: str = ""):
    bad = bf16_failures(got, ref64, g_ac, names)
    assert not bad, (what, len(bad), bad[:4])


def statistical(errs: dict):
    """The statistical form of the bf16 rule.  ``errs[name]`` is a list, one entry per fresh batch
    (STAT_BATCHES of them), of (our error, autocast's error) against the same reference.  Returns
    the tensors whose median per-batch ratio exceeds 1.5 or whose mean-error ratio exceeds 2.0."""
    bad = []
    for k, v in errs.items():
        assert len(v) == STAT_BATCHES, (k, len(v))
        med = float(np.median([a / max(b, 1e-300) for a, b in v]))
        mean = float(np.mean([a for a, _ in v]) / max(np.mean([b for _, b in v]), 1e-300))
        if not (med <= STAT_MEDIAN and mean <= STAT_MEAN):
            bad.append((med, mean, k))
    return sorted(bad, reverse=True)
