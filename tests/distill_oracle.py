"""The distillation loss of ``sdp_distill_loss`` / ``sdpnet_train.distillation_loss`` stated in fp64
torch CPU ops (helper of test_distill_host.py and test_gpu_distill.py; no test of its own).

    loss = (1 - alpha) * Base(z, y) + alpha * Distill(z, t)

Base, on targets smoothed to y' = (1 - eps) y + eps / K (y the one-hot of an int64 label or the
probability row):
    ce   mean over the B rows of  -sum_k y'_k log_softmax(z)_k
    bce  mean over the B K elements of binary_cross_entropy_with_logits(z, y')
A class index outside [0, K) makes its row NaN.
Distill:
    soft  T^2 / B * sum_i KL(softmax(t_i / T) || softmax(z_i / T)), written as
          T^2 [sum_k q_k (t_k - z_k) / T - lse(t / T) + lse(z / T)] with 0 * anything = 0
    hard  mean over the rows of  -log_softmax(z)[argmax t], the lowest index on ties, taken on the
          values as stored (bf16 values are exact in fp64)
The gradient is autograd's, of ``grad_scale * loss``; ``closed_form_dlogits`` restates it by hand.
"""
import torch
import torch.nn.functional as F


def _targets(y: torch.Tensor, K: int, eps: float):
    """fp64 smoothed target rows and the NaN mask of the rows with a class index outside [0, K)."""
    if y.is_floating_point():
        yy = y.detach().cpu().double()
        bad = torch.zeros(yy.shape[0], dtype=torch.bool)
    else:
        lab = y.detach().cpu().to(torch.int64)
        bad = (lab < 0) | (lab >= K)
        yy = F.one_hot(lab.clamp(0, K - 1), K).double()
    return (1.0 - eps) * yy + eps / K, bad


def teacher_label(t: torch.Tensor) -> torch.Tensor:
    """Lowest index of each row's maximum."""
    t = t.detach().cpu().double()
    K = t.shape[1]
    idx = torch.arange(K).expand_as(t)
    return torch.where(t == t.max(1, keepdim=True).values, idx, torch.full_like(idx, K)).min(1).values


def parts(z: torch.Tensor, t: torch.Tensor, y: torch.Tensor, *, temperature: float, eps: float, base: str,
          kind: str):
    """(Base, Distill) as fp64 scalars; ``z`` is used as given (fp64, maybe requiring grad)."""
    B, K = z.shape
    yy, bad = _targets(y, K, eps)
    # a factor, so that the row's gradient is NaN as well as its loss
    nan_rows = torch.where(bad, torch.full((B,), float("nan"), dtype=torch.float64), torch.ones(B, dtype=torch.float64))
    if base == "ce":
        b = (-(yy * torch.log_softmax(z, 1)).sum(1) * nan_rows).sum() / B
    elif base == "bce":
        b = (F.binary_cross_entropy_with_logits(z, yy, reduction="none").sum(1) * nan_rows).sum() / (B * K)
    else:
        raise ValueError(base)
    t = t.detach().cpu().double()
    if kind == "soft":
        T = float(temperature)
        q = torch.softmax(t / T, 1)
        cross = torch.where(q > 0, q * (t - z) / T, torch.zeros_like(q)).sum(1)
        d = T * T * (cross - torch.logsumexp(t / T, 1) + torch.logsumexp(z / T, 1)).sum() / B
    elif kind == "hard":
        d = -torch.log_softmax(z, 1).gather(1, teacher_label(t)[:, None]).sum() / B
    else:
        raise ValueError(kind)
    return b, d


def distill(z: torch.Tensor, t: torch.Tensor, y: torch.Tensor, *, alpha: float, temperature: float = 1.0,
            eps: float = 0.0, base: str = "ce", kind: str = "soft", grad_scale: float = 1.0):
    """(loss, parts [2], dlogits [B, K]), all fp64 on the CPU; bf16 / fp32 inputs are upcast."""
    zz = z.detach().cpu().double().requires_grad_(True)
    b, d = parts(zz, t, y, temperature=temperature, eps=eps, base=base, kind=kind)
    loss = (1.0 - alpha) * b + alpha * d
    (g,) = torch.autograd.grad(grad_scale * loss, zz)
    return loss.detach(), torch.stack([b.detach(), d.detach()]), g


def closed_form_dlogits(z: torch.Tensor, t: torch.Tensor, y: torch.Tensor, *, alpha: float, temperature: float = 1.0,
                        eps: float = 0.0, base: str = "ce", kind: str = "soft", grad_scale: float = 1.0):
    """The gradient as the kernel's contract writes it, in fp64."""
    z, t = z.detach().cpu().double(), t.detach().cpu().double()
    B, K = z.shape
    yy, bad = _targets(y, K, eps)
    if base == "ce":
        bg = (torch.softmax(z, 1) * yy.sum(1, keepdim=True) - yy) / B
    else:
        bg = (torch.sigmoid(z) - yy) / (B * K)
    bg[bad] = float("nan")
    if kind == "soft":
        T = float(temperature)
        dg = T / B * (torch.softmax(z / T, 1) - torch.softmax(t / T, 1))
    else:
        dg = (torch.softmax(z, 1) - F.one_hot(teacher_label(t), K).double()) / B
    return grad_scale * ((1.0 - alpha) * bg + alpha * dg)
