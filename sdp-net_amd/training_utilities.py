"""Drop-in subset of ``training_utilities`` (reference training_utilities.py).

Provided: ``KeLu`` (training_utilities.py:91-92), the activation on the hot
path's activation registry (model.py:22), running on the HIP elementwise kernel
(the same code path the GEMM epilogues use), plus the two stateless helpers
``BCEWithLogitsLoss`` (:95-107) and ``MeasureTime`` (:118-132), and the loss /
accuracy trackers ``distributed_loss_track`` and ``track_accuracy`` (:10-88) that
``model_train.py`` hands to the Trainer.

The trackers take a Python number or a 0-d device tensor and never synchronise in
``update``; ``log()`` all-reduces only when a process group is initialised.  This
module does not import wandb: ``log()`` reports to it only if the caller has already
imported it and started a run.  (The fused training loss is
``sdpnet_train.bce_with_logits``; ``BCEWithLogitsLoss`` here is the reference's
torch-op form.)
"""
from __future__ import annotations

import sys
from typing import Callable

import torch
import torch.distributed as dist

import sdpnet_hip as sp


def _dist_on() -> bool:
    return dist.is_available() and dist.is_initialized()


def _wandb_log(payload: dict) -> None:
    wb = sys.modules.get("wandb")  # never imported here
    if wb is not None and getattr(wb, "run", None) is not None:
        wb.log(payload)


class distributed_loss_track:
    """training_utilities.py:10-47: running sum / count of batch losses, mean per epoch."""

    def __init__(self, wandb_log: bool = True, task: str = "Train"):
        self.temp_loss = 0.0
        self.counter = 0
        self.epoch = 0
        self.task = task
        self.wandb_log = wandb_log

    def update(self, batch_loss):
        """``batch_loss``: a float or a 0-d tensor (accumulated on its device, no host read)."""
        if isinstance(batch_loss, torch.Tensor):
            batch_loss = batch_loss.detach()
        self.temp_loss = self.temp_loss + batch_loss
        self.counter += 1

    def reset(self):
        self.temp_loss = 0.0
        self.counter = 0
        self.epoch += 1

    def __all_reduce__(self):
        # NCCL / RCCL reduces device tensors, gloo host tensors
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        loss_tensor = torch.tensor([float(self.temp_loss), float(self.counter)], dtype=torch.float32, device=dev)
        dist.all_reduce(loss_tensor, dist.ReduceOp.SUM, async_op=False)
        self.temp_loss, self.counter = loss_tensor.cpu().tolist()

    def log(self):
        if _dist_on():
            self.__all_reduce__()
        loss = float(self.temp_loss) / self.counter
        if self.wandb_log:
            _wandb_log({"epoch": self.epoch, f"{self.task}_loss": loss})
        self.reset()
        return loss


class track_accuracy:
    """training_utilities.py:50-88: correct / total over an epoch."""

    def __init__(self, task="Validation", wandb_log=True):
        self.correct = 0.0
        self.total = 0.0
        self.epoch = 0
        self.task = task
        self.wandb_log = wandb_log

    def update(self, batch_accuracy, batch_size):
        """``batch_accuracy``: the number of correct rows, a number or a 0-d tensor (no host read)."""
        if isinstance(batch_accuracy, torch.Tensor):
            batch_accuracy = batch_accuracy.detach()
        self.correct = self.correct + batch_accuracy
        self.total = self.total + batch_size

    def reset(self):
        self.correct = 0.0
        self.total = 0.0
        self.epoch += 1

    def synchronize(self):
        if not _dist_on():
            return
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        t = torch.tensor([float(self.correct), float(self.total)], dtype=torch.float32, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        self.correct, self.total = t.cpu().tolist()

    def log(self):
        self.synchronize()
        total = float(self.total)
        acc = float(self.correct) / total if total > 0 else 0.0
        if self.wandb_log and (not _dist_on() or dist.get_rank() == 0):
            _wandb_log({"epoch": self.epoch, f"{self.task}_acc": acc})
        self.reset()
        return acc


def KeLu(x: torch.Tensor, a: float = 3.5) -> torch.Tensor:
    """0 for x < -a; x for x > a; 0.5 x (1 + x/a + sin(pi x / a) / pi) otherwise."""
    if a != 3.5:
        raise NotImplementedError("sdpnet HIP KeLu is compiled for a = 3.5 (the reference default)")
    if not x.is_cuda:
        raise RuntimeError("sdpnet KeLu runs on the HIP path only (CUDA/ROCm tensors)")
    xc = x.contiguous()
    if xc.dtype not in (torch.float32, torch.bfloat16):
        xc = xc.float()
    y = torch.empty_like(xc)
    sp.act(xc, y, sp.ACT_CODES["kelu"])
    return y


def BCEWithLogitsLoss(num_classes: int = 1000, label_smoothing: float = 0.1) -> Callable[[torch.Tensor, torch.Tensor], torch.Tensor]:
    def loss(input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if target.dim() == 1:
            target = torch.nn.functional.one_hot(target, num_classes)
        target_smoothed = target * (1 - label_smoothing) + label_smoothing / num_classes
        return torch.nn.functional.binary_cross_entropy_with_logits(input, target_smoothed)
    return loss


class MeasureTime:
    def __init__(self):
        self.start = torch.cuda.Event(enable_timing=True)
        self.stop = torch.cuda.Event(enable_timing=True)

    def __enter__(self):
        self.start.record()

    def __exit__(self, *args):
        self.stop.record()
        torch.cuda.synchronize()
        elapsed_time = self.start.elapsed_time(self.stop)
        print(f"Elapsed time: {elapsed_time/1000:.2f} seconds")
