"""Drop-in ``training_tools`` (reference training_tools.py): what ``model_train.py`` imports.

Same names and signatures -- ``Trainer``, ``return_scheduler_optimizer``, ``EMA_model``,
``TeacherModel`` -- on the fused HIP training step:

* the optimizer ``return_scheduler_optimizer`` returns is ``sdpnet_train.AdamW``; with it
  ``Trainer._run_batch`` replaces the reference's GradScaler / ``clip_grad_norm_`` / ``scaler.step``
  lines (training_tools.py:91-99) by ``opt.scale(loss).backward()`` and
  ``opt.step(grad_scale=None, max_norm=5.0)`` (one multi-tensor kernel, no host sync).  Any other
  optimizer runs the reference's lines as written;
* the loss is ``sdpnet_train.cross_entropy`` (``use_cross_entropy=True``, :72) or
  ``sdpnet_train.bce_with_logits`` (:74), each one kernel that also writes dlogits;
* ``EMA_model`` updates every fp32 entry in one ``sdp_ema_update`` launch (:291-297);
* ``_run_batch`` returns the loss as a 0-d device tensor and the epoch loop synchronises only on
  the batches it prints (the reference calls ``loss.item()`` and ``torch.cuda.synchronize()``
  every batch, :103, :115).

The reference has two behaviours a user may not expect, kept by default because this package
mirrors the reference (``reference_quirks=True``):

1. ``EMA_model.update_parameters`` overwrites every entry with the current value before mixing
   (:295-296: the condition is always true), so the "average" is the weights to within 1 ulp;
2. ``_run_batch`` zeroes the gradients at the start of every batch (:82), so with
   ``gradient_accumulation_steps > 1`` only the last micro-batch's gradient reaches the step.

``Trainer(..., reference_quirks=False)`` gives a true exponential average and zeroes the gradients
only after a batch on which the optimizer stepped.

The reference stores ``teacher_model`` and never calls it (:64), and so does this Trainer by default
(``distill_kind="none"``).  ``distill_kind="soft"`` / ``"hard"`` distils from it: the loss becomes
``sdpnet_train.distillation_loss`` -- (1 - distill_alpha) * the loss above + distill_alpha * the
teacher term, one kernel -- against the logits of a frozen teacher run once per micro-batch.
"""
from __future__ import annotations

import os
from typing import Any

import torch
import torch.distributed as dist
from torch import nn as nn
from torch.nn.parallel import DistributedDataParallel as DDP

import sdpnet_hip as sp
import sdpnet_train


class Trainer:
    def __init__(
        self,
        model: torch.nn.Module,
        train_data: torch.utils.data.DataLoader,
        val_data: torch.utils.data.DataLoader,
        optimizer: torch.optim.Optimizer,
        scheduler: torch.optim.lr_scheduler,
        gpu_id: int,
        save_every: int,
        gradient_accumulation_steps: int,
        val_loss_logger: Any = None,
        train_loss_logger: Any = None,
        val_accuracy_logger: Any = None,
        compile_model: bool = False,
        snapshot_name: str = "model.pt",
        snapshot_dir: str = "model",
        total_epochs: int = 300,
        report_every_epoch: int = 1,
        ema_decay: float = 0.999,
        use_cross_entropy: bool = True,
        teacher_model: Any = None,
        label_smoothing: float = 0.1,
        reference_quirks: bool = True,
        distill_kind: str = "none",
        distill_alpha: float = 0.5,
        distill_temperature: float = 1.0,
    ) -> None:
        self.gpu_id = gpu_id
        self.reference_quirks = bool(reference_quirks)
        self.model_config = model.config
        self.model = model.to(gpu_id)
        if dist.is_available() and dist.is_initialized():  # training_tools.py:36 (model_train.py runs under torchrun)
            self.model = DDP(self.model, device_ids=[gpu_id])
        if compile_model:
            self.model = torch.compile(self.model, dynamic=True, fullgraph=False)
        if ema_decay > 0:
            self.ema_model = EMA_model(self.model, decay=ema_decay)
            self.ema_model.reference_quirks = self.reference_quirks
        #
        self.snapshot_dir = snapshot_dir
        self.snapshot_name = snapshot_name
        self.PATH = os.path.join(self.snapshot_dir, self.snapshot_name) if os.path.exists(self.snapshot_dir) else None
        #
        self.train_data = train_data
        self.val_data = val_data
        self.total_epochs = total_epochs
        #
        self.optimizer = optimizer
        self.scheduler = scheduler
        self.grad_accum_steps = gradient_accumulation_steps
        #
        self.save_every = save_every
        self.report_in_every = report_every_epoch
        self.epoch = 0
        #
        self.val_loss_logger = val_loss_logger
        self.train_loss_logger = train_loss_logger
        self.val_accuracy_logger = val_accuracy_logger
        # "none": stored and never called, as in the reference.  "soft" / "hard": the loss becomes
        # sdpnet_train.distillation_loss against the teacher's logits (see _run_batch)
        if distill_kind not in ("none", "soft", "hard"):
            raise ValueError(f"distill_kind is 'none', 'soft' or 'hard', got {distill_kind!r}")
        self.distill_kind = distill_kind
        self.distill_alpha = float(distill_alpha)
        self.distill_temperature = float(distill_temperature)
        self.distill_parts = None  # [Base, Distill] of the last batch, unweighted, on the device
        if distill_kind != "none":
            if teacher_model is None:
                raise ValueError(f"distill_kind={distill_kind!r} needs a teacher_model")
            if not callable(teacher_model):
                raise ValueError("teacher_model must be a TeacherModel, an nn.Module or a callable")
            if not 0.0 <= self.distill_alpha <= 1.0:
                raise ValueError(f"distill_alpha must lie in [0, 1], got {distill_alpha}")
            if not 0.0 < self.distill_temperature < float("inf"):
                raise ValueError(f"distill_temperature must be positive and finite, got {distill_temperature}")
            # the teacher is frozen and stays outside DDP, torch.compile, the checkpoint and the EMA
            net = teacher_model.model if isinstance(teacher_model, TeacherModel) else teacher_model
            if isinstance(net, nn.Module):
                net.to(gpu_id).eval().requires_grad_(False)
        self.teacher_model = teacher_model
        #  Mixed precision training
        self.autocast = torch.autocast
        self.fused = isinstance(optimizer, sdpnet_train.AdamW)
        # the fused optimizer carries the GradScaler state on the device (optimizer.scaler)
        self.scaler = None if self.fused else torch.amp.GradScaler("cuda")
        # Recover from a checkpoint!
        try:
            self._load_checkpoint(self.PATH)
        except Exception as e:
            print(f"There is a problem with loading the model weights and the problem is: {e}")
        ## loss_fn
        self.label_smoothing = label_smoothing
        self.distill_base = "ce" if use_cross_entropy else "bce"
        if use_cross_entropy:
            self.loss_fn = lambda out, tgt: sdpnet_train.cross_entropy(out, tgt, label_smoothing)
        else:
            num_classes = int(self.model_config.get("output_classes", 1000))
            self.loss_fn = lambda out, tgt: sdpnet_train.bce_with_logits(out, tgt, label_smoothing, num_classes)

    def _run_batch(self, source: torch.Tensor, targets: torch.Tensor, batch_enum=None) -> torch.Tensor:
        step_now = (batch_enum + 1) % self.grad_accum_steps == 0
        if self.reference_quirks:
            # -- Zero the grads on the graph -- # (training_tools.py:82: every batch)
            self.optimizer.zero_grad(set_to_none=True)

        with self.autocast(device_type="cuda", dtype=torch.bfloat16):
            output = self.model(source)
            if self.distill_kind == "none":
                loss = self.loss_fn(output, targets)
            else:
                with torch.no_grad():
                    teacher_out = self.teacher_model(source)
                if not isinstance(teacher_out, torch.Tensor) or teacher_out.shape != output.shape:
                    got = tuple(teacher_out.shape) if isinstance(teacher_out, torch.Tensor) else type(teacher_out)
                    raise ValueError(f"the teacher returned {got}, the student's logits are {tuple(output.shape)}")
                loss, self.distill_parts = sdpnet_train.distillation_loss(
                    output, teacher_out, targets, alpha=self.distill_alpha, temperature=self.distill_temperature,
                    kind=self.distill_kind, base=self.distill_base, label_smoothing=self.label_smoothing,
                    return_parts=True)

        if self.fused:
            self.optimizer.scale(loss).backward()
            if step_now:
                # unscale, inf / nan skip, clip_grad_norm_(5), AdamW and the scale update (:94-99)
                self.optimizer.step(grad_scale=None, max_norm=5.0)
        else:
            self.scaler.scale(loss).backward()
            if step_now:
                self.scaler.unscale_(self.optimizer)
                torch.nn.utils.clip_grad_norm_(self.model.parameters(), 5)
                self.scaler.step(self.optimizer)
                self.scaler.update()
        if step_now and not self.reference_quirks:
            self.optimizer.zero_grad(set_to_none=True)

        ### We return the batch loss for logging purposses: on the device, no host read ###
        return loss.detach()

    def _run_epoch(self):
        init_start = torch.cuda.Event(enable_timing=True)
        init_end = torch.cuda.Event(enable_timing=True)
        for i, (source, targets) in enumerate(self.train_data):
            source, targets = source.to(self.gpu_id, non_blocking=True), targets.to(self.gpu_id, non_blocking=True)
            report = (self.gpu_id == 0) and i % 10 == 0
            if report:
                init_start.record()
            batch_loss = self._run_batch(source, targets, batch_enum=i)
            # update ema
            if hasattr(self, "ema_model"):
                self.ema_model.update_parameters(self.model)
            # log the batch loss onto local logger!!!
            self.train_loss_logger.update(batch_loss)
            ## print the loss
            if report:
                init_end.record()
                torch.cuda.synchronize()
                print(f"{i} Batch passed the average loss is {batch_loss.item()}, lr is {self.scheduler.get_last_lr()} -- {init_start.elapsed_time(init_end) / 1000}secs to pass a batch!")

    def train(self):
        for epoch in range(self.epoch + 1, self.total_epochs):
            self.epoch = epoch
            if epoch % self.report_in_every == 0:
                print(f"[GPU{self.gpu_id}] Epoch {self.epoch}\n")
            ##
            self.train_data.sampler.set_epoch(self.epoch)
            ##
            self.model.train()  ## Model in train mode!!!
            self._run_epoch()
            # ## let's log the loss now!!!
            self.train_loss_logger.log()
            ##  Epoch is done take one step scheduler,
            self.scheduler.step()
            if self.gpu_id == 0 and epoch % self.save_every == 0:
                self._save_checkpoint()
                if hasattr(self, "ema_model"):
                    self.ema_model.save_ema_model()
            ## Let's validate
            self.validate()

    def validate(self):
        self.model.eval()
        if self.gpu_id == 0:
            print("Validation is started!!!")
        with torch.no_grad():  ## block tracking gradients
            for source, targets in self.val_data:
                source, targets = source.to(self.gpu_id, non_blocking=True), targets.to(self.gpu_id, non_blocking=True)
                output = self.model(source)
                # per-row CE and top-1 hit of nn.CrossEntropyLoss()(output, targets) / argmax (:173-174)
                m = sp.logits_metrics(output.contiguous(), targets.to(torch.int64), 0.0)
                self.val_loss_logger.update(m[:, 0].mean())
                self.val_accuracy_logger.update(batch_accuracy=m[:, 2].sum(), batch_size=targets.shape[0])

            val_loss = self.val_loss_logger.log()
            val_acc = self.val_accuracy_logger.log()

        if self.gpu_id == 0:
            print(f"Epoch | {self.epoch} - validation loss is {val_loss}, accuracy is {val_acc}")

    ## Some tools ##
    def _load_checkpoint(self, checkpoint_file):
        model_dict = torch.load(checkpoint_file, map_location="cpu", weights_only=True)
        ### Now the state dict are obtained below ###
        model_state_dict = model_dict["model_state_dict"]
        model_optimizer_state = model_dict["optimizer_state"]
        model_scheduler_state = model_dict["scheduler_state"]

        ### ---Let's load the model states--- ###
        self.model.load_state_dict(model_state_dict)
        self.optimizer.load_state_dict(model_optimizer_state)
        self.scheduler.load_state_dict(model_scheduler_state)
        self.epoch = model_dict["epoch"]
        if hasattr(self, "ema_model"):  # the average restarts from the loaded weights (the reference's, built
            # before the load at :40-41, is overwritten by its first update anyway)
            self.ema_model = EMA_model(self.model, decay=self.ema_model.decay)
            self.ema_model.reference_quirks = self.reference_quirks
        print(f"Loaded the new model saved at {self.PATH}, will continue training from {self.epoch} epoch")

    def _optimizer_state(self):
        """optimizer.state_dict() with every ``step`` an independent 0-d host tensor, as
        torch.optim.AdamW stores it: sdpnet_train.AdamW keeps the step counts as views of one
        device array, which torch.save would write whole for every parameter.  Stored like this
        the file loads into torch.optim.AdamW and back."""
        sd = self.optimizer.state_dict()
        state = {}
        for k, st in sd["state"].items():
            st = dict(st)
            if isinstance(st.get("step"), torch.Tensor):
                st["step"] = st["step"].detach().to("cpu", copy=True)
            state[k] = st
        return {"state": state, "param_groups": sd["param_groups"]}

    def _save_checkpoint(self):
        ### If dir does not exist, create it!!
        if not os.path.exists(self.snapshot_dir):
            os.mkdir(self.snapshot_dir)
        self.PATH = os.path.join(self.snapshot_dir, self.snapshot_name)

        ### This are the necessary steps to recover the model from the pickled file!!!
        checkpoint = self._checkpoint()
        try:
            torch.save(checkpoint, self.PATH)
            print(f"Epoch {self.epoch} | Training checkpoint saved at {self.PATH}")
        except Exception as exp:
            print(f"Something went wrong with {exp}, the training will start from begining!!!")

    def _checkpoint(self):
        return {"model_state_dict": self.model.state_dict(),
                "model_config": self.model_config,
                "optimizer_state": self._optimizer_state(),
                "scheduler_state": self.scheduler.state_dict(),
                "epoch": self.epoch}


def return_scheduler_optimizer(model, **kwargs):
    #################
    ## -Optimizer- ##
    #################
    opt_kwargs = kwargs["optimizer_config"]
    optimizer = sdpnet_train.AdamW(model.parameters(), **opt_kwargs)

    #################
    ## Scheduler   ##
    #################
    scheduler_kwargs = kwargs["scheduler_config"]
    ### Warm up step starts ###
    scheduler0 = torch.optim.lr_scheduler.ConstantLR(optimizer, **scheduler_kwargs["constant_scheduler"])
    scheduler1 = torch.optim.lr_scheduler.LinearLR(optimizer, **scheduler_kwargs["linear_scheduler"])
    ## Scheduler 2 ##
    scheduler2 = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(optimizer, **scheduler_kwargs["cosine"])
    ## combine those dudes ###
    ms1 = scheduler_kwargs["constant_scheduler"]["total_iters"]
    ms2 = scheduler_kwargs["linear_scheduler"]["total_iters"]
    scheduler = torch.optim.lr_scheduler.SequentialLR(optimizer, schedulers=[scheduler0, scheduler1, scheduler2],
                                                      milestones=[ms1, ms1 + ms2])
    return optimizer, scheduler


class TeacherModel:
    def __init__(self, model: nn.Module, compile_model: bool = False):
        if compile_model:
            self.model = torch.compile(model)
        else:
            self.model = model.eval()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        with torch.inference_mode():
            return self.model(x)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return self.forward(x)

    @classmethod
    def from_checkpoint(cls, path: str, device="cuda", compile_model: bool = False,
                        config_from: str = None) -> "TeacherModel":
        """A frozen teacher from a file of this package (``eval_harness.return_model``): a Trainer
        checkpoint (``Trainer._save_checkpoint``; the model is rebuilt from its ``model_config``),
        or an EMA file (``EMA_model.save_ema_model``), which is a plain state dict: its
        ``model_config`` is read from the Trainer checkpoint ``config_from`` (default: ``model.pt``
        in the same folder)."""
        import eval_harness

        path = os.path.abspath(path)
        head = torch.load(path, map_location="cpu", weights_only=True)
        if isinstance(head, dict) and "model_config" in head and "model_state_dict" in head:
            model, _ = eval_harness.return_model("", path, None)
        else:
            ckpt = os.path.abspath(config_from) if config_from else os.path.join(os.path.dirname(path), "model.pt")
            if not os.path.exists(ckpt):
                raise FileNotFoundError(f"{path} holds weights only; the Trainer checkpoint {ckpt} that would give "
                                        "its model_config is missing (pass config_from)")
            _, model = eval_harness.return_model("", ckpt, path)
        del head
        model = model.to(device).eval().requires_grad_(False)
        return cls(model, compile_model=compile_model)


class EMA_model(sdpnet_train.EMA):
    """training_tools.py:282-302 on ``sdpnet_train.EMA`` in reference mode (``device`` is unused
    there too: the average lives where the model's state dict lives)."""

    def __init__(self, model: nn.Module, decay: float = 0.999, device="cuda", ema_model_name: str = "ema_model.pt"):
        super().__init__(model, decay=decay, reference_quirks=True, ema_model_name=ema_model_name)
