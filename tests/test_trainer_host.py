"""CPU: the host side of ``training_tools`` / ``training_utilities`` (no kernel launches): the LR
schedule against the reference's (tests/golden/trainer_ref.npz, recorded from the reference by
gen_trainer_golden.py), the loss / accuracy trackers, the wandb-free imports and the checkpoint
layout."""
import sys

import numpy as np
import pytest
import torch

import golden_util as gu


@pytest.fixture(scope="module")
def ref():
    return gu.load_case("trainer_ref")


def test_lr_schedule_matches_reference(ref):
    import sdpnet_train
    import training_tools as tt
    meta, arr = ref
    sc = meta["schedule"]
    lin = torch.nn.Linear(2, 2)
    opt, sched = tt.return_scheduler_optimizer(lin, optimizer_config=sc["optimizer_config"],
                                               scheduler_config=sc["scheduler_config"])
    assert isinstance(opt, sdpnet_train.AdamW)
    assert isinstance(sched, torch.optim.lr_scheduler.SequentialLR)
    assert sched._milestones == [2, 7]
    lrs = [sched.get_last_lr()[0]]
    for _ in range(sc["epochs"]):
        opt.step()  # no gradients: a no-op that only keeps the scheduler's call-order check quiet
        sched.step()
        lrs.append(sched.get_last_lr()[0])
    assert len(lrs) == len(arr["lr"]) == 13
    np.testing.assert_allclose(np.asarray(lrs), arr["lr"], rtol=1e-9, atol=0)
    assert opt.param_groups[0]["lr"] == lrs[-1]


def test_loss_tracker_takes_floats_and_tensors():
    import training_utilities as tu
    t = tu.distributed_loss_track(task="Train")
    t.update(1.0)
    t.update(torch.tensor(2.0))
    t.update(torch.tensor(4.5, requires_grad=True) * 2)  # a loss still on the graph: stored detached
    assert isinstance(t.temp_loss, torch.Tensor) and not t.temp_loss.requires_grad
    assert t.counter == 3
    assert t.log() == pytest.approx(4.0)
    assert (t.temp_loss, t.counter, t.epoch) == (0.0, 0, 1)
    t.update(0.5)
    assert t.log() == pytest.approx(0.5) and t.epoch == 2


def test_accuracy_tracker_takes_floats_and_tensors():
    import training_utilities as tu
    a = tu.track_accuracy(task="Validation")
    assert a.log() == 0.0 and a.epoch == 1  # nothing seen: 0, as the reference
    a.update(batch_accuracy=3, batch_size=4)
    a.update(batch_accuracy=torch.tensor(1.0), batch_size=4)
    assert a.log() == pytest.approx(0.5)
    assert (a.correct, a.total, a.epoch) == (0.0, 0.0, 2)


def test_training_modules_import_without_wandb():
    """Importing the modules and using the trackers never imports wandb."""
    import training_tools
    import training_utilities as tu
    t = tu.distributed_loss_track()
    t.update(1.0)
    t.log()
    a = tu.track_accuracy()
    a.update(1, 2)
    a.log()
    assert "wandb" not in sys.modules
    for name in ("Trainer", "return_scheduler_optimizer", "EMA_model", "TeacherModel"):
        assert hasattr(training_tools, name)
    assert issubclass(training_tools.EMA_model, __import__("sdpnet_train").EMA)


def test_trackers_report_to_an_active_wandb_run_only(monkeypatch):
    import types

    import training_utilities as tu
    logged = []
    wb = types.ModuleType("wandb")
    wb.run = None
    wb.log = logged.append
    monkeypatch.setitem(sys.modules, "wandb", wb)
    t = tu.distributed_loss_track(task="Train")
    t.update(2.0)
    t.log()
    assert logged == []  # imported, but no run started
    wb.run = object()
    t.update(3.0)
    t.log()
    assert logged == [{"epoch": 1, "Train_loss": 3.0}]
    quiet = tu.distributed_loss_track(wandb_log=False)
    quiet.update(1.0)
    quiet.log()
    assert len(logged) == 1


class _Sampler:
    def set_epoch(self, epoch):
        self.epoch = epoch


class _Loader(list):
    sampler = _Sampler()


def test_checkpoint_of_a_never_stepped_optimizer_has_the_five_keys(tmp_path):
    import model as ours
    import training_tools as tt
    import training_utilities as tu
    cfg = dict(embedding_dim=32, num_blocks=1, n_head=2, max_image_size=[16, 16], output_classes=10)
    m = ours.MainModel.from_dict(**cfg)
    sc = dict(constant_scheduler=dict(factor=0.001, total_iters=2), linear_scheduler=dict(start_factor=0.001, total_iters=5),
              cosine=dict(T_0=4, eta_min=1e-5))
    opt, sched = tt.return_scheduler_optimizer(m, optimizer_config=dict(lr=0.0015, weight_decay=0.05), scheduler_config=sc)
    snap = tmp_path / "snap"
    tr = tt.Trainer(m, _Loader(), _Loader(), opt, sched, "cpu", save_every=1, gradient_accumulation_steps=1,
                    val_loss_logger=tu.distributed_loss_track(task="Val"), train_loss_logger=tu.distributed_loss_track(),
                    val_accuracy_logger=tu.track_accuracy(), snapshot_dir=str(snap), total_epochs=3, ema_decay=0.999)
    assert tr.PATH is None and tr.epoch == 0 and tr.fused and tr.reference_quirks
    assert set(tr.ema_model.state_dict()) == set(m.state_dict())
    tr.epoch = 4
    tr._save_checkpoint()
    ck = torch.load(snap / "model.pt", map_location="cpu", weights_only=True)
    assert sorted(ck) == ["epoch", "model_config", "model_state_dict", "optimizer_state", "scheduler_state"]
    assert ck["epoch"] == 4 and ck["model_config"] == cfg
    assert list(ck["model_state_dict"]) == list(m.state_dict())
    assert ck["optimizer_state"]["state"] == {}
    assert ck["optimizer_state"]["param_groups"][0]["weight_decay"] == 0.05
    # the file loads into torch.optim.AdamW, and a second Trainer on the directory resumes from it
    torch.optim.AdamW(m.parameters()).load_state_dict(ck["optimizer_state"])
    m2 = ours.MainModel.from_dict(**cfg)
    opt2, sched2 = tt.return_scheduler_optimizer(m2, optimizer_config=dict(lr=0.0015, weight_decay=0.05),
                                                 scheduler_config=sc)
    tr2 = tt.Trainer(m2, _Loader(), _Loader(), opt2, sched2, "cpu", save_every=1, gradient_accumulation_steps=1,
                     snapshot_dir=str(snap), total_epochs=3, ema_decay=0.0)
    assert tr2.epoch == 4 and not hasattr(tr2, "ema_model")
    for (k, a), (k2, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k == k2 and torch.equal(a, b)


def test_bce_with_logits_checks_its_arguments():
    import sdpnet_train
    x = torch.zeros(2, 10)
    with pytest.raises(ValueError, match="num_classes"):
        sdpnet_train.bce_with_logits(x, torch.zeros(2, dtype=torch.int64), 0.1, num_classes=1000)
    with pytest.raises(ValueError, match="float targets"):
        sdpnet_train.bce_with_logits(x, torch.zeros(2, 9), 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sdpnet_train.bce_with_logits(x, torch.zeros(2, dtype=torch.int64), 0.1, num_classes=10)
