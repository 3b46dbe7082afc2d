"""CPU: the host side of knowledge distillation (no kernel launches): the fp64 oracle against the
closed-form gradient of the contract, the argument validation of ``sdp_distill_loss`` and of its
wrappers, the Trainer's constructor arguments, and ``TeacherModel.from_checkpoint``."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import distill_oracle as do
import sdpnet_hip as sp


def _case(B, K, seed, scale=3.0, soft=False):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, K, generator=g, dtype=torch.float64) * scale
    t = torch.randn(B, K, generator=g, dtype=torch.float64) * scale
    a = torch.randint(0, K, (B,), generator=g)
    if not soft:
        return z, t, a
    b = torch.randint(0, K, (B,), generator=g)
    lam = torch.rand(B, 1, generator=g, dtype=torch.float64)
    return z, t, lam * F.one_hot(a, K) + (1 - lam) * F.one_hot(b, K)


# ------------------------------------------------------------------------------------ oracle
@pytest.mark.parametrize("soft_y", [False, True])
@pytest.mark.parametrize("base,kind", itertools.product(["ce", "bce"], ["soft", "hard"]))
@pytest.mark.parametrize("alpha,T,scale", [(0.0, 1.0, 3.0), (0.5, 0.5, 30.0), (1.0, 4.0, 3.0), (0.3, 2.0, 30.0)])
def test_oracle_gradient_is_the_closed_form(base, kind, soft_y, alpha, T, scale):
    z, t, y = _case(7, 33, seed=1, scale=scale, soft=soft_y)
    kw = dict(alpha=alpha, temperature=T, eps=0.1, base=base, kind=kind, grad_scale=8.0)
    loss, parts, g = do.distill(z, t, y, **kw)
    ref = do.closed_form_dlogits(z, t, y, **kw)
    assert torch.isfinite(loss) and torch.isfinite(g).all()
    assert (g - ref).abs().max() <= 1e-12 * ref.abs().max()
    assert abs(loss - ((1 - alpha) * parts[0] + alpha * parts[1])) <= 1e-12 * max(1.0, abs(loss))


def test_oracle_matches_torch_losses():
    z, t, y = _case(6, 20, seed=2)
    T = 3.0
    _, parts, _ = do.distill(z, t, y, alpha=0.5, temperature=T, eps=0.1, base="ce", kind="soft")
    assert abs(parts[0] - F.cross_entropy(z, y, label_smoothing=0.1)) <= 1e-12
    kl = F.kl_div(torch.log_softmax(z / T, 1), torch.softmax(t / T, 1), reduction="batchmean") * T * T
    assert abs(parts[1] - kl) <= 1e-12 * kl
    _, parts, _ = do.distill(z, t, y, alpha=0.5, eps=0.1, base="bce", kind="hard")
    yy = 0.9 * F.one_hot(y, 20).double() + 0.1 / 20
    assert abs(parts[0] - F.binary_cross_entropy_with_logits(z, yy)) <= 1e-12
    assert abs(parts[1] - F.cross_entropy(z, t.argmax(1))) <= 1e-12


def test_oracle_edge_cases():
    z, t, y = _case(4, 12, seed=3)
    # ties: the lowest index of the maximum
    t[1, 3] = t[1, 9] = t[1].max() + 1
    assert do.teacher_label(t)[1] == 3
    # a teacher probability of exactly 0 adds 0, not NaN
    t[2, 5] = -float("inf")
    loss, _, g = do.distill(z, t, y, alpha=1.0, temperature=2.0)
    assert torch.isfinite(loss) and torch.isfinite(g).all()
    # a bad label: NaN loss, NaN in that row only
    ybad = y.clone()
    ybad[0] = 12
    loss, _, g = do.distill(z, t, ybad, alpha=0.5)
    assert torch.isnan(loss) and torch.isnan(g[0]).all() and torch.isfinite(g[1:]).all()
    # identical teacher: no distillation term
    _, parts, g = do.distill(z, z.clone(), y, alpha=1.0, temperature=4.0)
    assert abs(parts[1]) <= 1e-12 and g.abs().max() <= 1e-12
    # bf16 inputs are upcast, not rounded again
    zb = z.to(torch.bfloat16)
    assert torch.equal(do.distill(zb, t, y, alpha=1.0)[2], do.distill(zb.double(), t, y, alpha=1.0)[2])


# ------------------------------------------------------------------------------------ C ABI
def _abi(dtype=0, logits=8, tdtype=0, teacher=8, labels=8, targets=None, B=2, K=4, alpha=0.5, T=1.0, mode=0,
         loss=8):
    """sdp_distill_loss with small non-null integers as addresses: every case here returns before a launch."""
    return sp.lib().sdp_distill_loss(dtype, logits, K, tdtype, teacher, K, labels, targets, K, B, K, 0.1, alpha, T,
                                     mode, 1.0, None, 0, loss, None, None)


@pytest.mark.parametrize("bad", [
    dict(logits=None), dict(teacher=None), dict(loss=None),
    dict(labels=8, targets=8), dict(labels=None, targets=None),
    dict(B=-1), dict(K=0), dict(K=-3),
    dict(alpha=-0.01), dict(alpha=1.5), dict(alpha=float("nan")),
    dict(T=0.0), dict(T=-1.0), dict(T=float("inf")), dict(T=float("nan")),
    dict(mode=-1), dict(mode=4), dict(dtype=2), dict(tdtype=7), dict(dtype=-1),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_abi_rejects_invalid_arguments_before_launch(bad):
    assert _abi(**bad) == 1
    if "B" not in bad:  # validated for an empty batch too
        assert _abi(B=0, **bad) == 1


def test_abi_empty_batch_is_a_noop():
    assert _abi(B=0) == 0
    assert _abi(B=0, labels=None, targets=8, mode=3, dtype=1, tdtype=1, alpha=1.0, T=0.25) == 0
    assert "sdp_distill_loss" in sp.exported_symbols()


# ------------------------------------------------------------------------------------ wrappers
def test_distillation_loss_checks_its_arguments():
    import sdpnet_train
    z, t, y = torch.zeros(2, 10), torch.zeros(2, 10), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sdpnet_train.distillation_loss(z, t, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sp.distill_loss(z, t, y, 0.0, 0.5, 1.0, 0, 1.0, None, torch.zeros(1))
    with pytest.raises(ValueError, match="teacher logits"):
        sdpnet_train.distillation_loss(z, torch.zeros(2, 9), y)
    with pytest.raises(ValueError, match="teacher logits"):
        sdpnet_train.distillation_loss(z, torch.zeros(3, 10), y)
    with pytest.raises(ValueError, match="alpha"):
        sdpnet_train.distillation_loss(z, t, y, alpha=1.5)
    with pytest.raises(ValueError, match="temperature"):
        sdpnet_train.distillation_loss(z, t, y, temperature=0)
    with pytest.raises(ValueError, match="kind"):
        sdpnet_train.distillation_loss(z, t, y, kind="x")
    with pytest.raises(ValueError, match="base"):
        sdpnet_train.distillation_loss(z, t, y, base="mse")
    with pytest.raises(ValueError, match="num_classes"):
        sdpnet_train.distillation_loss(z, t, y, num_classes=1000)
    with pytest.raises(ValueError, match="float targets"):
        sdpnet_train.distillation_loss(z, t, torch.zeros(2, 9))
    with pytest.raises(ValueError, match="int64 class indices"):
        sdpnet_train.distillation_loss(z, t, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        sdpnet_train.distillation_loss(z, t.half(), y)


# ------------------------------------------------------------------------------------ Trainer
class _Sampler:
    def set_epoch(self, epoch):
        self.epoch = epoch


class _Loader(list):
    sampler = _Sampler()


CFG = dict(embedding_dim=32, num_blocks=1, n_head=2, max_image_size=[16, 16], output_classes=10)
SCHED = dict(constant_scheduler=dict(factor=0.001, total_iters=2), linear_scheduler=dict(start_factor=0.001, total_iters=5),
             cosine=dict(T_0=4, eta_min=1e-5))


def _trainer(snap, **kw):
    import model as ours
    import training_tools as tt
    import training_utilities as tu
    m = ours.MainModel.from_dict(**CFG)
    opt, sched = tt.return_scheduler_optimizer(m, optimizer_config=dict(lr=0.0015, weight_decay=0.05),
                                               scheduler_config=SCHED)
    tr = tt.Trainer(m, _Loader(), _Loader(), opt, sched, "cpu", save_every=1, gradient_accumulation_steps=1,
                    val_loss_logger=tu.distributed_loss_track(task="Val"), train_loss_logger=tu.distributed_loss_track(),
                    val_accuracy_logger=tu.track_accuracy(), snapshot_dir=str(snap), total_epochs=3, **kw)
    return m, tr


class _Exploding(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(3))

    def forward(self, x):
        raise AssertionError("the teacher was called")


def test_trainer_distillation_arguments(tmp_path):
    import training_tools as tt
    with pytest.raises(ValueError, match="teacher_model"):
        _trainer(tmp_path / "a", distill_kind="soft")
    with pytest.raises(ValueError, match="teacher_model"):
        _trainer(tmp_path / "a", distill_kind="hard", teacher_model=None)
    with pytest.raises(ValueError, match="distill_kind"):
        _trainer(tmp_path / "a", distill_kind="kl", teacher_model=_Exploding())
    with pytest.raises(ValueError, match="distill_alpha"):
        _trainer(tmp_path / "a", distill_kind="soft", teacher_model=_Exploding(), distill_alpha=1.5)
    with pytest.raises(ValueError, match="distill_temperature"):
        _trainer(tmp_path / "a", distill_kind="soft", teacher_model=_Exploding(), distill_temperature=0.0)
    # the defaults: a teacher is stored, left alone and never called
    teacher = _Exploding().train()
    m, tr = _trainer(tmp_path / "b", teacher_model=teacher, ema_decay=0.999)
    assert tr.teacher_model is teacher and tr.distill_kind == "none" and tr.distill_parts is None
    assert teacher.training and teacher.w.requires_grad
    tr.epoch = 2
    ck = tr._checkpoint()
    assert sorted(ck) == ["epoch", "model_config", "model_state_dict", "optimizer_state", "scheduler_state"]
    assert list(ck["model_state_dict"]) == list(m.state_dict())
    assert set(tr.ema_model.state_dict()) == set(m.state_dict())
    # distilling: any callable is taken; a module, bare or in a TeacherModel, is frozen and in eval mode
    _, tr = _trainer(tmp_path / "c", teacher_model=lambda x: x, distill_kind="soft")
    assert tr.distill_base == "ce"
    for wrap in (lambda t: t, tt.TeacherModel):
        teacher = _Exploding().train()
        m, tr = _trainer(tmp_path / "c", teacher_model=wrap(teacher), distill_kind="hard", distill_alpha=0.25,
                         distill_temperature=3.0, use_cross_entropy=False)
        assert (tr.distill_kind, tr.distill_alpha, tr.distill_temperature, tr.distill_base) == ("hard", 0.25, 3.0, "bce")
        assert not teacher.training and not teacher.w.requires_grad
        ck = tr._checkpoint()
        assert sorted(ck) == ["epoch", "model_config", "model_state_dict", "optimizer_state", "scheduler_state"]
        assert list(ck["model_state_dict"]) == list(m.state_dict())
        assert set(tr.ema_model.state_dict()) == set(m.state_dict())


def test_teacher_from_checkpoint(tmp_path):
    import training_tools as tt
    snap = tmp_path / "snap"
    m, tr = _trainer(snap, ema_decay=0.999)
    with torch.no_grad():  # make the average differ from the weights
        for v in tr.ema_model.ema_weights.values():
            if v.is_floating_point():
                v.mul_(0.5)
    tr._save_checkpoint()
    tr.ema_model.ema_model_name = str(snap / "ema_model.pt")
    tr.ema_model.save_ema_model()

    t1 = tt.TeacherModel.from_checkpoint(str(snap / "model.pt"), device="cpu")
    t2 = tt.TeacherModel.from_checkpoint(str(snap / "ema_model.pt"), device="cpu")
    t3 = tt.TeacherModel.from_checkpoint(str(snap / "ema_model.pt"), device="cpu", config_from=str(snap / "model.pt"))
    for t, want in ((t1, m.state_dict()), (t2, tr.ema_model.state_dict()), (t3, tr.ema_model.state_dict())):
        assert isinstance(t, tt.TeacherModel) and not t.model.training
        assert not any(p.requires_grad for p in t.model.parameters())
        got = t.model.state_dict()
        assert list(got) == list(want)
        for k in got:
            assert torch.equal(got[k], want[k].cpu()), k
    w = next(iter(m.state_dict()))
    assert not torch.equal(t1.model.state_dict()[w], t2.model.state_dict()[w]) or not m.state_dict()[w].is_floating_point()
    (tmp_path / "alone").mkdir()
    torch.save(dict(tr.ema_model.state_dict()), tmp_path / "alone" / "ema.pt")
    with pytest.raises(FileNotFoundError, match="model_config"):
        tt.TeacherModel.from_checkpoint(str(tmp_path / "alone" / "ema.pt"), device="cpu")
