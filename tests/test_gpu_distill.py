"""GPU: knowledge distillation -- ``sdp_distill_loss`` against the fp64 oracle
(tests/distill_oracle.py), its identities and edge cases, far placement, the autograd entry
``sdpnet_train.distillation_loss`` and the Trainer's distillation step.

Bounds are those of the CE kernels (test_gpu_train_kernels.py::test_ce_loss_soft_targets, the same
``close``): loss and parts 1e-5, fp32 dlogits 1e-5 of the reference's largest magnitude, bf16
dlogits 2e-2.
"""
import functools
import itertools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import distill_oracle as do
import golden_util as gu
import sdpnet_hip as sp
import synth
from test_gpu_train_kernels import close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32
NAN = float("nan")
EPS, GS = 0.1, 8.0
SHAPES = [(1, 1), (5, 10), (4, 64), (37, 1000), (6, 1537)]
MODES = {0: ("ce", "soft"), 1: ("bce", "soft"), 2: ("ce", "hard"), 3: ("bce", "hard")}
ALPHAS, TEMPS, SCALES = [0.0, 0.5, 1.0], [0.5, 1.0, 4.0], [3.0, 30.0]


def name(dt):
    return "bf16" if dt == BF else "fp32"


def padded(data, fill=NAN):
    """``data`` [B, K] as rows of a wider allocation (ld = K + 5 > K), NaN in the padding columns."""
    B, K = data.shape
    buf = torch.full((B, K + 5), fill, dtype=data.dtype, device=DEV)
    buf[:, :K] = data
    return buf, buf[:, :K]


@functools.lru_cache(maxsize=None)
def inputs(B, K, scale, zdt, tdt):
    """(student, teacher, int64 labels, fp32 target rows), the first two and the last inside padded rows."""
    g = torch.Generator().manual_seed(1000 * B + K)
    z = (torch.randn(B, K, generator=g) * scale).to(zdt).to(DEV)
    t = (torch.randn(B, K, generator=g) * scale).to(tdt).to(DEV)
    a = torch.randint(0, K, (B,), generator=g)
    b = torch.randint(0, K, (B,), generator=g)
    lam = torch.rand(B, 1, generator=g)
    rows = (lam * F.one_hot(a, K) + (1 - lam) * F.one_hot(b, K)).float().to(DEV)
    return padded(z)[1], padded(t)[1], a.to(DEV), padded(rows)[1]


def run(z, t, y, *, alpha, T, mode, eps=EPS, gs=GS, grad=True, loss0=0.0, parts0=(0.0, 0.0), want_parts=True):
    """One launch: (loss [1], parts [2] or None, dlogits in padded rows or None, its whole buffer)."""
    loss = torch.full((1,), loss0, device=DEV)
    parts = torch.tensor(parts0, device=DEV) if want_parts else None
    dbuf = d = None
    if grad:
        dbuf, d = padded(torch.zeros_like(z))
        d.fill_(NAN)
    sp.distill_loss(z, t, y, eps, alpha, T, mode, gs, d, loss, parts)
    return loss, parts, d, dbuf


@functools.lru_cache(maxsize=None)
def oracle(B, K, scale, zdt, tdt, soft_y, mode, alpha, T):
    z, t, lab, rows = inputs(B, K, scale, zdt, tdt)
    base, kind = MODES[mode]
    return do.distill(z, t, rows if soft_y else lab, alpha=alpha, temperature=T, eps=EPS, base=base, kind=kind,
                      grad_scale=GS)


# ----------------------------------------------------------------------- kernel against the oracle
@pytest.mark.parametrize("tdt", [F32, BF], ids=lambda d: "t_" + name(d))
@pytest.mark.parametrize("zdt", [F32, BF], ids=lambda d: "z_" + name(d))
@pytest.mark.parametrize("mode", list(MODES), ids=lambda m: "-".join(MODES[m]))
@pytest.mark.parametrize("B,K", SHAPES)
def test_kernel_matches_oracle(B, K, mode, zdt, tdt):
    """Every (alpha, T, logit scale) with both target kinds, for every shape x mode x dtype pair."""
    for scale, soft_y, alpha, T in itertools.product(SCALES, [False, True], ALPHAS, TEMPS):
        z, t, lab, rows = inputs(B, K, scale, zdt, tdt)
        assert z.stride(0) > K and t.stride(0) > K and rows.stride(0) > K
        want_loss, want_parts, want_d = oracle(B, K, scale, zdt, tdt, soft_y, mode, alpha, T)
        loss, parts, d, dbuf = run(z, t, rows if soft_y else lab, alpha=alpha, T=T, mode=mode)
        what = f"scale {scale} soft_y {soft_y} alpha {alpha} T {T}"
        print("%s: loss err %.3e of %.3e, dlogits err %.3e of %.3e" % (
            what, (loss.cpu().double() - want_loss).abs().item(), want_loss.abs().item(),
            (d.cpu().double() - want_d).abs().max().item(), want_d.abs().max().item()))
        close(loss.cpu(), want_loss.view(1), 1e-5, "loss, " + what)
        close(parts[:1].cpu(), want_parts[:1], 1e-5, "parts[0], " + what)
        close(parts[1:].cpu(), want_parts[1:], 1e-5, "parts[1], " + what)
        close(d.cpu(), want_d, 1e-5 if zdt == F32 else 2e-2, "dlogits, " + what)
        assert torch.isnan(dbuf[:, K:]).all(), "padding columns of dlogits written, " + what


# ----------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("zdt", [F32, BF], ids=name)
@pytest.mark.parametrize("soft_y", [False, True])
@pytest.mark.parametrize("mode", [0, 1], ids=["ce", "bce"])
def test_alpha_zero_is_the_base_kernel(mode, soft_y, zdt):
    B, K = 37, 1000
    z, t, lab, rows = inputs(B, K, 3.0, zdt, F32)
    y = rows if soft_y else lab
    fn = {(0, False): sp.ce_loss, (0, True): sp.ce_loss_soft, (1, False): sp.bce_loss, (1, True): sp.bce_loss_soft}
    want = torch.zeros(1, device=DEV)
    wd = torch.empty(B, K, dtype=zdt, device=DEV)
    fn[(mode, soft_y)](z, y, EPS, GS, wd, want)
    for m in (mode, mode | 2):  # whatever the teacher term
        loss, parts, d, _ = run(z, t, y, alpha=0.0, T=4.0, mode=m)
        close(loss, want, 1e-6, "loss at alpha 0")
        close(parts[:1], want, 1e-6, "parts[0]")
        close(d, wd, 1e-6, "dlogits at alpha 0")


@pytest.mark.parametrize("mode", list(MODES), ids=lambda m: "-".join(MODES[m]))
def test_loss_is_the_weighted_sum_of_its_parts_and_accumulates(mode):
    z, t, lab, rows = inputs(37, 1000, 3.0, BF, F32)
    alpha = 0.3
    loss, parts, d, _ = run(z, t, lab, alpha=alpha, T=2.0, mode=mode)
    close(loss, ((1 - alpha) * parts[0] + alpha * parts[1]).view(1), 1e-6, "loss from parts")
    # *loss and parts accumulate into what they hold
    loss2, parts2, d2, _ = run(z, t, lab, alpha=alpha, T=2.0, mode=mode, loss0=2.5, parts0=(-1.0, 7.0))
    close(loss2, loss + 2.5, 1e-6, "accumulated loss")
    close(parts2, parts + torch.tensor([-1.0, 7.0], device=DEV), 1e-6, "accumulated parts")
    # dlogits = NULL and parts = NULL leave the loss as it is
    loss3, _, _, _ = run(z, t, lab, alpha=alpha, T=2.0, mode=mode, grad=False, want_parts=False)
    close(loss3, loss, 1e-6, "loss without dlogits")
    # two runs: the same dlogits bit for bit
    assert torch.equal(d.view(torch.int16), d2.view(torch.int16))


@pytest.mark.parametrize("zdt", [F32, BF], ids=name)
def test_teacher_equal_to_student_distils_nothing(zdt):
    z, _, lab, _ = inputs(37, 1000, 30.0, zdt, zdt)
    for T in TEMPS:
        _, parts, d, _ = run(z, z.clone(), lab, alpha=1.0, T=T, mode=0, gs=1.0)
        assert parts[1].abs().item() <= 1e-6 and d.float().abs().max().item() <= 1e-6, T
    # across dtypes: the same stored values
    zb = inputs(37, 1000, 3.0, BF, BF)[0]
    _, parts, d, _ = run(zb, zb.float(), lab, alpha=1.0, T=2.0, mode=0, gs=1.0)
    assert parts[1].abs().item() <= 1e-6 and d.float().abs().max().item() <= 1e-6


def test_hard_ties_take_the_lowest_index():
    B, K = 6, 1000
    z, t, lab, _ = inputs(B, K, 3.0, F32, F32)
    for tdt in (F32, BF):
        tt_ = t.to(tdt).clone()
        tt_[:, 700] = tt_[:, 3] = 64.0  # exact in bf16, above every other value
        _, parts, d, _ = run(z, tt_, lab, alpha=1.0, T=1.0, mode=2, gs=1.0)
        want = F.cross_entropy(z, torch.full((B,), 3, device=DEV))
        close(parts[1:], want.view(1), 1e-5, "hard distillation towards column 3")
        p = torch.softmax(z, 1)
        assert ((d[:, 3] - (p[:, 3] - 1) / B).abs() <= 1e-6).all()
        assert ((d[:, 700] - p[:, 700] / B).abs() <= 1e-6).all() and (d[:, 700] >= 0).all()


@pytest.mark.parametrize("mode", list(MODES), ids=lambda m: "-".join(MODES[m]))
def test_label_out_of_range_is_nan_not_oob(mode):
    B, K = 8, 100
    g = torch.Generator().manual_seed(28)
    z, t = torch.randn(B, K, generator=g).to(DEV), torch.randn(B, K, generator=g).to(DEV)
    labels = torch.tensor([0, 5, -7, 99, 100, 3, 7, 1], device=DEV)
    for alpha in (0.5, 1.0):
        loss, parts, d, _ = run(z, t, labels, alpha=alpha, T=1.0, mode=mode, eps=0.0, gs=1.0)
        torch.cuda.synchronize()
        assert torch.isnan(loss).all() and torch.isnan(parts[0]) and torch.isfinite(parts[1])
        bad = torch.isnan(d).all(dim=1).cpu()
        assert bad.tolist() == [False, False, True, False, True, False, False, False]
        assert not torch.isnan(d[~bad.to(DEV)]).any()


# -------------------------------------------------------------------------------- far placement
@pytest.fixture
def big_memory():
    torch.cuda.empty_cache()
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", [F32, BF], ids=name)
def test_far_placement(dtype, big_memory):
    """One row per group, ``.view()`` as the strided operand (test_gpu_placement.py's
    test_ce_loss_and_softmax): logits, teacher and dlogits rows on both sides of 2^31 and 2^32 bytes
    give the near twin's dlogits bit for bit and leave every guard band alone.  The loss is summed by
    atomic adds in no fixed order: 1e-6, as in that test."""
    from test_gpu_placement import GROUPS, run_sparse
    B, K = GROUPS, 1000
    tdt = BF if dtype == F32 else F32
    g = torch.Generator().manual_seed(31)
    z = (torch.randn(B, K, generator=g) * 3).to(dtype).to(DEV)
    t = (torch.randn(B, K, generator=g) * 3).to(tdt).to(DEV)
    labels = torch.randint(0, K, (B,), generator=g).to(DEV)

    def call(P):
        loss, parts = torch.zeros(1, device=DEV), torch.zeros(2, device=DEV)
        sp.distill_loss(P["logits"].view(), P["teacher"].view(), labels, EPS, 0.5, 2.0, 0, GS, P["d"].view(), loss,
                        parts)
        return {"loss": loss, "parts": parts}

    spec = {"logits": (K, dtype, z), "teacher": (K, tdt, t), "d": (K, dtype, None)}
    near = lambda a, b, what: close(a, b, 1e-6, what)  # noqa: E731
    got = run_sparse(spec, {"d"}, call, [("logits",), ("teacher",), ("d",)], cmp={"loss": near, "parts": near})
    want_loss, want_parts, want_d = do.distill(z, t, labels, alpha=0.5, temperature=2.0, eps=EPS, grad_scale=GS)
    close(got["loss"].cpu(), want_loss.view(1), 1e-5, "loss")
    close(got["parts"].cpu(), want_parts, 1e-5, "parts")
    close(got["d"].cpu(), want_d, 1e-5 if dtype == F32 else 2e-2, "dlogits")


# -------------------------------------------------------------------------------- autograd entry
@pytest.mark.parametrize("zdt", [F32, BF], ids=name)
@pytest.mark.parametrize("base,kind,soft_y", [("ce", "soft", False), ("bce", "soft", True), ("ce", "hard", True),
                                               ("bce", "hard", False)])
def test_distillation_loss_autograd(base, kind, soft_y, zdt):
    import sdpnet_train as st
    B, K, factor = 37, 1000, 1024.0
    z, t, lab, rows = (v.contiguous() for v in inputs(B, K, 3.0, zdt, BF))
    y = rows if soft_y else lab
    with torch.inference_mode():
        teacher = t * 1.0  # an inference tensor, as TeacherModel.forward returns
    assert teacher.is_inference()
    zr = z.clone().requires_grad_(True)
    loss, parts = st.distillation_loss(zr, teacher, y, alpha=0.4, temperature=2.0, kind=kind, base=base,
                                       label_smoothing=EPS, num_classes=K, return_parts=True)
    assert loss.dim() == 0 and loss.dtype == F32 and loss.requires_grad
    assert parts.shape == (2,) and not parts.requires_grad
    (loss * factor).backward()
    want_loss, want_parts, want_d = do.distill(z, teacher, y, alpha=0.4, temperature=2.0, eps=EPS, base=base, kind=kind)
    close(loss.detach().cpu().view(1), want_loss.view(1), 1e-5, "distillation_loss")
    close(parts.cpu(), want_parts, 1e-5, "parts")
    close(zr.grad.cpu(), want_d * factor, 1e-5 if zdt == F32 else 2e-2, "gradient under an upstream factor")
    assert teacher.grad is None and not teacher.requires_grad
    # a teacher that asks for a gradient gets none either
    t2 = t.clone().requires_grad_(True)
    zr2 = z.clone().requires_grad_(True)
    l2 = st.distillation_loss(zr2, t2, y, alpha=0.4, temperature=2.0, kind=kind, base=base, label_smoothing=EPS)
    l2.backward()
    assert t2.grad is None and torch.equal(zr2.grad * factor, zr.grad)


# --------------------------------------------------------------------------------------- Trainer
SCHED = dict(constant_scheduler=dict(factor=0.5, total_iters=1), linear_scheduler=dict(start_factor=0.5, total_iters=2),
             cosine=dict(T_0=4, eta_min=1e-5))
OPT = dict(lr=0.0015, weight_decay=0.05)
LS, DECAY, EPOCHS = 0.1, 0.999, 2
TEACHER_CFG = dict(embedding_dim=64, num_blocks=1, n_head=2, conv_kernel_size=5, patch_size=16, max_image_size=[16, 16],
                   output_classes=10, head_output_from_register=True, conv_first=False)


class _Sampler:
    def __init__(self):
        self.epochs = []

    def set_epoch(self, epoch):
        self.epochs.append(epoch)


class _Loader(list):
    def __init__(self, batches):
        super().__init__(batches)
        self.sampler = _Sampler()


class _Rec:
    def __init__(self):
        self.seen = []

    def update(self, loss):
        self.seen.append(loss)

    def log(self):
        return 0.0


@functools.lru_cache(maxsize=None)
def _data():
    x = synth.synth_images(77, 12, 64).view(4, 3, 3, 64, 64)
    y = torch.randint(0, 10, (4, 3), generator=torch.Generator().manual_seed(5))
    return [(x[i], y[i]) for i in range(3)], [(x[3], y[3])]


def _student():
    import model as ours
    import training_tools as tt
    meta, _ = gu.load_case("train_cf")
    torch.manual_seed(0)
    m = ours.MainModel.from_dict(**meta["config"])
    m.load_state_dict(synth.synth_state_dict(m, meta["wseed"]))
    m = m.to(DEV)
    opt, sched = tt.return_scheduler_optimizer(m, optimizer_config=OPT, scheduler_config=SCHED)
    return m, opt, sched


def _teacher():
    import model as ours
    torch.manual_seed(1)
    m = ours.MainModel.from_dict(**TEACHER_CFG)
    m.load_state_dict(synth.synth_state_dict(m, 4242))
    return m.train()  # the Trainer has to put it into eval mode


def _state(m, opt, sched, ema, losses):
    out = {"p/" + k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    for k, p in m.named_parameters():
        st_ = opt.state[p]
        out["m/" + k] = st_["exp_avg"].cpu().clone()
        out["v/" + k] = st_["exp_avg_sq"].cpu().clone()
        out["s/" + k] = st_["step"].detach().cpu().clone().reshape(())
    out["scaler"] = opt.scaler.cpu().clone()
    out["lr"] = torch.tensor(sched.get_last_lr(), dtype=torch.float64)
    for k, v in ema.state_dict().items():
        out["e/" + k] = v.cpu().clone()
    out["losses"] = torch.stack([l.float().cpu() for l in losses])
    return out


def _trainer(m, opt, sched, rec, **kw):
    import training_tools as tt
    import training_utilities as tu
    train, val = _data()
    return tt.Trainer(m, _Loader(train), _Loader(val), opt, sched, 0, save_every=1000, gradient_accumulation_steps=1,
                      val_loss_logger=tu.distributed_loss_track(wandb_log=False, task="Val"), train_loss_logger=rec,
                      val_accuracy_logger=tu.track_accuracy(wandb_log=False), snapshot_dir="no_such_snapshot_dir",
                      total_epochs=EPOCHS + 1, ema_decay=DECAY, label_smoothing=LS, **kw)


@functools.lru_cache(maxsize=None)
def _trainer_run(use_ce, kind, wrap):
    """Trainer.train() with a teacher; ``kind`` None: no teacher at all."""
    import training_tools as tt
    m, opt, sched = _student()
    rec = _Rec()
    if kind is None:
        tr = _trainer(m, opt, sched, rec, use_cross_entropy=use_ce)
        tr.train()
        return _state(m, opt, sched, tr.ema_model, rec.seen), {}
    teacher = _teacher()
    before = {k: v.clone() for k, v in teacher.state_dict().items()}
    calls = []
    teacher.register_forward_hook(lambda mod, inp, out: calls.append(tuple(out.shape)))
    tr = _trainer(m, opt, sched, rec, use_cross_entropy=use_ce, teacher_model=tt.TeacherModel(teacher) if wrap else teacher,
                  distill_kind=kind, distill_alpha=0.5, distill_temperature=2.0)
    if kind != "none":
        assert not teacher.training and not any(p.requires_grad for p in teacher.parameters())
        assert all(p.is_cuda for p in teacher.parameters())
    tr.train()
    sd = teacher.state_dict()
    info = dict(calls=calls, training=teacher.training, parts=tr.distill_parts, last_loss=rec.seen[-1],
                unchanged=list(sd) == list(before) and all(torch.equal(sd[k].cpu(), before[k].cpu()) for k in sd),
                ckpt=tr._checkpoint(), ema_keys=list(tr.ema_model.state_dict()), model_keys=list(m.state_dict()),
                wrapped=isinstance(tr.model, nn.parallel.DistributedDataParallel))
    return _state(m, opt, sched, tr.ema_model, rec.seen), info


@functools.lru_cache(maxsize=None)
def _hand_run(use_ce, kind):
    """The same loop written out from the pieces."""
    import sdpnet_train as st
    train, _ = _data()
    m, opt, sched = _student()
    teacher = _teacher().to(DEV).eval().requires_grad_(False)
    ema = st.EMA(m, decay=DECAY, reference_quirks=True)
    losses = []
    for _ in range(EPOCHS):
        m.train()
        for x, y in train:
            x, y = x.to(DEV), y.to(DEV)
            opt.zero_grad(set_to_none=True)
            with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                out = m(x)
                with torch.no_grad():
                    tl = teacher(x)
                loss = st.distillation_loss(out, tl, y, alpha=0.5, temperature=2.0, kind=kind,
                                            base="ce" if use_ce else "bce", label_smoothing=LS)
            opt.scale(loss).backward()
            opt.step(grad_scale=None, max_norm=5.0)
            ema.update_parameters(m)
            losses.append(loss.detach())
        sched.step()
    return _state(m, opt, sched, ema, losses)


@pytest.mark.parametrize("use_ce,kind,wrap", [(True, "soft", True), (False, "soft", False), (True, "hard", False)])
def test_trainer_distils_as_the_hand_written_loop(use_ce, kind, wrap):
    (got, info), want = _trainer_run(use_ce, kind, wrap), _hand_run(use_ce, kind)
    assert list(got) == list(want)
    for k in want:
        if k == "losses":
            assert got[k].shape == (EPOCHS * 3,) and torch.isfinite(got[k]).all()
            close(got[k], want[k], 1e-5, "batch losses")
        else:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    # the teacher: called once per batch, on [B, K] logits, in eval mode, unchanged, and nowhere in the files
    assert info["calls"] == [(3, 10)] * (EPOCHS * 3) and not info["training"] and info["unchanged"]
    assert not info["wrapped"]
    assert sorted(info["ckpt"]) == ["epoch", "model_config", "model_state_dict", "optimizer_state", "scheduler_state"]
    assert list(info["ckpt"]["model_state_dict"]) == info["model_keys"] == info["ema_keys"]
    # the parts of the last batch stay on the device and give its loss
    parts = info["parts"]
    assert parts.is_cuda and parts.shape == (2,) and not parts.requires_grad
    close((0.5 * parts[0] + 0.5 * parts[1]).view(1), info["last_loss"].view(1), 1e-6, "last loss from its parts")
    # and the teacher matters: plain training ends elsewhere
    plain, _ = _trainer_run(use_ce, None, False)
    assert any(not torch.equal(got[k], plain[k]) for k in got if k.startswith("p/"))


@pytest.mark.parametrize("use_ce", [True, False])
def test_trainer_with_an_unused_teacher_is_plain_training(use_ce):
    (got, info), (want, _) = _trainer_run(use_ce, "none", False), _trainer_run(use_ce, None, False)
    assert info["calls"] == [] and info["training"] and info["unchanged"] and info["parts"] is None
    assert list(got) == list(want)
    for k in want:
        if k == "losses":  # summed over the rows by atomic adds, in no fixed order
            close(got[k], want[k], 1e-5, "batch losses")
        else:
            assert torch.equal(got[k], want[k]), k


def test_trainer_rejects_a_teacher_with_other_classes():
    import model as ours
    m, opt, sched = _student()
    teacher = ours.MainModel.from_dict(**dict(TEACHER_CFG, output_classes=7))
    tr = _trainer(m, opt, sched, _Rec(), teacher_model=teacher, distill_kind="soft")
    x, y = _data()[0][0]
    m.train()
    with pytest.raises(ValueError, match="teacher returned"):
        tr._run_batch(x.to(DEV), y.to(DEV), batch_enum=0)


def test_distillation_pulls_the_student_to_the_teacher():
    """One fixed batch, no dropout, alpha = 1: the distillation term after 20 steps is below its first value."""
    m, opt, sched = _student()
    tr = _trainer(m, opt, sched, _Rec(), teacher_model=_teacher(), distill_kind="soft", distill_alpha=1.0,
                  distill_temperature=2.0)
    x, y = _data()[0][0]
    x, y = x.to(DEV), y.to(DEV)
    m.train()
    seen = []
    for i in range(20):
        tr._run_batch(x, y, batch_enum=i)
        seen.append(tr.distill_parts[1])  # device tensors: read once, after the loop
    seen = torch.stack(seen).cpu()
    assert torch.isfinite(seen).all() and seen[0] > 0
    assert seen[-1] < seen[0], seen.tolist()
