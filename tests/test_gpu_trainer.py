"""GPU: the training loop of ``training_tools`` and the two kernels it adds.

* ``sdp_ema_update`` is bit-equal to ``d * e + (1 - d) * w`` in torch ops, and its reference mode
  reproduces the reference's own ``EMA_model`` state (tests/golden/trainer_ref.npz);
* ``sdp_bce_loss`` / ``sdp_bce_loss_soft`` against ``F.binary_cross_entropy_with_logits`` on the
  smoothed targets (the tolerances of the CE tests in test_gpu_train_kernels.py) and against the
  reference's loss and autograd gradient (fixture);
* ``Trainer.train()`` against the same loop written out here, state for state;
* the checkpoint / EMA files through ``eval_harness.return_model``, ``torch.optim.AdamW`` and
  a resuming second ``Trainer``.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import golden_util as gu
import sdpnet_hip as sp
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")


def rnd(*shape, seed=0, dtype=torch.float32, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def close(got, ref, rel, what=""):
    """As test_gpu_train_kernels.close: max abs error against rel * the reference's max magnitude."""
    got, ref = got.float(), ref.float()
    err = (got - ref).abs().max().item()
    scale = max(1.0, ref.abs().max().item()) if rel >= 1e-3 else max(1e-6, ref.abs().max().item())
    assert err <= rel * scale, f"{what}: max abs err {err:.3e} vs scale {scale:.3e} (rel tol {rel})"


@pytest.fixture(scope="module")
def ref():
    return gu.load_case("trainer_ref")


# --------------------------------------------------------------------------- sdp_ema_update
EMA_SHAPES = [(1,), (3,), (4095,), (4096,), (4097,), (8197,), (300, 70)]
GUARD = 4  # floats: keeps the 16-byte alignment of the allocation


def _guarded(shape, seed):
    """A tensor of ``shape`` inside a NaN-filled allocation (GUARD elements on each side)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), NAN, device=DEV)
    t = buf[GUARD:GUARD + n].view(shape)
    t.copy_(rnd(*shape, seed=seed))
    return buf, t


def _ema_tensors(seed):
    bufs, ts = [], []
    for i, shp in enumerate(EMA_SHAPES):
        b, t = _guarded(shp, seed + i)
        bufs.append(b)
        ts.append(t)
    # a contiguous view that starts 4 bytes into a 16-byte aligned tensor: element accesses only
    b, base = _guarded((4100,), seed + 50)
    bufs.append(b)
    ts.append(base[1:4098])
    assert ts[-1].data_ptr() % 16 == 4 and ts[0].data_ptr() % 16 == 0
    return bufs, ts


def _guards_intact(bufs, ts):
    for b, t in zip(bufs[:-1], ts[:-1]):
        n = t.numel()
        assert torch.isnan(b[:GUARD]).all() and torch.isnan(b[GUARD + n:]).all()
    b = bufs[-1]  # the view: its neighbours inside the base tensor hold data, the guards NaN
    assert torch.isnan(b[:GUARD]).all() and torch.isnan(b[GUARD + 4100:]).all()


def _ptrs(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("decay", [0.999, 0.9])
def test_ema_update_bit_equal_to_torch_ops(decay):
    ebufs, es = _ema_tensors(100)
    base_before = ebufs[-1].clone()
    blocks, nblocks = sp.mt_block_table([e.numel() for e in es], torch.device(DEV))
    assert nblocks == sum(-(-e.numel() // 4096) for e in es)
    sizes = torch.tensor([e.numel() for e in es], dtype=torch.int64, device=DEV)
    want = [e.clone() for e in es]
    for upd in range(3):
        wbufs, ws = _ema_tensors(200 + 10 * upd)
        wkeep = [b.clone() for b in wbufs]
        pe = _ptrs(es)
        sp.ema_update(pe, pe, _ptrs(ws), sizes, blocks, nblocks, decay, 1 - decay)
        want = [decay * e + (1 - decay) * w for e, w in zip(want, ws)]
        for i, (e, r) in enumerate(zip(es, want)):
            assert torch.equal(e, r), f"update {upd}, tensor {i} {tuple(e.shape)}"
        _guards_intact(ebufs, es)
        for b, k in zip(wbufs, wkeep):  # the weights (and their guards) are only read
            assert torch.equal(b.view(torch.int32), k.view(torch.int32))
    # around the unaligned view, the rest of its base tensor is untouched
    b = ebufs[-1]
    assert torch.equal(b[GUARD:GUARD + 1], base_before[GUARD:GUARD + 1])
    assert torch.equal(b[GUARD + 4098:GUARD + 4100], base_before[GUARD + 4098:GUARD + 4100])


def test_ema_update_reference_form_and_empty_list():
    """a = b = the weights: out = fl(fl(d w) + fl(c w)), whatever out held before."""
    ebufs, es = _ema_tensors(300)
    _, ws = _ema_tensors(400)
    blocks, nblocks = sp.mt_block_table([e.numel() for e in es], torch.device(DEV))
    sizes = torch.tensor([e.numel() for e in es], dtype=torch.int64, device=DEV)
    pw = _ptrs(ws)
    sp.ema_update(_ptrs(es), pw, pw, sizes, blocks, nblocks, 0.999, 1 - 0.999)
    for e, w in zip(es, ws):
        assert torch.equal(e, 0.999 * w + (1 - 0.999) * w)
    _guards_intact(ebufs, es)
    L = sp.lib()
    one = torch.zeros(2, dtype=torch.int64, device=DEV)
    assert L.sdp_ema_update(one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), 0,
                            0.5, 0.5, None) == 0                                     # nblocks == 0: no launch
    assert L.sdp_ema_update(None, one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), 1, 0.5, 0.5, None) == 1
    assert L.sdp_ema_update(one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), -1,
                            0.5, 0.5, None) == 1


class _Bag(nn.Module):
    def __init__(self, seed):
        super().__init__()
        self.ps = nn.ParameterList([nn.Parameter(rnd(*s, seed=seed + i)) for i, s in enumerate(EMA_SHAPES)])
        self.register_buffer("idx", torch.arange(7, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("quirks", [True, False])
def test_ema_class_matches_torch_expression(quirks):
    import sdpnet_train as st
    m = _Bag(500)
    ema = st.EMA(m, decay=0.9, reference_quirks=quirks)
    want = {k: v.clone() for k, v in m.state_dict().items()}
    for upd in range(3):
        with torch.no_grad():
            for i, p in enumerate(m.ps):
                p.add_(rnd(*p.shape, seed=600 + 10 * upd + i, scale=0.1))
            m.idx.add_(1)
        if upd == 2:  # a parameter reallocated between updates: the address tables are rebuilt
            m.ps[3].data = m.ps[3].data.clone()
        ema.update_parameters(m)
        for k, v in m.state_dict().items():
            if quirks:  # training_tools.py:295-297 as written
                want[k].copy_(v)
                want[k] = 0.9 * want[k] + (1 - 0.9) * v
            elif v.is_floating_point():
                want[k] = 0.9 * want[k] + (1 - 0.9) * v
            else:
                want[k] = v.clone()
        got = ema.state_dict()
        assert list(got) == list(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (upd, k)
    assert ema.state_dict()["idx"].dtype == (torch.float32 if quirks else torch.int32)


def _train_cf_model():
    import model as ours
    meta, _ = gu.load_case("train_cf")
    torch.manual_seed(0)
    m = ours.MainModel.from_dict(**meta["config"])
    sd = synth.synth_state_dict(m, meta["wseed"])
    assert gu.digest(sd) == meta["weights_sha256"]
    m.load_state_dict(sd)
    return meta, m, sd


def test_ema_reference_mode_matches_reference_fixture(ref):
    import training_tools as tt
    rmeta, arr = ref
    e = rmeta["ema"]
    meta, m, sd = _train_cf_model()
    assert meta["config"] == e["config"] and meta["wseed"] == e["wseed"]
    m = m.to(DEV)
    ema = tt.EMA_model(m, decay=e["decay"])
    sd = {k: v.clone() for k, v in sd.items()}
    for call in range(1, e["calls"] + 1):
        for k, v in sd.items():
            if v.is_floating_point():  # the fixture's seeded delta (gen_trainer_golden.perturbation)
                d = 1e-3 * synth.normal(synth.key_seed(e["seed"] + call, k), v.numel())
                v.add_(torch.from_numpy(d.astype(np.float32).reshape(tuple(v.shape))))
        m.load_state_dict(sd)
        ema.update_parameters(m)
    got = ema.state_dict()
    assert [[k, str(v.dtype)] for k, v in got.items()] == e["keys"]
    assert sum(1 for k, v in m.state_dict().items() if not v.is_floating_point()) == 3
    for k, v in got.items():
        assert v.dtype == torch.float32
        assert torch.equal(v.cpu(), torch.from_numpy(arr["ema/" + k])), k


# --------------------------------------------------------------------------- sdp_bce_loss
def _soft_targets(B, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, K, (B,), generator=g)
    b = torch.randint(0, K, (B,), generator=g)
    lam = torch.rand(B, 1, generator=g)
    return (lam * F.one_hot(a, K) + (1 - lam) * F.one_hot(b, K)).float().to(DEV)


def _bce_ref(logits, tgt, eps, K, grad_scale):
    """F.binary_cross_entropy_with_logits on the smoothed targets, fp32 on the device."""
    lr = logits.float().clone().requires_grad_(True)
    t = tgt if tgt.is_floating_point() else F.one_hot(tgt, K)
    loss = F.binary_cross_entropy_with_logits(lr, t * (1 - eps) + eps / K)
    (g,) = torch.autograd.grad(loss * grad_scale, lr)
    return loss.detach(), g


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,K", [(37, 1000), (1, 10)])
def test_bce_loss(dtype, eps, B, K):
    import sdpnet_train as st
    logits = rnd(B, K, seed=24, dtype=dtype, scale=3)
    labels = torch.randint(0, K, (B,), generator=torch.Generator().manual_seed(0)).to(DEV)
    soft = _soft_targets(B, K, 1)
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    for kind, tgt, fn in (("hard", labels, sp.bce_loss), ("soft", soft, sp.bce_loss_soft)):
        want, g = _bce_ref(logits, tgt, eps, K, 8.0)
        d = torch.empty_like(logits)
        loss = torch.zeros(1, device=DEV)
        fn(logits, tgt, eps, 8.0, d, loss)
        close(loss, want.view(1), 1e-5, f"bce loss ({kind})")
        close(d, g, tol, f"bce dlogits ({kind})")
        loss2 = torch.zeros(1, device=DEV)
        fn(logits, tgt, eps, 8.0, None, loss2)  # dlogits may be NULL
        close(loss2, want.view(1), 1e-5, f"bce loss without dlogits ({kind})")
        # the autograd entry point
        lr2 = logits.clone().requires_grad_(True)
        l2 = st.bce_with_logits(lr2, tgt, label_smoothing=eps, num_classes=K)
        assert l2.dim() == 0 and l2.dtype == torch.float32
        (l2 * 8.0).backward()
        close(l2.detach().view(1), want.view(1), 1e-5, f"bce_with_logits ({kind})")
        close(lr2.grad, g, tol, f"bce_with_logits grad ({kind})")


def test_bce_loss_matches_reference_fixture(ref):
    meta, arr = ref
    for K in meta["bce"]["K"]:
        logits = torch.from_numpy(arr[f"bce/K{K}/logits"]).to(DEV)
        tg = dict(hard=torch.from_numpy(arr[f"bce/K{K}/labels"]).to(DEV), soft=torch.from_numpy(arr[f"bce/K{K}/soft"]).to(DEV))
        for eps in meta["bce"]["eps"]:
            for kind, fn in (("hard", sp.bce_loss), ("soft", sp.bce_loss_soft)):
                d = torch.empty_like(logits)
                loss = torch.zeros(1, device=DEV)
                fn(logits, tg[kind], eps, 1.0, d, loss)
                pre = f"bce/K{K}/{kind}/eps{eps}/"
                close(loss, torch.tensor([float(arr[pre + "loss"])], device=DEV), 1e-5, pre + "loss")
                close(d, torch.from_numpy(arr[pre + "dlogits"]).to(DEV), 1e-5, pre + "dlogits")


def test_bce_loss_label_out_of_range_is_nan_not_oob():
    B, K = 8, 100
    logits = rnd(B, K, seed=28)
    labels = torch.tensor([0, 5, -7, 99, 100, 3, 7, 1], device=DEV)
    d = torch.empty_like(logits)
    loss = torch.zeros(1, device=DEV)
    sp.bce_loss(logits, labels, 0.0, 1.0, d, loss)
    torch.cuda.synchronize()
    assert torch.isnan(loss).all()
    bad = torch.isnan(d).all(dim=1).cpu()
    assert bad.tolist() == [False, False, True, False, True, False, False, False]
    assert not torch.isnan(d[~bad.to(DEV)]).any()


# --------------------------------------------------------------------------- Trainer
# a warm-up that starts at half the rate, so that two epochs move the weights well past rounding
SCHED = dict(constant_scheduler=dict(factor=0.5, total_iters=1), linear_scheduler=dict(start_factor=0.5, total_iters=2),
             cosine=dict(T_0=4, eta_min=1e-5))
OPT = dict(lr=0.0015, weight_decay=0.05)
LS, DECAY, EPOCHS = 0.1, 0.999, 2


class _Sampler:
    def __init__(self):
        self.epochs = []

    def set_epoch(self, epoch):
        self.epochs.append(epoch)


class _Loader(list):
    """An in-memory DataLoader: a list of (images, targets) batches with a ``sampler``."""

    def __init__(self, batches):
        super().__init__(batches)
        self.sampler = _Sampler()


class _Rec:
    """A loss logger that keeps every batch loss."""

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
    train = [(x[i], y[i]) for i in range(3)]
    return train, [(x[3], y[3])]


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


def _new(use_ce):
    import training_tools as tt
    _, m, _ = _train_cf_model()
    m = m.to(DEV)
    opt, sched = tt.return_scheduler_optimizer(m, optimizer_config=OPT, scheduler_config=SCHED)
    return m, opt, sched


@functools.lru_cache(maxsize=None)
def _trainer_run(use_ce, accum, quirks):
    import training_tools as tt
    import training_utilities as tu
    train, val = _data()
    m, opt, sched = _new(use_ce)
    rec = _Rec()
    loader = _Loader(train)
    tr = tt.Trainer(m, loader, _Loader(val), opt, sched, 0, save_every=1000, gradient_accumulation_steps=accum,
                    val_loss_logger=tu.distributed_loss_track(wandb_log=False, task="Val"), train_loss_logger=rec,
                    val_accuracy_logger=tu.track_accuracy(wandb_log=False), snapshot_dir="no_such_snapshot_dir",
                    total_epochs=EPOCHS + 1, ema_decay=DECAY, use_cross_entropy=use_ce, label_smoothing=LS,
                    reference_quirks=quirks)
    assert tr.fused and not isinstance(tr.model, nn.parallel.DistributedDataParallel)
    tr.train()
    assert loader.sampler.epochs == [1, 2] and tr.epoch == EPOCHS and not m.training
    assert all(l.is_cuda and l.dim() == 0 and not l.requires_grad for l in rec.seen)
    return _state(m, opt, sched, tr.ema_model, rec.seen)


@functools.lru_cache(maxsize=None)
def _hand_run(use_ce, accum, quirks):
    """Trainer.train() written out from the same pieces (training_tools.py:77-160)."""
    import sdpnet_train as st
    train, _ = _data()
    m, opt, sched = _new(use_ce)
    ema = st.EMA(m, decay=DECAY, reference_quirks=quirks)
    losses = []
    for _ in range(EPOCHS):
        m.train()
        for i, (x, y) in enumerate(train):
            x, y = x.to(DEV), y.to(DEV)
            if quirks:
                opt.zero_grad(set_to_none=True)
            with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                out = m(x)
                loss = st.cross_entropy(out, y, LS) if use_ce else st.bce_with_logits(out, y, LS, 10)
            opt.scale(loss).backward()
            if (i + 1) % accum == 0:
                opt.step(grad_scale=None, max_norm=5.0)
                if not quirks:
                    opt.zero_grad(set_to_none=True)
            ema.update_parameters(m)
            losses.append(loss.detach())
        sched.step()
    return _state(m, opt, sched, ema, losses)


@pytest.mark.parametrize("use_ce", [True, False])
@pytest.mark.parametrize("accum,quirks", [(1, True), (2, True), (2, False)])
def test_trainer_matches_hand_written_loop(use_ce, accum, quirks):
    got, want = _trainer_run(use_ce, accum, quirks), _hand_run(use_ce, accum, quirks)
    assert list(got) == list(want)
    steps = {EPOCHS * (3 // accum)}
    assert {int(v) for k, v in got.items() if k.startswith("s/")} == steps
    for k in want:
        if k == "losses":
            assert got[k].shape == (EPOCHS * 3,) and torch.isfinite(got[k]).all()
            close(got[k], want[k], 1e-5, "batch losses")
        else:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    # the average really is one: in reference mode it sits within 1 ulp of the weights, otherwise it lags
    lag = max((got["e/" + k[2:]].float() - v).abs().max().item() for k, v in got.items()
              if k.startswith("p/") and v.is_floating_point())
    assert (lag < 1e-6) if quirks else (lag > 1e-4)


@pytest.mark.parametrize("use_ce", [True, False])
def test_reference_quirks_switch_changes_the_result(use_ce):
    a, b = _trainer_run(use_ce, 2, True), _trainer_run(use_ce, 2, False)
    assert any(not torch.equal(a[k], b[k]) for k in a if k.startswith("p/"))
    assert any(not torch.equal(a[k], b[k]) for k in a if k.startswith("e/"))


def test_checkpoint_round_trip_under_ddp(tmp_path, monkeypatch):
    import torch.distributed as dist

    import eval_harness as eh
    import training_tools as tt
    import training_utilities as tu
    monkeypatch.chdir(tmp_path)  # the EMA file goes to the working directory (training_tools.py:287, :302)
    train, val = _data()

    def trainer(total_epochs):
        m, opt, sched = _new(True)
        loader = _Loader(train)
        tr = tt.Trainer(m, loader, _Loader(val), opt, sched, 0, save_every=1, gradient_accumulation_steps=1,
                        val_loss_logger=tu.distributed_loss_track(wandb_log=False, task="Val"),
                        train_loss_logger=tu.distributed_loss_track(wandb_log=False),
                        val_accuracy_logger=tu.track_accuracy(wandb_log=False), snapshot_dir=str(tmp_path),
                        total_epochs=total_epochs, ema_decay=DECAY, use_cross_entropy=True, label_smoothing=LS)
        return tr, m, opt, sched, loader

    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'store'}", rank=0, world_size=1)
    try:
        tr, m, opt, sched, _ = trainer(2)
        assert isinstance(tr.model, nn.parallel.DistributedDataParallel) and tr.epoch == 0
        tr.train()
        ck = torch.load(tmp_path / "model.pt", map_location="cpu", weights_only=True)
        assert sorted(ck) == ["epoch", "model_config", "model_state_dict", "optimizer_state", "scheduler_state"]
        assert ck["epoch"] == 1 and ck["model_config"] == m.config
        assert all(k.startswith("module.") for k in ck["model_state_dict"])
        ema_file = torch.load(tmp_path / "ema_model.pt", map_location="cpu", weights_only=True)
        assert list(ema_file) == list(ck["model_state_dict"])
        # model_test.py's loader takes both files
        model, ema_model = eh.return_model(str(tmp_path), "model.pt", "ema_model.pt")
        for k, v in m.state_dict().items():
            assert torch.equal(model.state_dict()[k], v.cpu()), k
            if v.is_floating_point():  # reference mode: the stored value is within 1 ulp of the weight
                assert torch.allclose(ema_model.state_dict()[k], v.cpu(), rtol=1e-6, atol=0), k
        # every step count is a 0-d tensor of its own, and torch.optim.AdamW takes the state
        steps = [st_["step"] for st_ in ck["optimizer_state"]["state"].values()]
        assert len(steps) == len(list(m.parameters())) and all(s.dim() == 0 and float(s) == 3.0 for s in steps)
        assert len({s.untyped_storage().data_ptr() for s in steps}) == len(steps)
        tadam = torch.optim.AdamW(m.parameters())
        tadam.load_state_dict(ck["optimizer_state"])
        p0 = next(m.parameters())
        assert torch.equal(tadam.state[p0]["exp_avg"], opt.state[p0]["exp_avg"])
        # a second Trainer on the same directory resumes after the saved epoch
        tr2, m2, opt2, sched2, loader2 = trainer(3)
        assert tr2.epoch == 1
        for (k, a), (k2, b) in zip(m.state_dict().items(), m2.state_dict().items()):
            assert k == k2 and torch.equal(a, b), k
        for p, p2 in zip(m.parameters(), m2.parameters()):
            assert torch.equal(opt.state[p]["exp_avg"], opt2.state[p2]["exp_avg"])
            assert torch.equal(opt.state[p]["exp_avg_sq"], opt2.state[p2]["exp_avg_sq"])
            assert float(opt2.state[p2]["step"]) == 3.0
        assert sched2.get_last_lr() == sched.get_last_lr() and sched2.last_epoch == 1
        tr2.train()
        assert loader2.sampler.epochs == [2] and tr2.epoch == 2
        assert all(float(opt2.state[p]["step"]) == 6.0 for p in m2.parameters())
    finally:
        dist.destroy_process_group()
