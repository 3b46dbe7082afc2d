"""GPU: every forward sees the weights the last update wrote.

The eval forward keeps prepared weights on the modules (sdpnet_engine.cached: the fused and
LayerNorm-folded wqkv / w1 of every encoder, the folded ConvMixer weights, the padded patch weight,
the head's padded Linears, bf16 casts, the positional tables), keyed on the parameters' version
counters and addresses.  The fused optimizer writes parameters from inside a kernel, through raw
addresses; it has to make those writes visible (sdpnet_train.AdamW.step bumps the counters), or a
later forward computes with last step's derived weights and this step's everything else.

Two references, used together (tests/lifecycle.py):

* ``fresh_twin``: a module that never ran a forward, loaded with the live module's state.  Same
  kernels, caches built from the current weights by construction: live and twin must be equal BIT
  FOR BIT, in every path (fp32, bf16 autocast, the fp32-stream eval, raw outputs, the hooked
  module-by-module path, num_registers=0), for the model, for each sub-module on its own, for the
  training forwards that take a positional table from the cache, and for what Trainer.validate()
  logs.  One stale ulp fails.
* the fp64 oracle trajectory: three fused fp32 steps against autograd + clip_grad_norm_ +
  torch.optim.AdamW on the CPU oracle, every parameter tensor and the eval logits after every step.

Every comparison is guarded by ``assert_moved``: the quantity compared changed between the two
points by more than a floor (logits: 1e-2 per step; the CPU oracle moves them by 0.40 / 0.50 / 0.67
on s_base), so a test that cannot see the step fails instead of passing.

Trajectory bounds (TRAJ_BOUND below): 4x the deviation from the fp64 trajectory measured on an
MI355X (profiles/lifecycle_trajectory.md holds every figure, next to the CPU oracle's own
fp32-vs-fp64 deviation); the logit bound is additionally capped at lifecycle.LOGIT_CAP, 1e-3 of the
config's smallest per-step logit movement.  tests/test_lifecycle_selfcheck.py shows a stale-cache
forward missing that cap by 36x or more.
"""
import pytest
import torch
import torch.nn as nn

import lifecycle as lc
import sdpnet_oracle as orc
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")

# name -> (bf16 autocast, eval_fp32_stream, return_raw_outputs, forward hook on blocks[0], num_registers)
PATHS = {
    "fp32": (False, False, False, False, None),
    "bf16": (True, False, False, False, None),
    "fp32_stream": (True, True, False, False, None),
    "raw": (False, False, True, False, None),
    "hooked": (False, False, False, True, None),
    "nreg0": (False, False, False, False, 0),
}
LOGIT_FLOOR = 1e-2

# (parameters, logits): 4x the largest deviation from the fp64 oracle trajectory over the three
# steps, measured on an MI355X (profiles/lifecycle_trajectory.md); logits also <= lc.LOGIT_CAP
TRAJ_BOUND = {
    "s_base": (4 * 8.59e-6, 4 * 1.56e-6),           # blocks.0.t_block.v_proj.weight; logits at step 3
    "s_convemb": (4 * 1.89e-5, 4 * 1.70e-6),        # blocks.1.t_block.ff_linear2.weight; step 3
    "s_poolhead_bias": (4 * 1.03e-5, 4 * 1.59e-7),  # conv_init.conv.weight; step 3
}


def _noop_hook(module, inputs, output):
    return None


def _autocast(on):
    return torch.autocast("cuda", dtype=torch.bfloat16, enabled=on)


class _Run:
    """A live MainModel of a small fixture on one eval path, with its training batch."""

    def __init__(self, name, path):
        import model as ours
        self.c = c = lc.case(name)
        self.bf16, stream, self.raw, self.hook, nreg = PATHS[path]
        self.nreg = c["nreg"] if nreg is None else nreg
        torch.manual_seed(0)
        m = ours.MainModel.from_dict(**c["cfg"])
        m.load_state_dict(c["sd"])
        self.m = m.to(DEV)
        if stream:
            self.m.eval_fp32_stream = True
        if self.hook:
            self.m.blocks[0].register_forward_hook(_noop_hook)
        self.x, self.y, self.xval = c["x"].to(DEV), c["y"].to(DEV), c["xval"].to(DEV)

    def eval(self, mod=None):
        mod = self.m if mod is None else mod
        mod.eval()
        with _autocast(self.bf16):
            out = mod(self.xval, num_registers=self.nreg, return_raw_outputs=self.raw)
        return out if isinstance(out, tuple) else (out,)

    def twin_eval(self, **kw):
        twin = lc.fresh_twin(self.m, **kw)
        if self.hook:
            twin.blocks[0].register_forward_hook(_noop_hook)
        return self.eval(twin)

    def backward(self):
        import sdpnet_train
        self.m.train()
        self.m.zero_grad(set_to_none=True)
        with _autocast(self.bf16):
            logits = self.m(self.x, num_registers=self.nreg)
            loss = sdpnet_train.cross_entropy(logits, self.y, lc.LS)
        loss.backward()


def _fused(m):
    import sdpnet_train
    return sdpnet_train.AdamW(m.parameters(), lr=lc.LR, weight_decay=lc.WD)


# ------------------------------------------------------------------ (a) eval after the fused step
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", lc.CONFIGS)
def test_eval_sees_the_fused_step_bit_for_bit(name, path):
    r = _Run(name, path)
    opt = _fused(r.m)
    prev = r.eval()  # warms every cache
    assert lc.same(prev, r.twin_eval())
    for step in range(lc.STEPS):
        r.backward()
        opt.step(grad_scale=1.0, max_norm=lc.MAX_NORM)
        out = r.eval()
        moved = lc.assert_moved(out[0], prev[0], LOGIT_FLOOR, f"{name}/{path} step {step + 1}")
        print(f"{name}/{path} step {step + 1}: logits moved {moved:.3f}")
        twin = r.twin_eval()
        bad = [i for i, (a, b) in enumerate(zip(out, twin)) if not torch.equal(a, b)]
        assert len(out) == len(twin) and not bad, (
            f"{name}/{path} step {step + 1}: eval differs from a fresh twin at the same weights, outputs {bad}, "
            f"max|diff| {[lc.maxabs(out[i], twin[i]) for i in bad]}")
        prev = out
    # a step GradScaler semantics skip (one gradient element inf): nothing may change, bit for bit
    r.backward()
    next(r.m.parameters()).grad.view(-1)[0] = INF
    before = {k: v.detach().clone() for k, v in r.m.state_dict().items()}
    opt.step(grad_scale=None, max_norm=lc.MAX_NORM)
    assert all(torch.equal(v, before[k]) for k, v in r.m.state_dict().items())
    assert lc.same(r.eval(), prev) and lc.same(r.twin_eval(), prev)


# ------------------------------------------------------------------ (b) the control
@pytest.mark.parametrize("path", ["fp32", "bf16"])
@pytest.mark.parametrize("name", lc.CONFIGS)
def test_eval_sees_a_stock_optimizer_step(name, path):
    """torch.optim.SGD updates in place through torch, which bumps the version counters itself.
    lr 0.05: the fp32 CPU oracle's logits move by 0.14 to 0.22 per step at it (gradient norm 1.6
    to 2.0, under the clip)."""
    r = _Run(name, path)
    opt = torch.optim.SGD(r.m.parameters(), lr=0.05)
    prev = r.eval()
    for step in range(lc.STEPS):
        r.backward()
        opt.step()
        out = r.eval()
        lc.assert_moved(out[0], prev[0], LOGIT_FLOOR, f"{name}/{path} SGD step {step + 1}")
        assert lc.same(out, r.twin_eval()), (name, path, step)
        prev = out


# ------------------------------------------------------------------ (c) sub-modules on their own
def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _modules():
    """name -> (constructor, forward arguments); inputs as tests/test_gpu_train_modules.py builds them."""
    from layers import (Block, ClassificationHead, ConvEmbedding, ConvMixer, ConvPatcher, EmbeddingLayer,
                        EncoderLayer, FinalBlock, LayerNorm)
    x, reg = _rand(2, 64, 7, 6, seed=6), _rand(2, 3, 64, seed=4)
    off = dict(ff_dropout=0.0, att_dropout=0.0, drop_p=0.0)
    return {
        # 3 * 16 * 16 = 768 columns: no K padding, the fp32 weight is the parameter itself
        "patcher_p16": (lambda: ConvPatcher(64, 16), (_rand(2, 3, 70, 48, seed=2),)),
        # 3 * 4 * 4 = 48 columns padded to 64: a copy in every dtype
        "patcher_p4": (lambda: ConvPatcher(64, 4), (_rand(2, 3, 22, 12, seed=2),)),
        "embedding": (lambda: EmbeddingLayer(64, max_num_registers=5, max_image_size=[16, 16], activation=nn.GELU()),
                      (x, 2)),
        "conv_embedding": (lambda: ConvEmbedding(64, kernel_size=5, max_image_size=[16, 16], activation=nn.GELU(),
                                                 trainable_bone=True), (x, 3)),
        "conv_mixer": (lambda: ConvMixer(64, kernel_size=5, mixer_ffn_bias=True, mixer_deptwise_bias=True, drop_p=0.0),
                       (x,)),
        "encoder": (lambda: EncoderLayer(64, n_head=4, activation_func=nn.GELU(), **off), (x, reg)),
        "block": (lambda: Block(embedding_dim=64, n_head=4, conv_block_num=2, multiplication_factor=4,
                                conv_kernel_size=7, conv_first=True, **off), (x, reg)),
        "final_block": (lambda: FinalBlock(64, n_head=4, activation_func=nn.GELU(), multiplication_factor=4, **off),
                        (x, reg)),
        "head_register": (lambda: ClassificationHead(64, 10, from_register=True, dropout=0.0, bias=True),
                          (None, _rand(3, 4, 64, seed=1))),
        "head_pool": (lambda: ClassificationHead(64, 10, from_register=False, dropout=0.0, bias=True),
                      (_rand(3, 64, 5, 4, seed=2), None)),
        "layernorm": (lambda: LayerNorm(64), (x,)),
    }


MODULES = ["patcher_p16", "patcher_p4", "embedding", "conv_embedding", "conv_mixer", "encoder", "block",
           "final_block", "head_register", "head_pool", "layernorm"]
# AdamW's first step moves every parameter with a gradient by lr = 1.5e-3 and the outputs are O(1)
# sums over 64 or more of them; 1e-4 is a tenth of one parameter's move
MODULE_FLOOR = 1e-4


def _call(mod, args, bf16=False):
    """Forward on fresh copies of the inputs (EmbeddingLayer's eval forward adds in place)."""
    a = [t.clone().to(DEV) if isinstance(t, torch.Tensor) else t for t in args]
    with _autocast(bf16):
        out = mod(*a)
    return out if isinstance(out, tuple) else (out,)


def _square_loss(outs):
    return sum(o.float().square().mean() for o in outs)


def _live_module(make, seed=21):
    mod = make()
    mod.load_state_dict(synth.synth_state_dict(mod, seed))
    return mod.to(DEV)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("which", MODULES)
def test_submodule_eval_sees_the_fused_step(which, bf16):
    import sdpnet_train
    make, args = _modules()[which]
    mod = _live_module(make)
    opt = sdpnet_train.AdamW(mod.parameters(), lr=lc.LR, weight_decay=lc.WD)
    mod.eval()
    prev = _call(mod, args, bf16)  # warms the cache
    assert lc.same(prev, _call(lc.fresh_twin(mod, make), args, bf16))
    mod.train()
    _square_loss(_call(mod, args)).backward()
    opt.step(grad_scale=1.0, max_norm=lc.MAX_NORM)
    mod.eval()
    out = _call(mod, args, bf16)
    moved = max(lc.maxabs(a, b) for a, b in zip(out, prev))
    print(f"{which} {'bf16' if bf16 else 'fp32'}: outputs moved {moved:.3e}")
    assert moved > MODULE_FLOOR, (which, moved)
    twin = _call(lc.fresh_twin(mod, make), args, bf16)
    assert lc.same(out, twin), (which, [lc.maxabs(a, b) for a, b in zip(out, twin)])


# ------------------------------------------------------------------ (d) training forward on a cached table
def _emb_oracle(which, sd, params, x, nreg, steps):
    """``steps`` steps of autograd + clip_grad_norm_ + torch.optim.AdamW on the oracle's embedding
    layer in fp64, loss as _square_loss; returns the parameters after the last."""
    state = {"embedding_layer." + k: (v.double().clone() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    names = ["embedding_layer." + k for k in params]
    leaves = [state[k].requires_grad_(True) for k in names]
    opt = torch.optim.AdamW(leaves, lr=lc.LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=lc.WD)
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        if which == "embedding":
            outs = orc.embedding_layer(x.double(), state, nreg, "gelu")
        else:
            outs = orc.conv_embedding_layer(x.double(), state, nreg, 5, "gelu")
        _square_loss_64(outs).backward()
        torch.nn.utils.clip_grad_norm_(leaves, lc.MAX_NORM)
        opt.step()
    return {k[len("embedding_layer."):]: state[k].detach() for k in names}


def _square_loss_64(outs):
    return sum(o.square().mean() for o in outs)


@pytest.mark.parametrize("which", ["embedding", "conv_embedding"])
def test_training_forward_takes_the_current_positional_table(which):
    """Standalone EmbeddingLayer / ConvEmbedding(trainable_bone=True) in train(): the forward adds a
    positional table that comes from the cache and is derived from parameters the step trains.
    Second forward equal to a fresh twin's; parameters after two steps within 1e-5 of the same two
    steps on the oracle (the bound of test_adamw_step_matches_reference)."""
    import sdpnet_train
    make, (_, nreg) = _modules()[which]
    x = _rand(4, 64, 7, 7, seed=9)
    mod = make()
    sd = synth.synth_state_dict(mod, 22)
    params = [k for k, _ in mod.named_parameters()]
    assert ("bone" in params) == (which == "conv_embedding")
    mod.load_state_dict(sd)
    mod = mod.to(DEV).train()
    opt = sdpnet_train.AdamW(mod.parameters(), lr=lc.LR, weight_decay=lc.WD)
    first = None
    for step in range(2):
        mod.zero_grad(set_to_none=True)
        outs = _call(mod, (x, nreg))
        if step == 0:
            first = [o.detach().clone() for o in outs]
        else:
            moved = max(lc.maxabs(a, b) for a, b in zip(outs, first))
            assert moved > MODULE_FLOOR, (which, moved)
            twin = lc.fresh_twin(mod, make)
            assert twin.training
            touts = _call(twin, (x, nreg))
            assert lc.same([o.detach() for o in outs], [o.detach() for o in touts]), (
                which, [lc.maxabs(a, b) for a, b in zip(outs, touts)])
        _square_loss(outs).backward()
        opt.step(grad_scale=1.0, max_norm=lc.MAX_NORM)
    ref = _emb_oracle(which, sd, params, x, nreg, 2)
    errs = {k: lc.maxabs(p, ref[k]) for k, p in mod.named_parameters()}
    print(which, "parameters after 2 steps vs fp64 oracle:", {k: f"{e:.2e}" for k, e in errs.items()})
    assert set(errs) == set(ref) and max(errs.values()) <= 1e-5, errs


# ------------------------------------------------------------------ (e) trajectory against the oracle
def trajectory_deviation(name):
    """Three fused fp32 steps of the live model; per step (worst parameter deviation from the fp64
    oracle trajectory, its name, logit deviation, logit movement)."""
    c = lc.trajectories(name)
    r = _Run(name, "fp32")
    opt = _fused(r.m)
    prev = r.eval()[0]
    rows = []
    for step in range(lc.STEPS):
        r.backward()
        opt.step(grad_scale=1.0, max_norm=lc.MAX_NORM)
        logits = r.eval()[0]
        want = c["t64"]["steps"][step]
        sd = r.m.state_dict()
        floats = [k for k, v in want["params"].items() if v.is_floating_point()]
        assert set(c["names"]) <= set(floats) <= set(sd)
        errs = sorted(((lc.maxabs(sd[k], want["params"][k]), k) for k in floats), reverse=True)
        rows.append((errs[0][0], errs[0][1], lc.maxabs(logits, want["logits"]), lc.maxabs(logits, prev)))
        prev = logits
    return rows


@pytest.mark.parametrize("name", lc.TRAJ_CONFIGS)
def test_three_fused_steps_follow_the_fp64_oracle_trajectory(name):
    rows = trajectory_deviation(name)
    c = lc.trajectories(name)
    own = lc.deviation(c["t32"], c["t64"])
    for k, (row, o) in enumerate(zip(rows, own)):
        print(f"{name} step {k + 1}: params {row[0]:.2e} ({row[1]}) [oracle fp32 {o[0]:.2e}], "
              f"logits {row[2]:.2e} [oracle fp32 {o[2]:.2e}], moved {row[3]:.3f}")
    pb, lb = TRAJ_BOUND[name]
    assert lb <= lc.LOGIT_CAP[name]
    for k, row in enumerate(rows):
        assert row[3] > LOGIT_FLOOR, (name, k, row)
        assert row[0] <= pb, (name, k + 1, "parameters", row[:2], pb)
        assert row[2] <= lb, (name, k + 1, "logits", row[2], lb)


# ------------------------------------------------------------------ (f) Trainer.validate()
class _ValRec:
    """A validation logger that keeps what update() receives."""

    def __init__(self):
        self.seen = []

    def update(self, *a, **kw):
        v = a[0] if a else kw["batch_accuracy"]
        self.seen.append(v.detach().clone())

    def log(self):
        return 0.0


def test_trainer_validate_reports_the_model_it_has():
    """Trainer.validate() is eval() + an fp32 forward: from epoch 2 on it meets caches warmed by
    the previous epoch's validation, after a whole epoch of fused steps."""
    import sdpnet_hip as sp
    import test_gpu_trainer as tg
    import training_tools as tt
    train, val = tg._data()
    m, opt, sched = tg._new(True)
    vloss, vacc, snaps = _ValRec(), _ValRec(), []
    tr = tt.Trainer(m, tg._Loader(train), tg._Loader(val), opt, sched, 0, save_every=1000,
                    gradient_accumulation_steps=1, val_loss_logger=vloss, train_loss_logger=tg._Rec(),
                    val_accuracy_logger=vacc, snapshot_dir="no_such_snapshot_dir", total_epochs=3,
                    ema_decay=tg.DECAY, use_cross_entropy=True, label_smoothing=tg.LS, reference_quirks=True)
    assert tr.fused
    validate = tr.validate

    def recording_validate():
        snaps.append({k: v.detach().clone() for k, v in m.state_dict().items()})
        validate()

    tr.validate = recording_validate
    tr.train()
    assert len(snaps) == len(vloss.seen) == len(vacc.seen) == 2
    (xv, yv), = val
    xv, yv = xv.to(DEV), yv.to(DEV)
    for epoch, snap in enumerate(snaps):
        m.load_state_dict(snap)
        twin = lc.fresh_twin(m).eval()
        with torch.no_grad():
            met = sp.logits_metrics(twin(xv).contiguous(), yv.to(torch.int64), 0.0)
        print(f"epoch {epoch + 1}: logged loss {float(vloss.seen[epoch]):.6f}, twin {float(met[:, 0].mean()):.6f}")
        assert torch.equal(vloss.seen[epoch], met[:, 0].mean()), (epoch + 1, vloss.seen[epoch], met[:, 0].mean())
        assert torch.equal(vacc.seen[epoch], met[:, 2].sum()), (epoch + 1, vacc.seen[epoch], met[:, 2].sum())
    # three fused steps lie between the two validations (the loss is O(1); 1e-4 of it is far above
    # what rounding alone could move)
    lc.assert_moved(vloss.seen[0], vloss.seen[1], 1e-4, "validation loss, epoch 1 -> 2")


# ------------------------------------------------------------------ (g) writes nobody can see
def test_invalidate_after_a_data_write():
    import sdpnet_engine
    r = _Run("s_base", "fp32")
    prev = r.eval()
    r.m.blocks[0].t_block.ff_linear1.weight.data.mul_(1.5)  # no version bump, same address
    sdpnet_engine.invalidate(r.m)
    out = r.eval()
    lc.assert_moved(out[0], prev[0], 1e-6, "ff_linear1.weight * 1.5")
    assert lc.same(out, r.twin_eval())


def test_load_state_dict_onto_inference_tensor_parameters():
    """A model built under torch.inference_mode() (TeacherModel runs its forward there): its
    parameters have no version counter and load_state_dict copies into them at the same address."""
    import model as ours
    c = lc.case("s_base")
    other = synth.synth_state_dict(ours.MainModel.from_dict(**c["cfg"]), 4242)
    xval = c["xval"].to(DEV)
    with torch.inference_mode():
        m = ours.MainModel.from_dict(**c["cfg"])
        m.load_state_dict(c["sd"])
        m = m.to(DEV).eval()
        assert all(p.is_inference() for p in m.parameters())
        prev = m(xval, num_registers=c["nreg"])
        m.load_state_dict(other)
        out = m(xval, num_registers=c["nreg"])
        lc.assert_moved(out, prev, LOGIT_FLOOR, "load_state_dict of other weights")
        twin = lc.fresh_twin(m, inference=True)
        assert all(p.is_inference() for p in twin.parameters()) and not twin.training
        assert torch.equal(out, twin(xval, num_registers=c["nreg"]))
