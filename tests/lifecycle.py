"""Weights across time (test infrastructure; a plain module, not a conftest).

The kernel tests judge one forward or one training step.  The helpers here judge what happens
BETWEEN steps: that a forward run after a parameter update computes with the updated parameters,
wherever the module keeps something derived from them (the prepared-weight caches of
sdpnet_engine.cached: fused / LayerNorm-folded / padded / cast weights, positional tables).

``oracle_trajectory``   several optimizer steps of the committed CPU oracle (autograd,
                        clip_grad_norm_, torch.optim.AdamW), with the parameters and the eval
                        logits on a validation batch after every step; fp64 is the reference,
                        fp32 shows what the number format alone costs.
``fresh_twin``          a module of the same construction that has never run a forward, loaded
                        with clones of the live module's state: its caches are built from the
                        current weights by construction and it runs the same kernels, so any
                        difference from the live module is a difference of state, not of rounding.
``assert_moved``        the guard of every test here: the quantity compared really changed
                        between the two points, so a test that cannot see the update fails.

LOGIT_CAP[config] is the condition the trajectory test's logit bound has to respect whatever is
measured: 1e-3 of the smallest per-step movement of that config's fp64 logits (0.40 on s_base, so
4e-4 there).
"""
import contextlib
import json
import os

import torch
import torch.nn.functional as F

import golden_util as gu
import sdpnet_oracle as orc
import synth

LS = 0.1
LR, WD, MAX_NORM, STEPS = 1.5e-3, 0.05, 5.0, 3
BATCH, XVAL_SEED = 4, 999
CONFIGS = ["s_base", "s_convemb", "s_poolhead_bias", "s_noqv"]
TRAJ_CONFIGS = ["s_base", "s_convemb", "s_poolhead_bias"]
# 1e-3 of the smallest per-step movement of each config's fp64 logits on xval (CPU oracle: s_base
# 0.401 / 0.498 / 0.666, s_convemb 0.415 / 0.510 / 0.689, s_poolhead_bias 0.091 / 0.114 / 0.163,
# rounded down); tests/test_lifecycle_selfcheck.py asserts the movements are at least 1e3 times these
LOGIT_CAP = {"s_base": 4.0e-4, "s_convemb": 4.1e-4, "s_poolhead_bias": 9.0e-5}

MANIFEST = json.load(open(os.path.join(gu.GOLDEN, "MANIFEST.json")))


def maxabs(a, b) -> float:
    a = torch.as_tensor(a).detach().to("cpu", torch.float64)
    b = torch.as_tensor(b).detach().to("cpu", torch.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) if a.numel() else 0.0


def assert_moved(a, b, floor: float, what: str = "") -> float:
    """max|a - b| > floor: the two points of the comparison are really different."""
    d = maxabs(a, b)
    assert d > floor, f"{what}: moved by {d:.3e}, not more than {floor:.1e} -- the test cannot see the update"
    return d


_CASE = {}


def case(name: str) -> dict:
    """Config (dropout and drop path off), synthetic weights and the batches of a small fixture
    (built once and shared; nobody modifies it)."""
    if name not in _CASE:
        _CASE[name] = _case(name)
    return _CASE[name]


def _case(name: str) -> dict:
    meta = MANIFEST[name]
    cfg = dict(meta["config"], ffn_dropout=0.0, attn_dropout=0.0)
    import model as ours
    torch.manual_seed(0)
    m = ours.MainModel.from_dict(**cfg)
    sd = synth.synth_state_dict(m, meta["wseed"])
    return dict(cfg=cfg, sd=sd, x=synth.synth_images(meta["xseed"], BATCH, meta["image"]),
                y=torch.arange(BATCH) % 7, xval=synth.synth_images(XVAL_SEED, BATCH, meta["image"]),
                nreg=meta["num_registers"], names=[k for k, _ in m.named_parameters()])


def oracle_trajectory(cfg, sd, x, y, xval, nreg, steps, lr, wd, max_norm, dtype, names=None):
    """``steps`` training steps of the CPU oracle in ``dtype``: cross entropy (label smoothing 0.1)
    on (x, y), autograd, clip_grad_norm_(max_norm), torch.optim.AdamW(lr, betas (0.9, 0.999),
    eps 1e-8, weight_decay wd).  ``names``: the trainable entries of ``sd`` (default: the
    parameters of MainModel(**cfg); a float buffer such as ConvEmbedding.bone is not trained).

    Returns dict(logits0, steps=[dict(params, logits, loss)]): the eval logits on ``xval`` before
    the first step, and after every step the full state (trained entries updated) and the eval
    logits on ``xval``, all detached in ``dtype``."""
    if names is None:
        import model as ours
        names = [k for k, _ in ours.MainModel.from_dict(**cfg).named_parameters()]
    state = {k: (v.detach().to(dtype).clone() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    leaves = [state[k].requires_grad_(True) for k in names]
    opt = torch.optim.AdamW(leaves, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    x, xval = x.to(dtype), xval.to(dtype)

    def ev():
        return orc.forward(xval, state, cfg, num_registers=nreg).detach().clone()

    out = dict(logits0=ev(), steps=[])
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(orc.forward.__wrapped__(x, state, cfg, num_registers=nreg), y, label_smoothing=LS)
        loss.backward()
        if max_norm:
            torch.nn.utils.clip_grad_norm_(leaves, max_norm)
        opt.step()
        out["steps"].append(dict(params={k: v.detach().clone() for k, v in state.items()}, logits=ev(),
                                 loss=float(loss.detach())))
    return out


_TRAJ = {}


def trajectories(name: str) -> dict:
    """case(name) plus its fp64 and fp32 oracle trajectories (computed once; never modified)."""
    if name not in _TRAJ:
        c = dict(case(name))
        for key, dt in (("t64", torch.float64), ("t32", torch.float32)):
            c[key] = oracle_trajectory(c["cfg"], c["sd"], c["x"], c["y"], c["xval"], c["nreg"], STEPS, LR, WD,
                                       MAX_NORM, dt, names=c["names"])
        _TRAJ[name] = c
    return _TRAJ[name]


def movements(traj: dict):
    """max|logits_k - logits_{k-1}| of a trajectory, one per step."""
    seq = [traj["logits0"]] + [s["logits"] for s in traj["steps"]]
    return [maxabs(a, b) for a, b in zip(seq[1:], seq[:-1])]


def deviation(traj: dict, ref: dict):
    """Per step: (max over tensors of max|param - ref|, its name, max|logits - ref logits|)."""
    rows = []
    for s, r in zip(traj["steps"], ref["steps"]):
        errs = sorted(((maxabs(s["params"][k], v), k) for k, v in r["params"].items() if v.is_floating_point()),
                      reverse=True)
        rows.append((errs[0][0], errs[0][1], maxabs(s["logits"], r["logits"])))
    return rows


def fresh_twin(model, make=None, inference: bool = False):
    """A module built like ``model`` that has never run a forward, holding clones of its state, in
    its mode, on its device.  MainModel is rebuilt from ``model.config``; a sub-module from
    ``make()``, a callable that constructs it with the arguments ``model`` was constructed with.
    ``inference``: built, loaded and moved under torch.inference_mode(), so its parameters are
    inference tensors like those of a model built that way."""
    with torch.inference_mode() if inference else contextlib.nullcontext():
        if make is None:
            assert getattr(model, "config", None), "fresh_twin: a module without .config needs make()"
            twin = type(model).from_dict(**model.config)
        else:
            twin = make()
        assert type(twin) is type(model)
        assert all("_sdp_cache" not in m.__dict__ for m in twin.modules())
        twin.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()})
        dev = next((p.device for p in model.parameters()), None)
        if dev is None:
            dev = next((b.device for b in model.buffers()), torch.device("cpu"))
        twin = twin.to(dev)
    twin.train(model.training)
    for attr in ("eval_fp32_stream", "final_rows", "num_streams"):
        if attr in model.__dict__:
            setattr(twin, attr, model.__dict__[attr])
    return twin


def same(a, b) -> bool:
    """torch.equal over a tensor or a tuple of tensors (shapes and dtypes included)."""
    if isinstance(a, torch.Tensor):
        a, b = (a,), (b,)
    return len(a) == len(b) and all(u.dtype == v.dtype and torch.equal(u, v) for u, v in zip(a, b))

