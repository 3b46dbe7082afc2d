"""Gradients of the HIP training path with dropout and drop path ON.

Model: embedding_dim 64, 4 heads, 2 blocks, patch 16 on 64x64 images (16 patches + 4 register
rows = 20 tokens), ffn_dropout = attn_dropout = 0.2, stochastic_depth_p = [0.3, 0.3], batch 6,
default activation, both ``conv_first`` values and one ``fast_att=False`` case;
``torch.manual_seed(s)`` before every forward (every mask seed and every drop-path draw comes
from torch's CPU generator, so the seeded forward is bit-reproducible).

Directional derivative (fp32).  The masks do not depend on the parameters, so the seeded
forward is a smooth function of them and its gradient can be checked without knowing any mask:
per parameter tensor, a fixed random direction v and a step h with h |v| = 3e-2 |theta|;
<grad, v> from one seeded backward against (L(theta + h v) - L(theta - h v)) / 2h of the seeded
forward, L computed from the returned logits in fp64 on the host.  The discrepancy of a tensor
is |<grad, v> - fd| / max(|<grad, v>|, |fd|, |grad| |v| / sqrt(numel)): relative to the
directional derivative, with the RMS size of a directional derivative of that gradient as the
least denominator, so a direction that happens to be nearly orthogonal to the gradient (1 in 50
is, to 2 %) is not judged on a chance cancellation.  ``*k_norm.bias`` (exact gradient zero, see
tests/grad_judge.py) is judged against the same layer's k_norm.weight scale.

Weights.  The synthetic weights, with every Linear / Conv2d weight multiplied by 10
(std 0.1, about 1 / sqrt(fan_in)).  With the plain synthetic weights (std 0.01) the method has
no power on this model: each branch's gradient passes two 0.01-scale weights, the conv-block
gradients are 1e-8 of the head's, the loss difference of a 1 % step is 1e-12 against 1e-10 of
fp32 forward rounding, and the p = 0 floor measured 1.9 (h |v| = 1e-2 |theta|) and 0.79
(1e-1 |theta|) -- neither a larger h nor fewer blocks changes a per-branch attenuation.

Tolerance.  Nobody had measured this, so it is derived: the identical procedure with all
dropouts at 0 -- where the analytic gradient is pinned to the oracle by
tests/test_gpu_train_matrix.py -- gives the method's noise floor, the worst discrepancy over
tensors: 1.081e-2 (conv_first) and 1.088e-2 (transformer first), both set by a conv-block
layer_norm_1.beta.  FLOOR = 1.1e-2 (rounded up), and the dropout-on tolerance is TOL = 4 x FLOOR
= 4.4e-2 (< 0.1); the margin covers the masks' 1 / (1 - p) amplification of rounding.  Measured with
dropout on: 3.5e-3 / 5.1e-3.  Power: judged against the central difference under seed s + 1
(other masks), 92 % / 89 % of the ``blocks.*`` tensors miss TOL (asserted: >= 3 / 4).
profiles/train_dropout_gradcheck.md has the table.  (In fp32 the ``fast_att=False`` case runs the
same kernels with the same p -- the manual attention path drops with the FFN dropout, 0.2 as
well -- so its figures equal conv_first's.)

bf16 against fp32 at the same seed.  Both dtypes draw the same four seeds per encoder layer and
the same host-side drop-path scales, and the FFN / head dropout masks are the same counter hash
of (seed, element index) in both.  The ATTENTION masks are not: the flash kernels keep an
element when ``hash4(seed, batch * H + head, query, key) >= thresh``
(csrc/attn_train.hip:29-45), the materialised softmax when
``uniform01(seed, row * N + column) >= p`` (csrc/train.hip:1740 and :1839, uniform01 at
csrc/common.h:122-125) -- two different hash functions, so the same seed gives different
masks (test_flash_and_softmax_attention_masks_differ pins that).  The bf16 case therefore runs
with attn_dropout = 0 (FFN and head dropout plus drop path); attention dropout in bf16 is
covered at kernel level by test_gpu_bf16_budget.py::test_flash_train_attention_budget.
"""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import grad_judge as gj
import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
CFG = dict(embedding_dim=64, n_head=4, num_blocks=2, conv_kernel_size=7, patch_size=16, max_image_size=[16, 16],
           head_output_from_register=True, output_classes=10, ffn_dropout=0.2, attn_dropout=0.2,
           stochastic_depth_p=[0.3, 0.3])
OFF = dict(ffn_dropout=0.0, attn_dropout=0.0, stochastic_depth_p=[0.0, 0.0])
B, IMG, NREG, WSEED, LS = 6, 64, 3, 231424314, 0.1
SEED = 1
WSCALE = 10.0         # Linear / Conv2d weights: synthetic x 10 (module docstring)
H_REL = 3e-2          # step: h * |v| = H_REL * |theta|, per tensor, the same with dropout on and off
FLOOR = 1.1e-2        # measured noise floor of the method at p = 0, 1.088e-2, rounded up (module docstring)
TOL = 4 * FLOOR       # 4.4e-2
assert TOL < 0.1

_X = synth.synth_images(0, B, IMG)
_Y = torch.arange(B) % 7


def _model(**over):
    import model as ours
    cfg = dict(CFG, **over)
    torch.manual_seed(0)
    m = ours.MainModel.from_dict(**cfg)
    m.load_state_dict(synth.synth_state_dict(m, WSEED))
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (torch.nn.Linear, torch.nn.Conv2d)):
                mod.weight.mul_(WSCALE)
    return cfg, m.to(DEV).train()


def _direction(name, p):
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    return torch.randn(p.shape, generator=g, dtype=torch.float64)


def _loss64(logits):
    """The loss from the returned logits, in fp64 on the host."""
    return float(F.cross_entropy(logits.detach().double().cpu(), _Y, label_smoothing=LS))


def _forward(m, seed, bf16=False):
    torch.manual_seed(seed)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        return m(_X.to(DEV), num_registers=NREG)


def _backward(m, seed, bf16=False):
    """(logits, {name: fp64 gradient on the host}) of one seeded forward + backward."""
    import sdpnet_train
    m.zero_grad(set_to_none=True)
    logits = _forward(m, seed, bf16)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        loss = sdpnet_train.cross_entropy(logits, _Y.to(DEV), LS)
    loss.backward()
    return logits.detach(), {k: p.grad.detach().double().cpu() for k, p in m.named_parameters()}


def _analytic(grads):
    """<grad, v> per tensor."""
    return {k: float((g * _direction(k, g)).sum()) for k, g in grads.items()}


def _central(m, seed, h_rel=H_REL):
    """(L(theta + h v) - L(theta - h v)) / 2h per tensor, of the seeded forward."""
    out = {}
    with torch.no_grad():
        for k, p in m.named_parameters():
            v = _direction(k, p)
            h = h_rel * float(p.detach().double().norm()) / float(v.norm())
            keep = p.detach().clone()
            step = (h * v).to(torch.float32).to(DEV)
            p.copy_(keep + step)
            lp = _loss64(_forward(m, seed))
            p.copy_(keep - step)
            lm = _loss64(_forward(m, seed))
            p.copy_(keep)
            out[k] = (lp - lm) / (2.0 * h)
    return out


def _drop_path_draws(m, seed):
    """The per-sample keep flags of every drop-path draw of a forward under ``seed``, replayed on
    the host as sdpnet_train draws them: one torch.randint for the mask seed base (_RNG), then one
    torch.rand(B) per active StochasticDepth in execution order (_drop_path_scale)."""
    import sdpnet_train
    torch.manual_seed(seed)
    torch.randint(0, 2 ** 62, (1,))
    draws = []
    for kind, mod in sdpnet_train.train_layers(m):
        sds = {"mixer": ("drop_path_2", "drop_path_1"), "enc": ("drop_path1", "drop_path2")}.get(kind, ())
        for attr in sds:
            p = sdpnet_train._drop_p(getattr(mod, attr))
            if p > 1e-5:
                draws.append(torch.rand(B) >= p)
    return draws


def _discrepancy(grads, fd):
    """Per tensor: |<grad, v> - fd| over max(|<grad, v>|, |fd|, |grad| |v| / sqrt(numel)); a
    ``k_norm.bias`` (exact gradient zero) over that last scale of the same layer's k_norm.weight."""
    a = _analytic(grads)
    out = {}
    for k, g in grads.items():
        ks = k[: -len("bias")] + "weight" if k.endswith(gj.EXEMPT_SUFFIX) else k
        rms = float(grads[ks].norm()) * float(_direction(ks, grads[ks]).norm()) / grads[ks].numel() ** 0.5
        den = rms if ks != k else max(abs(a[k]), abs(fd[k]), rms)
        out[k] = abs(a[k] - fd[k]) / den
    return out


def _worst(d, n=3):
    return [(k, f"{v:.2e}") for v, k in sorted(((v, k) for k, v in d.items()), reverse=True)[:n]]


CASES = {"conv_first": dict(conv_first=True), "transformer_first": dict(conv_first=False),
         "conv_first_slow_att": dict(conv_first=True, fast_att=False)}
_RUNS = {}


def _run(case):
    """Dropout-on model of a case: its seeded backward and the central differences under the same
    seed and under the next one (computed once, shared by the check and its power test)."""
    if case not in _RUNS:
        cfg, m = _model(**CASES[case])
        _, grads = _backward(m, SEED)
        _RUNS[case] = dict(grads=grads, same=_central(m, SEED), other=_central(m, SEED + 1))
    return _RUNS[case]


@pytest.mark.parametrize("conv_first", [True, False])
def test_seed_drops_and_keeps_samples_in_a_drop_path_draw(conv_first, monkeypatch):
    """Under SEED some drop-path draw drops one sample and keeps another (so a wrong drop-path group
    or scale changes the loss), shown by replaying torch.rand(B) on the host as _drop_path_scale
    draws it; the replay is checked against the scales the forward really used."""
    import sdpnet_train
    cfg, m = _model(conv_first=conv_first)
    used = []
    real = sdpnet_train._drop_path_scale

    def recording(p, nb, dev):
        s = real(p, nb, dev)
        if s is not None:
            used.append(s.cpu())
        return s

    monkeypatch.setattr(sdpnet_train, "_drop_path_scale", recording)
    with torch.no_grad():
        _forward(m, SEED)
    draws = _drop_path_draws(m, SEED)
    assert len(draws) == len(used) == 2 * (2 * 2 + 2)  # 2 blocks x (2 mixers + 1 encoder) x 2 branches
    for keep, s in zip(draws, used):
        assert torch.equal(keep.float() / (1.0 - 0.3), s)
    assert any(bool(k.any()) and not bool(k.all()) for k in draws), draws


@pytest.mark.parametrize("conv_first", [True, False])
def test_method_noise_floor_with_dropout_off(conv_first):
    """The measurement the tolerance is derived from, repeated: all dropouts at 0 (the analytic
    gradient is pinned to the oracle by test_gpu_train_matrix.py), the worst discrepancy over
    tensors stays at the recorded floor."""
    cfg, m = _model(conv_first=conv_first, **OFF)
    _, grads = _backward(m, SEED)
    d = _discrepancy(grads, _central(m, SEED))
    print(f"p = 0 floor, conv_first={conv_first}: {max(d.values()):.3e}", _worst(d))
    assert max(d.values()) <= FLOOR, _worst(d)


@pytest.mark.parametrize("case", list(CASES))
def test_directional_derivative_with_dropout_and_drop_path(case):
    """Every parameter tensor: <grad, v> of the seeded backward equals the central difference of
    the seeded forward within TOL = 4 x the p = 0 noise floor."""
    r = _run(case)
    d = _discrepancy(r["grads"], r["same"])
    print(f"dropout on, {case}: worst {max(d.values()):.3e} (TOL {TOL:.3e})", _worst(d))
    assert max(d.values()) <= TOL, _worst(d)


@pytest.mark.parametrize("case", list(CASES))
def test_directional_derivative_has_power_against_other_masks(case):
    """The backward under SEED against the central difference under SEED + 1 (other masks, other
    dropped samples) misses TOL for at least three quarters of the ``blocks.*`` tensors: a
    backward that regenerates a mask from the wrong seed does not pass the check above."""
    r = _run(case)
    d = {k: v for k, v in _discrepancy(r["grads"], r["other"]).items() if k.startswith("blocks.")}
    frac = sum(v > TOL for v in d.values()) / len(d)
    print(f"wrong seed, {case}: {frac:.2f} of {len(d)} block tensors miss TOL; median {np.median(list(d.values())):.2f}")
    assert frac >= 0.75, frac


@pytest.mark.parametrize("bf16", [False, True])
def test_fused_and_unfused_dropout_paths_agree(bf16, monkeypatch):
    """sdpnet_train._DMODE (the encoder's output-projection dropout fused into the drop-path /
    residual pass, or as its own launch): the same seed gives bit-identical logits and gradients
    within the fp32 rule of each other -- in fp32, and under bf16 autocast, where the fused form
    also writes the attention branch's gradient from the norm2 backward (dmode 2)."""
    import sdpnet_train
    cfg, m = _model(conv_first=True)
    out = {}
    for mode in (1, 0):
        monkeypatch.setattr(sdpnet_train, "_DMODE", mode)
        logits, grads = _backward(m, SEED, bf16)
        out[mode] = (logits.clone(), {k: g.numpy() for k, g in grads.items()})
    assert torch.equal(out[0][0], out[1][0])
    rows, _ = gj.fp32_report(out[0][1], out[1][1])
    print(f"unfused vs fused dropout, bf16={bf16}: worst", [(k, f"{q:.2e}") for q, _, _, k in rows[:3]])
    gj.assert_fp32(out[0][1], out[1][1], gj.qv_layers(cfg), what="_DMODE 0 vs 1")


@pytest.mark.parametrize("conv_first", [True, False])
def test_bf16_gradients_match_fp32_at_the_same_seed(conv_first):
    """attn_dropout = 0 (the flash and softmax attention masks differ, module docstring); FFN and
    head dropout 0.2 and drop path 0.3 on.  The same seed gives both dtypes the same masks and the
    same dropped samples, so the bf16 gradients are within the bf16 rule of the fp32 gradients of
    the same model: per tensor max|g_bf16 - g_fp32| <= 4 x the oracle's own CPU-autocast error
    against its fp64 gradients, taken from the same model with dropout off."""
    cfg, m = _model(conv_first=conv_first, attn_dropout=0.0)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    names = [k for k, _ in m.named_parameters()]
    _, g64 = gj.oracle_grads(cfg, sd, _X, _Y, NREG, LS, dtype=torch.float64)
    _, gac = gj.oracle_grads(cfg, sd, _X, _Y, NREG, LS, autocast=True)
    _, g32 = _backward(m, SEED)
    _, g16 = _backward(m, SEED, bf16=True)
    rows = gj.bf16_report(g16, g32, gac, names, ac_ref=g64)
    print(f"bf16 vs fp32 at one seed, conv_first={conv_first}: worst (error, autocast's)",
          [(k, f"{e:.2e}", f"{eac:.2e}") for _, e, eac, k in rows[:4]])
    bad = [r for r in rows if not r[0] <= 1.0]
    assert not bad, (len(bad), bad[:4])


def test_flash_and_softmax_attention_masks_differ():
    """The restriction of the bf16 case above rests on this: for one seed, the flash kernels' keep
    mask (sdp_attn_dropout_mask) and the one sdp_softmax_fwd applies are different masks, both
    with the asked keep rate."""
    import sdpnet_hip as sp
    Z, N, p, seed = 8, 24, 0.2, 0x1234567890ABCDEF & 0x7FFFFFFFFFFFFFFF
    flash = sp.attn_dropout_mask(Z, N, p, seed, DEV).bool()
    S = torch.zeros(Z * N, N, device=DEV)
    P, Pd = torch.empty_like(S), torch.empty_like(S)
    sp.softmax_fwd(S, P, Pd, Z * N, N, N, 1.0, p, seed)
    soft = (Pd > 0).view(Z, N, N)
    assert torch.allclose(P, torch.full_like(P, 1.0 / N))
    for mk in (flash, soft):  # 4608 Bernoulli(0.8) draws: sigma 0.006
        assert abs(float(mk.float().mean()) - (1 - p)) < 0.03
    agree = float((flash == soft).float().mean())
    print("flash vs softmax attention mask agreement", agree)
    assert agree < 0.75  # independent masks agree on 0.8^2 + 0.2^2 = 0.68 of the elements (sigma 0.007)
