"""Backward through the HIP training path for every small forward-fixture configuration.

The 24 ``s_*`` entries of tests/golden/MANIFEST.json cover every constructor switch (kernel
size, patch size, register count, head forms, q/k head norm, slow attention, biases, conv
embedding, the activations, head dims 12 / 16 / 128, batch 1).  Per case: synthetic weights and
images of the manifest entry, labels ``arange(B) % 7``, label smoothing 0.1, dropout off; the
reference is autograd through the CPU oracle in fp64, computed once per case and shared.

fp32: loss within 1e-5 and every parameter gradient within the per-tensor fp32 rule of
tests/grad_judge.py (1e-4 of that tensor's own largest gradient; the fp32 oracle sits within
2.7e-6 of the fp64 one judged this way, and the smallest tensor is 1e-7 of the largest).
bf16 (autocast, fp32 residual stream): each tensor's error against the fp64 reference within 4x
the oracle's own CPU-autocast-bf16 error for that tensor.  Counting wrappers around the flash
attention, the 8-phase weight-gradient GEMM and the materialised attention assert which path a
case took, not only that its numbers are right.  relu, leaky_relu and selu stay fp32 only: CPU
autocast alone is 0.12 to 0.23 off at own scale there, from mask flips at near-zero
pre-activations.

Measured on an MI355X: fp32 worst tensor 5.1e-6 of its own largest gradient (s_tanh,
blocks.1.t_block.q_proj.weight; every case <= 5.1e-6); bf16 worst 2.4x autocast's error (s_base,
blocks.0.conv_blocks.1.layer_norm_1.gamma, a tensor 1e-7 of the model's largest), every tensor of
every bf16 case on the single batch -- the statistical fallback of the rule is not used.
"""
import json
import os

import pytest
import torch

import golden_util as gu
import grad_judge as gj
import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
MANIFEST = json.load(open(os.path.join(gu.GOLDEN, "MANIFEST.json")))
CASES = sorted(k for k in MANIFEST if k.startswith("s_"))
assert len(CASES) == 24
# s_c256_h2 at batch 6: its token rows (>= 256) and 256 / 768 / 1024-wide layers take the 8-phase dW GEMM
BATCH = {"s_c256_h2": 6}
BF16_CASES = ["s_base", "s_tf", "s_c256_h2", "s_c96_h8", "s_p14", "s_nreg0", "s_k3", "s_noqv", "s_slowatt",
              "s_poolhead_bias"]
# flash attention needs bf16 and head_dim % 16 == 0; s_c96_h8 (head_dim 12) is the one bf16 case without it
FLASH = {k: k != "s_c96_h8" for k in BF16_CASES}
LS = 0.1

_REF = {}


def _ref(name):
    """Inputs and the fp64 oracle gradients of a case (computed once; never modified)."""
    if name not in _REF:
        import model as ours
        meta = MANIFEST[name]
        cfg = dict(meta["config"], ffn_dropout=0.0, attn_dropout=0.0)
        B = BATCH.get(name, meta["batch"])
        torch.manual_seed(0)
        m = ours.MainModel.from_dict(**cfg)
        sd = synth.synth_state_dict(m, meta["wseed"])
        x = synth.synth_images(meta["xseed"], B, meta["image"])
        y = torch.arange(B) % 7
        names = [k for k, _ in m.named_parameters()]
        loss, g64 = gj.oracle_grads(cfg, sd, x, y, meta["num_registers"], LS, dtype=torch.float64)
        assert set(names) <= set(g64)
        _REF[name] = dict(cfg=cfg, sd=sd, x=x, y=y, nreg=meta["num_registers"], names=names, loss=loss, g64=g64)
    return _REF[name]


def _ref_ac(name):
    r = _ref(name)
    if "gac" not in r:
        _, r["gac"] = gj.oracle_grads(r["cfg"], r["sd"], r["x"], r["y"], r["nreg"], LS, autocast=True)
    return r["gac"]


def _model(r):
    import model as ours
    torch.manual_seed(0)
    m = ours.MainModel.from_dict(**r["cfg"])
    m.load_state_dict(r["sd"])
    return m.to(DEV).train()


def _step(m, r, bf16):
    import sdpnet_train
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        logits = m(r["x"].to(DEV), num_registers=r["nreg"])
        loss = sdpnet_train.cross_entropy(logits, r["y"].to(DEV), LS)
    loss.backward()
    grads = {}
    for k, p in m.named_parameters():
        assert p.grad is not None, f"{k}: no gradient"
        assert p.grad.dtype == torch.float32 and p.grad.shape == p.shape, k
        grads[k] = p.grad.detach().cpu().numpy()
    return float(loss.detach()), grads


@pytest.fixture
def calls(monkeypatch):
    """Counters of the three paths: sp.attn_train_fwd (flash), sp.gemm_wgrad (8-phase dW),
    sdpnet_train._attn_materialized."""
    import sdpnet_hip as sp
    import sdpnet_train
    n = dict(flash=0, wgrad8=0, mat=0)

    def counted(key, fn):
        def wrapper(*a, **kw):
            n[key] += 1
            return fn(*a, **kw)
        return wrapper

    monkeypatch.setattr(sp, "attn_train_fwd", counted("flash", sp.attn_train_fwd))
    monkeypatch.setattr(sp, "gemm_wgrad", counted("wgrad8", sp.gemm_wgrad))
    monkeypatch.setattr(sdpnet_train, "_attn_materialized", counted("mat", sdpnet_train._attn_materialized))
    return n


@pytest.mark.parametrize("name", CASES)
def test_fp32_gradients_every_configuration(name, calls):
    r = _ref(name)
    loss, g = _step(_model(r), r, False)
    rows, _ = gj.fp32_report(g, r["g64"], r["names"])
    print(f"{name} fp32: loss {loss:.6f} (ref {r['loss']:.6f}); worst",
          [(k, f"{q:.2e}") for q, _, _, k in rows[:3]])
    assert abs(loss - r["loss"]) <= 1e-5, (loss, r["loss"])
    gj.assert_fp32(g, r["g64"], gj.qv_layers(r["cfg"]), r["names"], name)
    # fp32 never takes the bf16 kernels: attention materialised in every encoder layer
    assert calls["flash"] == 0 and calls["wgrad8"] == 0, calls
    assert calls["mat"] == r["cfg"]["num_blocks"] + 1, calls


@pytest.mark.parametrize("name", BF16_CASES)
def test_bf16_gradients_within_four_times_autocast(name, calls):
    r = _ref(name)
    gac = _ref_ac(name)
    loss, g = _step(_model(r), r, True)
    rows = gj.bf16_report(g, r["g64"], gac, r["names"])
    print(f"{name} bf16: loss {loss:.6f} (ref {r['loss']:.6f}); worst (error, autocast's)",
          [(k, f"{e:.2e}", f"{eac:.2e}") for _, e, eac, k in rows[:4]], "calls", calls)
    assert abs(loss - r["loss"]) <= 2e-2, (loss, r["loss"])
    layers = r["cfg"]["num_blocks"] + 1
    if FLASH[name]:
        assert calls["flash"] == layers and calls["mat"] == 0, calls
    else:
        assert calls["flash"] == 0 and calls["mat"] == layers, calls
    if name == "s_c256_h2":
        assert calls["wgrad8"] >= 1, calls
    if name == "s_c96_h8":
        assert calls["wgrad8"] == 0, calls
    gj.assert_bf16(g, r["g64"], gac, r["names"], name)


def test_tape_gradients_equal_eager_bit_for_bit():
    """s_base in fp32 through sdpnet_train.tape_forward / tape_backward (the torch.compile custom
    op's body).  The tape calls the same autograd Functions' forward and backward directly, in
    the same order, with the same arguments and the same seed draws (sdpnet_train.tape_forward
    is the same plan, sdpnet_train._plan, driven by Function.forward where train_forward drives it
    by Function.apply; every reduction is ordered, the side stream changes
    timing only), so its gradients equal the eager ones bit for bit -- and therefore pass the fp32
    rule against the oracle, which is asserted as well."""
    import sdpnet_train
    r = _ref("s_base")
    m = _model(r)
    _, eager = _step(m, r, False)
    m.zero_grad(set_to_none=True)
    xd, yd = r["x"].to(DEV), r["y"].to(DEV)
    logits, tape = sdpnet_train.tape_forward(m, xd, r["nreg"], torch.float32)
    lg = logits.detach().requires_grad_(True)
    sdpnet_train.cross_entropy(lg, yd, LS).backward()
    params = [p for _, p in m.named_parameters()]
    grads = sdpnet_train.tape_backward(tape, lg.grad, params)
    got = {k: gr.detach().cpu().numpy() for k, gr in zip(r["names"], grads)}
    gj.assert_fp32(got, r["g64"], gj.qv_layers(r["cfg"]), r["names"], "tape")
    diff = [k for k in r["names"] if not (got[k] == eager[k]).all()]
    assert not diff, diff
