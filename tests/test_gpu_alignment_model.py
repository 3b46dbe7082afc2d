"""GPU: whole-model forwards on operands the public surface can hand the kernels off their natural
alignment (the kernel-level twin is test_gpu_alignment.py).

* Flat parameters: every parameter rebound as a view of one fp32 buffer, the first 4 B past a 16-B
  boundary and the following at 4, 8 and 12 (mod 16) in turn -- what _flatten_dense_tensors, a
  bucket view or a packing checkpoint loader produce.  Biases, LayerNorm and q / k norm vectors,
  depthwise weights and tables then reach the kernels as they lie.
* Sliced input: an image batch that is contiguous at a storage offset of one element.
* Flat gradients: every ``.grad`` a view of one flat buffer (``gradient_as_bucket_view=True``) through
  one training step, judged per tensor and against a twin model.

The logits must meet the bounds test_gpu_model.py holds ordinary tensors to, against the same golden
logits; a refusal of the C layer that reaches the caller as an exception fails the test."""
import numpy as np
import pytest
import torch

import golden_util as gu
from test_gpu_alignment import flat_views, pads_untouched
from test_gpu_model import BF16_TOL, FP32_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = ["s_base", "s_tf"]   # conv_first, and the transformer-first twin
_MODELS = {}


def flat_model(name):
    """(model in eval mode with every parameter a view of one flat fp32 buffer, meta, arrays, x, the
    buffer as int32, the mask of its pad elements); cached per case."""
    if name not in _MODELS:
        import model as ours
        meta, arr = gu.load_case(name)
        torch.manual_seed(0)
        m = ours.MainModel.from_dict(**meta["config"])
        sd, x = gu.build_inputs(meta, m)
        assert gu.digest(sd) == meta["weights_sha256"]
        m.load_state_dict(sd)
        m = m.to(DEV).eval()
        ps = [p for p in m.parameters()]
        assert all(p.dtype == torch.float32 and p.is_contiguous() for p in ps)
        views, ibuf, pad = flat_views([p.numel() for p in ps], 0, first=4, fill=0.0)
        for p, v in zip(ps, views):
            v.copy_(p.detach().reshape(-1))
            p.data = v.view(p.shape)
        assert {p.data_ptr() % 16 for p in ps} == {4, 8, 12}
        _MODELS.clear()
        _MODELS[name] = (m, meta, arr, x, ibuf, pad)
    return _MODELS[name]


def _err(y, arr):
    return float(np.abs(y.float().cpu().numpy() - arr["logits"]).max())


@pytest.mark.parametrize("name", CASES)
def test_flat_parameters_fp32(name):
    m, meta, arr, x, ibuf, pad = flat_model(name)
    y = m(x.to(DEV), num_registers=meta["num_registers"])
    err = _err(y, arr)
    print(f"ALIGN model {name} flat parameters fp32: max abs err {err:.3e} (bound {FP32_TOL})")
    assert err <= FP32_TOL
    assert pads_untouched(ibuf, pad), "a forward wrote between the parameters"


@pytest.mark.parametrize("mode", ["default", "low_latency", "mx_fp8"])
@pytest.mark.parametrize("name", CASES + ["m_cf_b2"])   # M: the fast GEMM, flash attention and MX tiers apply
def test_flat_parameters_bf16_autocast(name, mode, monkeypatch):
    """Which path ran is counted: a planned split-K call runs on sdp_gemm_splitk only when
    _splitk_aligned accepts its operands (a flat bias sends it back to sdp_gemm); the MX pair runs on
    m_cf_b2 only (C = 64 of the small cases is no multiple of 128), through the aligned copies of
    layers._mx_weights."""
    import sdpnet_hip as sp
    n = dict(planned=0, accepted=0, splitk=0, mx=0)
    g0, sk0, mx0 = sp.gemm, sp.gemm_splitk, sp.gemm_mx

    def gemm(x, w, y, M, N, K, bias=None, resid=None, act=0, resid_pre=False, ln=None, part=None):
        if sp.low_latency_enabled() and x.t.dtype == torch.bfloat16 and \
                sp.gemm_split_plan(M, N, K, sp._cus(y.t.device)) is not None:
            n["planned"] += 1
            n["accepted"] += bool(sp._splitk_aligned(x, w, y, bias, resid, ln, part))
        return g0(x, w, y, M, N, K, bias=bias, resid=resid, act=act, resid_pre=resid_pre, ln=ln, part=part)

    def count(key, fn):
        def wrapper(*a, **kw):
            n[key] += 1
            return fn(*a, **kw)
        return wrapper
    monkeypatch.setattr(sp, "gemm", gemm)
    monkeypatch.setattr(sp, "gemm_splitk", count("splitk", sk0))
    monkeypatch.setattr(sp, "gemm_mx", count("mx", mx0))
    m, meta, arr, x, ibuf, pad = flat_model(name)
    m.low_latency, m.mx_fp8 = mode == "low_latency", mode == "mx_fp8"
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(x.to(DEV), num_registers=meta["num_registers"])
    finally:
        m.low_latency, m.mx_fp8 = None, None
    print(f"ALIGN model {name} {mode}: paths {n}")
    assert n["splitk"] == n["accepted"], n
    if mode == "low_latency" and name == "m_cf_b2":
        assert n["planned"] > 0, n
    assert (n["mx"] > 0) == (mode == "mx_fp8" and name == "m_cf_b2"), n
    if mode != "low_latency":
        assert n["planned"] == 0, n
    assert y.dtype == torch.bfloat16
    err = _err(y, arr)
    print(f"ALIGN model {name} flat parameters bf16 autocast {mode}: max abs err {err:.3e} (bound {BF16_TOL})")
    assert err <= BF16_TOL
    assert pads_untouched(ibuf, pad), "a forward wrote between the parameters"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", CASES)
def test_input_at_a_storage_offset_of_one_element(name, dtype):
    """x[..., 1:]-style: the batch is contiguous, its first element 4 B (fp32) / 2 B (bf16) into the
    storage, so patchify and the first layer see an image base off every vector boundary."""
    m, meta, arr, x, _, _ = flat_model(name)
    buf = torch.zeros(x.numel() + 1, dtype=dtype, device=DEV)
    xs = buf[1:].view(x.shape)
    xs.copy_(x)
    assert xs.is_contiguous() and xs.data_ptr() % 16 == xs.element_size()
    y = m(xs, num_registers=meta["num_registers"])
    err, tol = _err(y, arr), FP32_TOL if dtype == torch.float32 else BF16_TOL
    print(f"ALIGN model {name} input at one element {dtype}: max abs err {err:.3e} (bound {tol})")
    assert err <= tol


# --------------------------------------------------------------------------- flat gradients
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_flat_gradients_one_training_step(bf16):
    """Every ``.grad`` is a view of one flat fp32 buffer at 4, 8 and 12 B (mod 16), set before the
    backward as ``gradient_as_bucket_view=True`` does.  One step of s_base: forward, backward, the
    fused AdamW with clipping.  The gradients stay in the views and pass tests/grad_judge.py exactly
    as in test_gpu_train_matrix.py (same reference, same rule); the updated parameters equal, bit for
    bit, those of a twin model with ordinary tensors given the same gradients; no pad float of the
    buffer is written."""
    import grad_judge as gj
    import sdpnet_train
    import test_gpu_train_matrix as tm
    r = tm._ref("s_base")
    m, twin = tm._model(r), tm._model(r)
    ps, pt = [p for _, p in m.named_parameters()], [p for _, p in twin.named_parameters()]
    views, ibuf, pad = flat_views([p.numel() for p in ps], 0, first=4, fill=0.0)
    for p, v in zip(ps, views):
        p.grad = v.view(p.shape)
    ptrs = [p.grad.data_ptr() for p in ps]
    assert {q % 16 for q in ptrs} == {4, 8, 12}
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        logits = m(r["x"].to(DEV), num_registers=r["nreg"])
        loss = sdpnet_train.cross_entropy(logits, r["y"].to(DEV), tm.LS)
    loss.backward()
    assert [p.grad.data_ptr() for p in ps] == ptrs, "a gradient left its view of the flat buffer"
    g = {k: p.grad.detach().cpu().numpy() for k, p in zip(r["names"], ps)}
    if bf16:
        assert abs(float(loss) - r["loss"]) <= 2e-2
        gj.assert_bf16(g, r["g64"], tm._ref_ac("s_base"), r["names"], "s_base flat gradients")
    else:
        assert abs(float(loss) - r["loss"]) <= 1e-5
        gj.assert_fp32(g, r["g64"], gj.qv_layers(r["cfg"]), r["names"], "s_base flat gradients")
    for p, q in zip(ps, pt):
        q.grad = p.grad.detach().clone()
        assert q.grad.data_ptr() % 16 == 0
    oa, ob = sdpnet_train.AdamW(ps, lr=1e-3, weight_decay=0.05), sdpnet_train.AdamW(pt, lr=1e-3, weight_decay=0.05)
    oa.step(grad_scale=1.0, max_norm=1.0)
    ob.step(grad_scale=1.0, max_norm=1.0)
    torch.cuda.synchronize()
    diff = [k for k, p, q in zip(r["names"], ps, pt) if not torch.equal(p.detach(), q.detach())]
    assert not diff, f"parameters differ from the twin's after the step: {diff[:4]}"
    moved = sum(not torch.equal(p.detach().cpu(), r["sd"][k]) for k, p in zip(r["names"], ps))
    assert moved > len(ps) // 2, "the step did not update the parameters"
    assert pads_untouched(ibuf, pad), "a pad float between the gradients was written"
