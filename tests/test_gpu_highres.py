"""GPU: patch grids above 16 x 16 (384-512 px inputs).

* ``sdp_dw_wgrad`` above 640 pixels per plane runs the row-banded kernel (csrc/train.hip).  Exact
  data: A and DY hold integers in [-3, 3], so every product and partial sum is an integer below
  2^24 and the result equals the fp64 reference whatever the order of additions; the shapes put a
  band boundary at many different rows, so a wrong halo row or a double-counted boundary row
  changes an integer.  General data: the ``randn`` operands of test_gpu_train_kernels.test_dw_wgrad
  element-wise within (n + 2) 2^-24 sum |dy| |a| of the fp64 result of the stored values, n =
  B H W (the sequential worst case, valid for any order); repeated calls bit-equal.  The bounds:
  625 and 640 pixels still run the whole-plane kernel under the same rule; W = 200 at k = 7 is
  refused and leaves ``part`` untouched.
* A small model at a 28 x 26 grid (728 tokens): training loss and gradients under the rules of
  test_gpu_train_matrix.py, eval logits under the standing bounds, one fused AdamW step.
* A checkpoint moved to another grid (sdpnet_engine.with_max_image_size) against the oracle
  loaded with the same resampled state.

* The tiled matrix-core depthwise conv (dwconv3t_mfma, csrc/norm_dw.hip) for H > 16 or W > 16:
  ``sdp_dwconv_variant`` says which kernel a shape takes; exact data (x integers in [-2, 2], w in
  {-1, 0, 1}, bias integers in [-3, 3]: |y| <= 2 * 49 + 3 = 101 is exact in bf16) must equal the
  fp64 conv on shapes with one extra row or column, partial tiles on both edges and interior
  tiles (the kernel is routed by measurement, so 17 x 16 and 16 x 17 run dwconv2_nhwc and the
  one-row tile edge is covered by 33 x 40); the tier-3 rounding model of test_gpu_bf16_budget.test_dwconv_mfma_budget, copied here,
  holds with the same element bound and RMS margin.
"""
import ctypes

import pytest
import torch

import bf16_budget as bb
import grad_judge as gj
import sdpnet_hip as sp
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

BANDED = [(2, 26, 25, 40, 7), (1, 27, 27, 64, 7), (3, 32, 32, 96, 5), (1, 41, 17, 32, 9), (2, 19, 40, 72, 3),
          (1, 7, 100, 32, 7), (70, 26, 26, 32, 3)]
WHOLE = [(1, 25, 25, 32, 7), (1, 20, 32, 32, 7)]


def rnd(*shape, seed=0, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype).to(DEV)


def ints(*shape, seed, lo, hi, dtype):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype).to(DEV)


def wgrad64(a, dy, B, H, W, C, k):
    """fp64 on the CPU from the stored operand values: (dW [C, k*k], sum |dy| |a| [C, k*k])."""
    P = k // 2
    a = torch.nn.functional.pad(a.detach().cpu().double().view(B, H, W, C), (0, 0, P, P, P, P))
    dy = dy.detach().cpu().double().view(B, H, W, C)
    ref = torch.empty(C, k * k, dtype=torch.float64)
    sabs = torch.empty(C, k * k, dtype=torch.float64)
    for ty in range(k):
        for tx in range(k):
            win = a[:, ty:ty + H, tx:tx + W]
            ref[:, ty * k + tx] = (dy * win).sum((0, 1, 2))
            sabs[:, ty * k + tx] = (dy.abs() * win.abs()).sum((0, 1, 2))
    return ref, sabs


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("B,H,W,C,k", BANDED)
def test_dw_wgrad_banded_exact(dtype, B, H, W, C, k):
    a = ints(B * H * W, C, seed=41, lo=-3, hi=3, dtype=dtype)
    dy = ints(B * H * W, C, seed=42, lo=-3, hi=3, dtype=dtype)
    assert H * W > 640 and 9 * B * H * W < 2 ** 24
    got = sp.dw_wgrad(sp.dense(a), sp.dense(dy), B, H, W, C, k)
    ref, _ = wgrad64(a, dy, B, H, W, C, k)
    assert got.dtype == torch.float32 and got.shape == (C, k * k)
    assert torch.equal(got.cpu().double(), ref), (got.cpu().double() - ref).abs().max()


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("B,H,W,C,k", BANDED + WHOLE)
def test_dw_wgrad_general_within_sequential_bound(dtype, B, H, W, C, k):
    a = rnd(B * H * W, C, seed=22, dtype=dtype)
    dy = rnd(B * H * W, C, seed=23, dtype=dtype)
    got = sp.dw_wgrad(sp.dense(a), sp.dense(dy), B, H, W, C, k)
    again = sp.dw_wgrad(sp.dense(a), sp.dense(dy), B, H, W, C, k)
    ref, sabs = wgrad64(a, dy, B, H, W, C, k)
    bb.assert_elementwise(got.cpu(), ref, (B * H * W + 2) * 2.0 ** -24 * sabs, f"dw_wgrad {(B, H, W, C, k)} {dtype}")
    assert torch.equal(got, again)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_dw_wgrad_refuses_what_cannot_be_staged(dtype):
    B, H, W, C, k = 1, 4, 200, 32, 7   # 800 pixels; one DY row with 7 A rows is 200 KiB
    a = rnd(B * H * W, C, seed=22, dtype=dtype)
    dy = rnd(B * H * W, C, seed=23, dtype=dtype)
    with pytest.raises(ValueError, match=r"1280 / \(k \+ 1\) = 160"):
        sp.dw_wgrad(sp.dense(a), sp.dense(dy), B, H, W, C, k)
    L = sp.lib()
    part = torch.full((L.sdp_dw_wgrad_chunks(B), C * k * k), float("nan"), device=DEV)
    rc = L.sdp_dw_wgrad(sp.dcode(dtype), *sp.dense(a).args(), *sp.dense(dy).args(), B, H, W, C, k,
                        ctypes.c_void_p(part.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 1, rc   # hipErrorInvalidValue
    assert bool(torch.isnan(part).all())
    # the widest plane the contract takes at k = 7 above 640 pixels
    B, H, W = 1, 5, 160
    a = ints(B * H * W, C, seed=43, lo=-3, hi=3, dtype=dtype)
    dy = ints(B * H * W, C, seed=44, lo=-3, hi=3, dtype=dtype)
    got = sp.dw_wgrad(sp.dense(a), sp.dense(dy), B, H, W, C, k)
    assert torch.equal(got.cpu().double(), wgrad64(a, dy, B, H, W, C, k)[0])


# ---------------------------------------------------------------------------
# A model at a 28 x 26 grid
CFG = dict(embedding_dim=64, num_blocks=1, n_head=2, conv_kernel_size=7, patch_size=4, conv_block_num=2,
           max_image_size=[28, 28], max_num_registers=5, output_classes=10, ffn_dropout=0.0, attn_dropout=0.0)
MODEL_CASES = {"table": CFG, "bone": dict(CFG, conv_embedding=True, conv_embedding_kernel_size=5)}
NREG, LS = 3, 0.1
_REF = {}


def _ref(name):
    """Inputs, the fp64 oracle gradients and the oracle's eval logits (computed once, never modified)."""
    if name not in _REF:
        import model as ours
        import sdpnet_oracle as orc
        cfg = MODEL_CASES[name]
        torch.manual_seed(0)
        m = ours.MainModel.from_dict(**cfg)
        sd = synth.synth_state_dict(m, 20260384)
        x = torch.randn(2, 3, 112, 104, generator=torch.Generator(device="cpu").manual_seed(384))
        y = torch.arange(2) % 7
        names = [k for k, _ in m.named_parameters()]
        loss, g64 = gj.oracle_grads(cfg, sd, x, y, NREG, LS, dtype=torch.float64)
        assert set(names) <= set(g64)
        _REF[name] = dict(cfg=cfg, sd=sd, x=x, y=y, names=names, loss=loss, g64=g64,
                          logits=orc.forward(x, sd, cfg, num_registers=NREG))
    return _REF[name]


def _model(r):
    import model as ours
    torch.manual_seed(0)
    m = ours.MainModel.from_dict(**r["cfg"])
    m.load_state_dict(r["sd"])
    return m.to(DEV)


def _step(m, r, bf16):
    import sdpnet_train
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        logits = m(r["x"].to(DEV), num_registers=NREG)
        loss = sdpnet_train.cross_entropy(logits, r["y"].to(DEV), LS)
    loss.backward()
    grads = {}
    for k, p in m.named_parameters():
        assert p.grad is not None, f"{k}: no gradient"
        grads[k] = p.grad.detach().cpu().numpy()
    return float(loss.detach()), grads


@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_train_fp32_at_28x26(name):
    import sdpnet_train
    r = _ref(name)
    m = _model(r).train()
    loss, g = _step(m, r, False)
    rows, _ = gj.fp32_report(g, r["g64"], r["names"])
    print(f"{name} fp32: loss {loss:.6f} (ref {r['loss']:.6f}); worst", [(k, f"{q:.2e}") for q, _, _, k in rows[:3]])
    assert abs(loss - r["loss"]) <= 1e-5, (loss, r["loss"])
    gj.assert_fp32(g, r["g64"], gj.qv_layers(r["cfg"]), r["names"], name)
    # one fused optimizer step runs and changes every parameter
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    sdpnet_train.AdamW(m.parameters(), lr=1e-2, weight_decay=0.05).step()
    torch.cuda.synchronize()
    same = [k for k, p in m.named_parameters() if torch.equal(p.detach(), before[k])]
    assert not same, same
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_train_bf16_at_28x26(name):
    r = _ref(name)
    if "gac" not in r:
        _, r["gac"] = gj.oracle_grads(r["cfg"], r["sd"], r["x"], r["y"], NREG, LS, autocast=True)
    loss, g = _step(_model(r).train(), r, True)
    rows = gj.bf16_report(g, r["g64"], r["gac"], r["names"])
    print(f"{name} bf16: loss {loss:.6f} (ref {r['loss']:.6f}); worst (error, autocast's)",
          [(k, f"{e:.2e}", f"{eac:.2e}") for _, e, eac, k in rows[:4]])
    assert abs(loss - r["loss"]) <= 2e-2, (loss, r["loss"])
    gj.assert_bf16(g, r["g64"], r["gac"], r["names"], name)


@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_eval_at_28x26(name):
    r = _ref(name)
    m = _model(r).eval()
    x = r["x"].to(DEV)
    with torch.no_grad():
        e32 = (m(x, num_registers=NREG).float().cpu() - r["logits"]).abs().max().item()
        e16 = (m(x.to(BF), num_registers=NREG).float().cpu() - r["logits"]).abs().max().item()
    print(f"{name} eval 28x26: fp32 max|err| {e32:.2e}, bf16 {e16:.2e}")
    assert e32 <= 1e-3 and e16 <= 1e-2, (e32, e16)


@pytest.mark.parametrize("conv_embedding", [False, True])
def test_moved_checkpoint_equals_oracle_with_resampled_state(conv_embedding):
    """[14, 14] -> the smallest size that holds a 24 x 20 grid, run at that grid: [20, 24] for the
    tables (the one sized by max_image_size[1] is indexed by rows), [24, 20] for the bone (rows
    first).  The oracle loaded with the same resampled state is the reference."""
    import model as ours
    import sdpnet_engine as eng
    import sdpnet_oracle as orc
    cfg = dict(CFG, max_image_size=[14, 14], conv_embedding=conv_embedding, conv_embedding_kernel_size=5)
    torch.manual_seed(0)
    m = ours.MainModel.from_dict(**cfg)
    m.load_state_dict(synth.synth_state_dict(m, 77))
    size = [24, 20] if conv_embedding else [20, 24]
    big = eng.with_max_image_size(m.to(DEV).eval(), size)
    assert big.config["max_image_size"] == size and not big.training
    sd, cfg2 = eng.resize_positions({k: v.cpu() for k, v in m.state_dict().items()}, cfg, size)
    for k, v in big.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
    x = torch.randn(2, 3, 96, 80, generator=torch.Generator(device="cpu").manual_seed(5))
    ref = orc.forward(x, sd, cfg2, num_registers=NREG)
    with torch.no_grad():
        e32 = (big(x.to(DEV), num_registers=NREG).float().cpu() - ref).abs().max().item()
        e16 = (big(x.to(DEV).to(BF), num_registers=NREG).float().cpu() - ref).abs().max().item()
    print(f"moved checkpoint at 24x20: fp32 max|err| {e32:.2e}, bf16 {e16:.2e}")
    assert e32 <= 1e-3 and e16 <= 1e-2, (e32, e16)


# ---------------------------------------------------------------------------
# The tiled matrix-core depthwise conv
def conv64(x, w, k):
    """x fp64 [B, H, W, C], w fp64 [C, k, k]: 'same' cross-correlation per channel, by shifts."""
    B, H, W, C = x.shape
    p = k // 2
    xp = torch.zeros(B, H + 2 * p, W + 2 * p, C, dtype=torch.float64, device=x.device)
    xp[:, p:p + H, p:p + W] = x
    out = torch.zeros_like(x)
    for ky in range(k):
        for kx in range(k):
            out += xp[:, ky:ky + H, kx:kx + W] * w[:, ky, kx]
    return out


def test_dwconv_variant_query():
    L = sp.lib()
    assert L.sdp_dwconv_set_kernel(0) == 3
    assert L.sdp_dwconv_variant(1, 28, 28, 64, 7) == 5
    assert L.sdp_dwconv_variant(1, 16, 16, 64, 7) == 3
    # routed by measurement (profiles/highres.md): k = 3 from 28 x 28 up, not at 24 x 24; tiles less
    # than 9/16 full stay on dwconv2_nhwc
    assert L.sdp_dwconv_variant(1, 28, 28, 64, 3) == 5 and L.sdp_dwconv_variant(1, 24, 24, 64, 3) == 2
    assert L.sdp_dwconv_variant(1, 24, 24, 64, 5) == 5 and L.sdp_dwconv_variant(1, 24, 24, 64, 7) == 5
    assert L.sdp_dwconv_variant(1, 17, 16, 32, 7) == 2 and L.sdp_dwconv_variant(1, 16, 17, 32, 3) == 2
    assert L.sdp_dwconv_variant(1, 28, 28, 36, 9) == 1      # k = 9 and C % 8 != 0: the general kernel
    assert L.sdp_dwconv_variant(1, 28, 28, 40, 7) == 2      # C % 32 != 0: no MFMA form
    assert L.sdp_dwconv_variant(0, 28, 28, 64, 7) == 2      # fp32
    assert L.sdp_dwconv_variant(1, 28, 28, 64, 4) == -1 and L.sdp_dwconv_variant(2, 28, 28, 64, 7) == -1
    old = L.sdp_dwconv_set_kernel(2)
    try:
        assert L.sdp_dwconv_variant(1, 28, 28, 64, 7) == 2 and L.sdp_dwconv_variant(1, 16, 16, 64, 7) == 2
        L.sdp_dwconv_set_kernel(1)
        assert L.sdp_dwconv_variant(1, 28, 28, 64, 7) == 1
    finally:
        L.sdp_dwconv_set_kernel(old)
    assert L.sdp_dwconv_variant(1, 28, 28, 64, 7) == 5


@pytest.mark.parametrize("B,H,W,C,k,variant", [(2, 17, 16, 32, 7, 2), (1, 16, 17, 32, 3, 2), (1, 28, 26, 64, 7, 5),
                                             (2, 33, 40, 96, 5, 5), (1, 56, 56, 32, 7, 5)])
def test_dwconv_tiled_exact(B, H, W, C, k, variant):
    """The two planes with one extra row or column fill 17/32 of their two tiles and are routed to
    dwconv2_nhwc (the tiled kernel was not measured there); 33 x 40 keeps a one-row tile edge and a
    half-width one on the tiled kernel, 28 x 26 partial tiles on both edges, 56 x 56 interior tiles."""
    M = B * H * W
    x = ints(M, C, seed=51, lo=-2, hi=2, dtype=BF)
    w = ints(C, k * k, seed=52, lo=-1, hi=1, dtype=torch.float32)
    b = ints(C, seed=53, lo=-3, hi=3, dtype=torch.float32)
    assert sp.lib().sdp_dwconv_variant(1, H, W, C, k) == variant
    y = torch.full((M, C), float("nan"), dtype=BF, device=DEV)
    sp.dwconv(sp.dense(x), w, b, sp.dense(y), B, H, W, C, k)
    torch.cuda.synchronize()
    ref = conv64(x.double().view(B, H, W, C), w.double().view(C, k, k), k) + b.double()
    bad = (y.double().view(B, H, W, C) != ref).nonzero()
    assert len(bad) == 0, (len(bad), bad[:4].tolist())


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("B,H,W,C,k", [(1, 28, 26, 64, 7), (2, 24, 24, 32, 5)])
def test_dwconv_tiled_budget(B, H, W, C, k, ln):
    """The tier-3 model of test_gpu_bf16_budget.test_dwconv_mfma_budget on the tiled kernel: the
    fp32 weights and the LayerNorm'd input are rounded to bf16 before the MFMA, so the model is
    bf16(bf16(LN(x)) (*) bf16(w) + bias).  Element bound against the fp64 conv of those rounded
    operands, e = 2 (k^2 + 2) 2^-24 sum |x^||w^|; the RMS against the unrounded conv, margin 1.10."""
    M = B * H * W
    def randn(*shape, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return torch.randn(*shape, generator=g, dtype=torch.float64).to(DEV)
    rows = ((randn(M, C, seed=40) * 2.0 + 0.5) * bb.pow2((M, 1), -6, 6, 41, DEV)).to(BF)
    w = (randn(C, k, k, seed=42) * 0.2 * bb.pow2((C, 1, 1), -3, 3, 43, DEV)).float()
    b = (randn(C, seed=44) * bb.pow2((C,), -3, 3, 43, DEV)).float()
    x64 = xh = rows.double()
    kw = {}
    if ln:
        g, be = (randn(C, seed=45) * 0.1 + 1).float(), (randn(C, seed=46) * 0.1).float()
        stats = torch.empty(M, 2, device=DEV)
        sp.rowstats(sp.dense(rows), 1e-6, stats, M, C)
        kw = dict(stats=stats, ln_gamma=g, ln_beta=be)
        x64 = (x64 - stats[:, 0:1].double()) * stats[:, 1:2].double() * g.double() + be.double()
        # the staged operand, operation for operation: fp32 subtract, multiply, one fma, then bf16
        t = (rows.float() - stats[:, 0:1]) * stats[:, 1:2]
        xh = (t.double() * g.double() + be.double()).float().to(BF).double()
    assert sp.lib().sdp_dwconv_variant(1, H, W, C, k) == 5
    y = torch.full((M, C), float("nan"), dtype=BF, device=DEV)
    sp.dwconv(sp.dense(rows), w.view(C, k * k).contiguous(), b, sp.dense(y), B, H, W, C, k, **kw)
    torch.cuda.synchronize()
    img = lambda t: t.view(B, H, W, C)  # noqa: E731
    wh = bb.rne_bf16(w.double())
    ref = (conv64(img(x64), w.double(), k) + b.double()).view(M, C)
    ref_r = (conv64(img(xh), wh, k) + b.double()).view(M, C)
    sabs = (conv64(img(xh.abs()), wh.abs(), k) + b.double().abs()).view(M, C)
    what = f"dwconv3t {(B, H, W, C, k)} {'ln' if ln else 'plain'}"
    bb.assert_elementwise(y, ref_r, 2.0 * (k * k + 2) * 2.0 ** -24 * sabs, what)
    bb.assert_rms_vs_model(y, bb.rne_bf16(ref_r), ref, bb.budget_scale(ref, sabs), 1.10, what)
