"""GPU: the bf16 fast-path kernels against a rounding budget (tests/bf16_budget.py), not 1e-2 of max.

The fast GEMM (kernels 9 and 14), the flash attention tiers, the Toeplitz-MFMA depthwise conv and
the flash training attention are otherwise only held to ``close()``: 1.2e-2 (or 2e-2) of the
reference's largest element, about five bf16 ulps of it for every element.  Here every case

* makes its inputs in bf16 and takes the reference in fp64 of those bf16 values (on the device),
* asserts which kernel ran where the library can be asked,
* scales rows by powers of two 2^-6 .. 2^6 (weight rows / value columns 2^-3 .. 2^3), so that
  small rows are judged at their own ulp,
* applies ``assert_elementwise`` with a derived fp32-arithmetic bound ``e`` and / or
  ``assert_rms_vs_model`` against the fp64 reference rounded to bf16 exactly where the kernel
  rounds (include/sdpnet_hip.h, "bf16 rounding points").

The derivation of ``e``: bf16 x bf16 products are exact in fp32; the K - 1 accumulations and each
epilogue operation are taken at 2^-23 relative each (twice the round-to-nearest unit: MFMA
accumulation is not guaranteed round-to-nearest), every term entering by its absolute value.
The RMS margins (GEMM, depthwise conv 1.10; attention 1.25) are those of the self-check
(tests/test_budget_selfcheck.py), where they separate the correct emulations from the faulty."""
import functools
import math

import pytest
import torch

import bf16_budget as bb
import sdpnet_hip as sp

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _diag_library():
    try:
        return sp.lib().sdp_build_info() != 0
    except Exception:  # library not loadable here (CPU collection without a build)
        return False


DIAG = _diag_library()
ATTN_TIERS = [2, 3, 4, 5, 6] if DIAG else [3, 4, 5]


def randn(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(DEV)


# =========================================================================== a. fast GEMM
ROWMAP = "rowmap"  # the token buffer of test_gemm_row_maps_and_inplace_residual: B 3, R 4, P 196, C 256, K 128
GEMM_SHAPES = [(128, 128, 64), (257, 264, 64), (300, 384, 768), (513, 1000, 3072), ROWMAP]
RM_B, RM_R, RM_P, RM_C, RM_K = 3, 4, 196, 256, 128
N_EPI = 4  # epilogue operations per element, at most: LN fold 3 (two fma, one mul) + residual add

# name: (bias, activation, residual)
EPILOGUES = {
    "plain": (False, "none", None),
    "bias": (True, "none", None),
    "relu": (True, "relu", None),
    "gelu_tanh": (True, "gelu_tanh", None),
    "gelu_erf": (True, "gelu_erf", None),
    "resid_post": (True, "gelu_tanh", "post"),
    "resid_pre": (True, "none", "pre"),
    "resid_pre_gelu": (True, "gelu_tanh", "pre"),
    "resid_part": (True, "none", "post"),  # + the LN partials buffer: the model's specialised epilogue
    "ln_fold": (True, "none", None),
}
ACT_CODE = {"none": 0, "relu": 2, "gelu_tanh": 1, "gelu_erf": 1}


def shape_of(shape):
    return (RM_B * RM_P, RM_C, RM_K) if shape == ROWMAP else shape


@functools.lru_cache(maxsize=None)
def gemm_data(shape):
    """Inputs and fp64 references of one shape, made once and left unchanged."""
    M, N, K = shape_of(shape)
    rs, cs = bb.pow2((M, 1), -6, 6, 11, DEV), bb.pow2((N, 1), -3, 3, 12, DEV)
    d = {}
    d["x"] = (randn(M, K, seed=13) * rs).to(BF)
    d["w"] = (randn(N, K, seed=14) * 0.05 * cs).to(BF)
    d["b"] = (randn(N, seed=15) * 0.3 * cs[:, 0]).float()
    d["r"] = (randn(M, N, seed=16) * (0.05 * math.sqrt(K)) * rs * cs[:, 0]).to(BF)
    d["z"] = (randn(M, N, seed=17) * 1.5).to(BF)  # the saved pre-activation of training mode 2
    x64, w64 = d["x"].double(), d["w"].double()
    d["acc"] = x64 @ w64.t()
    d["sabs"] = x64.abs() @ w64.abs().t()
    # LN fold: rows with a mean, fp32 master weight
    d["xl"] = ((randn(M, K, seed=18) * 1.3 + randn(M, 1, seed=19) * 2.0) * rs).to(BF)
    d["w32"] = (randn(N, K, seed=14) * 0.05 * cs).float()
    d["g"], d["be"] = (randn(K, seed=20) * 0.2 + 1).float(), (randn(K, seed=21) * 0.2).float()
    return d


def act64(name, z):
    """(act(z), evaluation-error bound of the kernel's fp32 form, Lipschitz constant)."""
    if name == "none":
        return z, torch.zeros_like(z), 1.0
    if name == "relu":
        return torch.relu(z), torch.zeros_like(z), 1.0
    if name == "gelu_tanh":
        # common.h gelu_fast: u = x (x^2 K2 + K) (two fma, one mul), exp2 and rcp at 1 ulp, one add, one
        # mul: (8 + 2 |u|) 2^-24 relative, |u| the exponent (its rounding scales with its size)
        a = bb.gelu_tanh64(z)
        u = (z * (z * z * 0.10294324471 + 2.3022081983)).abs()
        return a, (8.0 + 2.0 * u) * 2.0 ** -24 * a.abs() + 2.0 ** -60, bb.GELU_LIPSCHITZ
    # common.h norm_cdf (Abramowitz & Stegun 7.1.26): |d gelu| <= 4.2e-7 absolute, plus two roundings
    a = bb.gelu_erf64(z)
    return a, 4.2e-7 + 2.0 ** -22 * a.abs(), bb.GELU_LIPSCHITZ


def gemm_expect(kern, d, epi, K, x_key="x", ln=None, w64=None):
    """(ref64, model64, e, sum_abs_terms) of one epilogue, following csrc/gemm.hip: kernel 9
    (tile_epilogue16) rounds once; kernel 14 (tile_epilogue_rows / tile_epilogue_fl) stages
    bf16(act(acc + b)) and its drain adds the residual to that and rounds again -- for resid_pre
    as well, which it only takes without an activation (with one the call goes to kernel 9)."""
    has_b, act, resid = EPILOGUES[epi]
    c = 2.0 * (K + N_EPI) * 2.0 ** -24
    if ln is None:
        b = d["b"].double() if has_b else torch.zeros_like(d["b"]).double()
        z0 = d["acc"] + b
        terms = d["sabs"] + b.abs()
    else:
        st, colsum, cvec = ln
        mean, rstd = st[:, 0:1].double(), st[:, 1:2].double()
        x64 = d[x_key].double()
        z0 = rstd * (x64 @ w64.t()) - rstd * mean * colsum.double() + cvec.double()
        terms = rstd * (x64.abs() @ w64.abs().t() + mean.abs() * colsum.double().abs()) + cvec.double().abs()
    ez = c * terms
    R = d["r"].double()
    if resid is None:
        a, ev, L = act64(act, z0)
        return a, bb.rne_bf16(a), L * ez + ev, terms
    terms = terms + R.abs()
    double_round = kern == 14 and not (resid == "pre" and act != "none")
    if resid == "pre" and not double_round:
        a, ev, L = act64(act, z0 + R)
        return a, bb.rne_bf16(a), L * (ez + c * R.abs()) + ev, terms
    a, ev, L = act64(act, z0)
    ea = L * ez + ev
    ref = a + R
    if not double_round:
        return ref, bb.rne_bf16(ref), ea + c * (a.abs() + R.abs()), terms
    staged = bb.rne_bf16(a)
    e = ea + 0.5 * bb.ulp_bf16(a.abs() + ea) + c * (a.abs() + R.abs())
    return ref, bb.rne_bf16(staged + R), e, terms


@pytest.mark.parametrize("epi", list(EPILOGUES))
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=str)
@pytest.mark.parametrize("kern", [9, 14])
def test_fast_gemm_budget(kern, shape, epi):
    M, N, K = shape_of(shape)
    d = gemm_data(shape)
    has_b, act, resid = EPILOGUES[epi]
    assert sp.gemm_variant(BF, M, N, K) == 1
    L = sp.lib()
    x, w, bias, ln, lnx = d["x"], d["w"], d["b"] if has_b else None, None, None
    if epi == "ln_fold":
        x = d["xl"]
        part = torch.empty(M, (K + 63) // 64, 2, device=DEV)
        sp.row_partials(sp.dense(x), M, K, part)
        st = torch.empty(M, 2, device=DEV)
        sp.ln_stats(part, sp.dense(x), M, K, 1e-5, st)
        w, colsum, bias = sp.fold_ln_weight(d["w32"], d["g"], d["be"], d["b"], BF)
        ln, lnx = (st, colsum), (st, colsum, bias)
    # output (and in-place residual) rows: dense, or the image rows of a [B, R + P, C] token buffer
    if shape == ROWMAP:
        Nt = RM_R + RM_P
        tok = (randn(RM_B * Nt, N, seed=22)).to(BF)
        tok.view(RM_B, Nt, N)[:, RM_R:] = d["r"].view(RM_B, RM_P, N)
        tok0 = tok.clone()
        out = sp.Rows(tok, N, RM_P, Nt, RM_R)
        res = out if resid else None
        prow = RM_B * Nt
    else:
        y = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
        out = sp.dense(y)
        res = sp.dense(d["r"]) if resid else None
        prow = M
    pbuf = torch.empty(prow, (N + 63) // 64, 2, device=DEV) if epi == "resid_part" else None
    old = L.sdp_gemm_set_fast_kernel(kern)
    oldg = L.sdp_gemm_set_exact_gelu(1 if act == "gelu_erf" else 0)
    try:
        sp.gemm(sp.dense(x), w, out, M, N, K, bias=bias, resid=res, act=ACT_CODE[act],
                resid_pre=resid == "pre", ln=ln, part=pbuf)
        torch.cuda.synchronize()
    finally:
        L.sdp_gemm_set_exact_gelu(oldg)
        L.sdp_gemm_set_fast_kernel(old)
    if shape == ROWMAP:
        got = tok.view(RM_B, Nt, N)[:, RM_R:].reshape(M, N)
        assert torch.equal(tok.view(RM_B, Nt, N)[:, :RM_R], tok0.view(RM_B, Nt, N)[:, :RM_R])  # register rows
    else:
        got = y
    ref, model, e, terms = gemm_expect(kern, d, epi, K, "xl", lnx, w.double() if ln else None)
    what = f"gemm k{kern} {shape} {epi}"
    bb.assert_elementwise(got, ref, e, what)
    bb.assert_rms_vs_model(got, model, ref, bb.budget_scale(ref, terms), 1.10, what)


@pytest.mark.parametrize("shape", GEMM_SHAPES[:-1], ids=str)
def test_fast_gemm_training_epilogues_budget(shape):
    """sdp_gemm_train_epi (dense rows; whole-line epilogue).  Mode 1: Y = bf16(acc + b) and Y2 =
    bf16(gelu(Y)) of the *stored* Y (erf form, sdp_act_fwd's arithmetic).  Mode 2: Y =
    bf16(bf16(acc) * gelu'(Z)) -- the staged bf16 dh times act'(Z), sdp_act_bwd's arithmetic."""
    M, N, K = shape
    d = gemm_data(shape)
    c = 2.0 * (K + N_EPI) * 2.0 ** -24
    b = d["b"].double()
    y, y2 = (torch.full((M, N), float("nan"), dtype=BF, device=DEV) for _ in range(2))
    assert sp.gemm_train_epi(1, d["x"], d["w"], y, M, N, K, bias=d["b"], y2=y2, act=1)
    z0, terms = d["acc"] + b, d["sabs"] + b.abs()
    ez = c * terms
    D = bb.budget_scale(z0, terms)
    bb.assert_elementwise(y, z0, ez, f"train mode 1 Y {shape}")
    bb.assert_rms_vs_model(y, bb.rne_bf16(z0), z0, D, 1.10, f"gemm train mode 1 Y {shape}")
    a, ev, Lg = act64("gelu_erf", z0)
    e2 = Lg * (ez + 0.5 * bb.ulp_bf16(z0.abs() + ez)) + ev
    model2 = bb.rne_bf16(bb.gelu_erf64(bb.rne_bf16(z0)))
    bb.assert_elementwise(y2, a, e2, f"train mode 1 Y2 {shape}")
    bb.assert_rms_vs_model(y2, model2, a, bb.budget_scale(a, Lg * terms), 1.10, f"gemm train mode 1 Y2 {shape}")
    # mode 2
    dz = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
    assert sp.gemm_train_epi(2, d["x"], d["w"], dz, M, N, K, z=d["z"], act=1)
    gp = bb.gelu_erf_grad64(d["z"].double())
    acc, ea = d["acc"], c * d["sabs"]
    ref = acc * gp
    model = bb.rne_bf16(bb.rne_bf16(acc) * gp)
    # |d gelu'| <= 3.0e-7 absolute (common.h), one rounding of gelu' and one of the product
    e = gp.abs() * (ea + 0.5 * bb.ulp_bf16(acc.abs() + ea)) + (acc.abs() + ea) * (3.0e-7 + 2.0 ** -22 * gp.abs())
    bb.assert_elementwise(dz, ref, e, f"train mode 2 {shape}")
    bb.assert_rms_vs_model(dz, model, ref, bb.budget_scale(ref, d["sabs"] * gp.abs()), 1.10,
                           f"gemm train mode 2 {shape}")


# =========================================================================== e. fold_ln_weight
@pytest.mark.parametrize("N,K", [(128, 64), (1000, 768)])
def test_fold_ln_weight_budget(N, K):
    """colsum[n] is the sum of the *rounded* Wf row (the fold's subtraction only cancels against what
    the MFMA actually sums), cvec = beta . W^T + bias; both fp32 sums of K terms: K 2^-24 sum |t|."""
    w = (randn(N, K, seed=30) * 0.05 * bb.pow2((N, 1), -3, 3, 31, DEV)).float()
    g, be, b = (randn(K, seed=32) * 0.2 + 1).float(), (randn(K, seed=33) * 0.2).float(), randn(N, seed=34).float()
    wf, colsum, cvec = sp.fold_ln_weight(w, g, be, b, BF)
    assert torch.equal(wf, (w * g).to(BF))  # one fp32 product, one rounding
    wf64 = wf.double()
    err = (colsum.double() - wf64.sum(1)).abs()
    bound = K * 2.0 ** -24 * wf64.abs().sum(1)
    assert bool((err <= bound).all()), f"colsum: worst {float((err / bound).max()):.3f} of the bound"
    t = be.double() * w.double()
    err = (cvec.double() - (t.sum(1) + b.double())).abs()
    bound = K * 2.0 ** -24 * (t.abs().sum(1) + b.double().abs())
    assert bool((err <= bound).all()), f"cvec: worst {float((err / bound).max()):.3f} of the bound"
    print(f"BUDGET fold_ln_weight {N}x{K}: colsum / cvec within K 2^-24 sum|t|")


# =========================================================================== b. eval attention
# shape -> (tier to select, variant that selection must give there)
ATTN_HOME = {
    (2, 200, 2, 96): (4, 4), (1, 33, 2, 32): (4, 4), (1, 256, 2, 64): (4, 4), (2, 1, 2, 32): (4, 4),  # attn_fa4
    (1, 257, 2, 96): (3, 3), (1, 288, 2, 64): (3, 3), (1, 289, 2, 32): (3, 3),  # whole head; 9 key tiles
    (1, 300, 2, 128): (5, 5),  # streaming
}


@functools.lru_cache(maxsize=None)
def attn_data(B, N, H, hd, norm):
    C = H * hd
    s = 1000 * N + hd + (7 if norm else 0)
    q, k, v = (randn(B * N, C, seed=s + i) for i in range(3))
    v = v * bb.pow2((C,), -3, 3, s + 3, DEV)
    if norm:
        q, k = q * 2.0 + 0.3, k * 2.0 - 0.2
        gq, gk = ((2.0 + 0.1 * randn(hd, seed=s + 4 + i)).float() for i in range(2))
        bq, bk = ((0.1 * randn(hd, seed=s + 6 + i)).float() for i in range(2))
        nrm = (gq, bq, gk, bk)
    else:
        q, nrm = q * 4.0, None  # scores of std ~ 4: a scale or exponent error shows
    qkv = torch.cat([q, k, v], 1).to(BF).contiguous()
    q64, k64, v64 = qkv.double().view(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    scale = 1.0 / math.sqrt(hd)
    ref, model, sabs, _, qn, kn = bb.attention_ref_model(q64, k64, v64, scale, nrm, 1e-5)
    e = None
    if not norm:
        e = bb.attention_element_bound(qn, kn, sabs, scale)
    unperm = lambda t: None if t is None else t.permute(0, 2, 1, 3).reshape(B * N, C)  # noqa: E731
    return qkv, nrm, unperm(ref), unperm(model), unperm(sabs), unperm(e)


def attention_budget(B, N, H, hd, norm, kern, want, what):
    qkv, nrm, ref, model, sabs, e = attn_data(B, N, H, hd, norm)
    o = torch.full((B * N, H * hd), float("nan"), dtype=BF, device=DEV)
    old = sp.lib().sdp_attention_set_kernel(kern) if kern else None
    try:
        v = sp.attention_variant(BF, N, H, hd)
        assert v >= 2, f"{what}: no MFMA attention kernel (variant {v})"
        assert want is None or v == want, f"{what}: variant {v}, expected {want}"
        sp.attention(qkv.clone(), o, B, N, H, hd, qk_norm=nrm, eps=1e-5)
        torch.cuda.synchronize()
    finally:
        if kern:
            sp.lib().sdp_attention_set_kernel(old)
    what = f"{what} variant {v}"
    if e is not None:
        bb.assert_elementwise(o, ref, e, what)
    bb.assert_rms_vs_model(o, model, ref, bb.budget_scale(ref, sabs), 1.25, what)


@pytest.mark.parametrize("norm", [False, True], ids=["nonorm", "qknorm"])
@pytest.mark.parametrize("B,N,H,hd", list(ATTN_HOME))
@pytest.mark.parametrize("kern", ATTN_TIERS)
def test_attention_budget(kern, B, N, H, hd, norm):
    """Every shape under every tier the library offers; under the tier a shape is listed for, the
    kernel that must take it is asserted.  No element bound with the q/k norm on: through the
    rounding of the normalised q and k the worst case is looser than close()'s tolerance."""
    home, variant = ATTN_HOME[(B, N, H, hd)]
    attention_budget(B, N, H, hd, norm, kern, variant if kern == home else None,
                     f"attention tier {kern} {(B, N, H, hd)} {'qknorm' if norm else 'nonorm'}")


@pytest.mark.parametrize("norm", [False, True], ids=["nonorm", "qknorm"])
def test_attention_persistent_cycling_budget(norm):
    """B * H > 3 x 256: every persistent workgroup cycles through its three K / V images (as
    test_attention_xl_persistent), under the default selection."""
    B, N, H, hd = 100, 260, 8, 96
    try:
        attention_budget(B, N, H, hd, norm, 0, 3,
                         f"attention persistent {(B, N, H, hd)} {'qknorm' if norm else 'nonorm'}")
    finally:
        attn_data.cache_clear()  # the one large reference: not kept


# =========================================================================== c. depthwise conv tier 3
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


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("B,H,W,C,k", [(2, 16, 16, 32, 7), (1, 14, 14, 64, 7), (3, 7, 7, 32, 3), (2, 5, 16, 96, 5)])
def test_dwconv_mfma_budget(B, H, W, C, k, ln):
    """dwconv3_mfma (tier 3).  The library has no query for the depthwise tier taken, so every
    shape here lies strictly inside the documented tier-3 domain -- bf16, C % 32 == 0, H, W <= 16,
    k in {3, 5, 7}, dense 16-B aligned rows -- under the default selection (3).
    csrc/norm_dw.hip rounds the fp32 *weights* and the LayerNorm'd input to bf16 before the MFMA:
    the model is bf16(bf16(LN(x)) (*) bf16(w) + bias).  The element bound is taken against the fp64
    conv of those rounded operands (e = 2 (k^2 + 2) 2^-24 sum |x^||w^|: k^2 products, bias, and the
    MFMA's zero-padded 32-wide sums add no non-zero term); the RMS against the unrounded conv."""
    M = B * H * W
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
        # the staged operand, operation for operation (norm_dw.hip `put`): fp32 subtract, multiply,
        # one fma, then bf16 -- rounding the fp64 LN instead flips an occasional element by one bf16
        # ulp of the *input*, which no fp32-arithmetic bound on the output covers
        t = (rows.float() - stats[:, 0:1]) * stats[:, 1:2]
        xh = (t.double() * g.double() + be.double()).float().to(BF).double()
    assert sp.lib().sdp_dwconv_set_kernel(0) == 3
    y = torch.full((M, C), float("nan"), dtype=BF, device=DEV)
    sp.dwconv(sp.dense(rows), w.view(C, k * k).contiguous(), b, sp.dense(y), B, H, W, C, k, **kw)
    torch.cuda.synchronize()
    img = lambda t: t.view(B, H, W, C)  # noqa: E731
    wh = bb.rne_bf16(w.double())
    ref = (conv64(img(x64), w.double(), k) + b.double()).view(M, C)
    ref_r = (conv64(img(xh), wh, k) + b.double()).view(M, C)
    sabs = (conv64(img(xh.abs()), wh.abs(), k) + b.double().abs()).view(M, C)
    what = f"dwconv3 {(B, H, W, C, k)} {'ln' if ln else 'plain'}"
    bb.assert_elementwise(y, ref_r, 2.0 * (k * k + 2) * 2.0 ** -24 * sabs, what)
    bb.assert_rms_vs_model(y, bb.rne_bf16(ref_r), ref, bb.budget_scale(ref, sabs), 1.10, what)


# =========================================================================== d. flash training attention
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("B,N,H,hd", [(2, 53, 2, 16), (1, 64, 2, 96), (1, 77, 2, 64), (1, 260, 2, 96), (1, 33, 1, 128)])
def test_flash_train_attention_budget(B, N, H, hd, p):
    """sdp_attn_train_fwd / bwd with the kernels' own dropout mask.  Rounding points of
    csrc/attn_train.hip (all to bf16, fp32 everything else):
      :198  forward dropout(P) = p keep / (1 - p), p = exp2(s - running max) un-normalised, for P V
            (:188 the row sum takes the unrounded, undropped p);
      :218  O = acc / l, stored; :458 D = rowsum(dO o O) reads that *stored* O;
      :367  backward dropout(P), P = exp2(s - lse) normalised, for dV;
      :368 / :499  dS = P o (dP keep - D), for dK / dQ;
      :393 / :394 / :518  the outputs dK = scale acc, dV, dQ = scale acc.
    O, dV, dQ and dK are each judged in units of their own budget D (t_j = Pd_ij v_j; Pd_ij dO_i;
    scale dS_ij k_j; scale dS_ij q_i) against that model, margin 1.25; LSE (fp32) to 1e-5 relative."""
    assert sp.attn_train_applies(BF, N, hd)
    C, T = H * hd, B * N
    qkv = randn(T, 3 * C, seed=50 + N) * 1.5
    qkv[:, 2 * C:] *= bb.pow2((C,), -3, 3, 51, DEV)
    qkv = qkv.to(BF)
    do = (randn(T, C, seed=52 + N) * bb.pow2((C,), -3, 3, 53, DEV)).to(BF)
    seed, scale = 7654321 + N, 1.0 / math.sqrt(hd)
    o = torch.full((T, C), float("nan"), dtype=BF, device=DEV)
    lse = torch.empty(B * H * N, dtype=torch.float32, device=DEV)
    sp.attn_train_fwd(qkv, o, lse, B, N, H, hd, scale, p, seed)
    dqkv = torch.full((T, 3 * C), float("nan"), dtype=BF, device=DEV)
    delta = torch.empty(B * H * N, dtype=torch.float32, device=DEV)
    sp.attn_train_bwd(qkv, o, do, lse, delta, (dqkv, 0), (dqkv, C), (dqkv, 2 * C), B, N, H, hd, scale, p, seed)
    torch.cuda.synchronize()
    keep = sp.attn_dropout_mask(B * H, N, p, seed, DEV).view(B, H, N, N).double() / (1.0 - p)
    q, k, v = qkv.double().view(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    g = do.double().view(B, N, H, hd).permute(0, 2, 1, 3)
    tr = lambda t: t.transpose(-1, -2)  # noqa: E731
    # exact
    s = q @ tr(k) * scale
    P = torch.softmax(s, -1)
    Pd = P * keep
    O = Pd @ v
    dP = (g @ tr(v)) * keep
    dS = P * (dP - (g * O).sum(-1, keepdim=True))
    ref = {"O": O, "dV": tr(Pd) @ g, "dQ": scale * (dS @ k), "dK": scale * (tr(dS) @ q)}
    terms = {"O": Pd @ v.abs(), "dV": tr(Pd) @ g.abs(), "dQ": scale * (dS.abs() @ k.abs()),
             "dK": scale * (tr(dS.abs()) @ q.abs())}
    # model
    pu = torch.exp(s - s.amax(-1, keepdim=True))
    Om = bb.rne_bf16((bb.rne_bf16(pu * keep) @ v) / pu.sum(-1, keepdim=True))
    Pdb = bb.rne_bf16(Pd)
    dSm = bb.rne_bf16(P * (dP - (g * Om).sum(-1, keepdim=True)))
    model = {"O": Om, "dV": bb.rne_bf16(tr(Pdb) @ g), "dQ": bb.rne_bf16(scale * (dSm @ k)),
             "dK": bb.rne_bf16(scale * (tr(dSm) @ q))}
    gq, gk, gv = dqkv.double().view(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    got = {"O": o.double().view(B, N, H, hd).permute(0, 2, 1, 3), "dV": gv, "dQ": gq, "dK": gk}
    ref_lse = torch.logsumexp(s, -1) / math.log(2.0)
    lerr = (lse.double().view(B, H, N) - ref_lse).abs() / ref_lse.abs().clamp_min(1.0)
    print(f"BUDGET train attention {(B, N, H, hd)} p={p}: lse worst relative error {float(lerr.max()):.3e}")
    fails = []
    for name in ("O", "dV", "dQ", "dK"):
        try:
            bb.assert_rms_vs_model(got[name], model[name], ref[name], bb.budget_scale(ref[name], terms[name]), 1.25,
                                   f"train attention {(B, N, H, hd)} p={p} {name}")
        except AssertionError as ex:
            fails.append(str(ex))
    assert not fails, "; ".join(fails)
    assert float(lerr.max()) <= 1e-5, f"lse: {float(lerr.max()):.3e} relative"
