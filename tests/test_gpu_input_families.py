"""GPU: the kernels on the input families of tests/input_families.py -- rows with an offset far above
their spread, constant rows with one element one ulp higher, flat rows, an outlier channel, tiny and
huge spreads, three values of eps; logit rows with a common offset, a dominant class, equal classes,
a wide spread and -inf classes; every bf16 value through the activations.

Every LayerNorm entry point is held, element by element, to ``input_families.ln_bound`` (derived
there; bf16 outputs through ``bf16_budget.assert_elementwise``), its statistics to
``assert_stats``.  The fused q/k head LayerNorm of the eval attention kernels is judged as
test_gpu_bf16_budget.py judges attention: ``assert_rms_vs_model`` against ``attention_ref_model``,
margin 1.25.  Losses and softmax are compared with fp64 torch on the stored logits; gradients per
element with torch's own fp32 error as the yardstick.  Activations are compared with fp64 on all
65,536 bf16 bit patterns within the bound stated per function in ``act_bound``.

Every ``FAMILY`` / ``BUDGET`` / ``RATIO`` line printed (pytest -s) is a measured figure;
profiles/input_families.md records them."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import bf16_budget as bb
import input_families as fam
import sdpnet_hip as sp
from test_gpu_bf16_budget import ATTN_HOME, conv64

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32
DTYPES = [F32, BF]
DT_IDS = ["fp32", "bf16"]
M_ROWS = 64
LN_CS = [96, 768, 1032]  # ln_fwd_sm / one 8-wide pass per lane / three passes and C % 64 != 0


@pytest.fixture(autouse=True)
def _full_precision_references():
    old = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("highest")
    yield
    torch.set_float32_matmul_precision(old)


def randn(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(DEV)


@functools.lru_cache(maxsize=None)
def ln_case(C, dtype, M=M_ROWS):
    """(x [M, C] in dtype, family names, gamma, beta): made once, left unchanged."""
    x, names = fam.family_rows(M, C, dtype, seed=200 + C)
    gamma = (1.0 + 0.2 * randn(C, seed=201 + C)).float()
    beta = (0.2 * randn(C, seed=202 + C)).float()
    return x.to(DEV), names, gamma, beta


def judge_ln(y, x, gamma, beta, eps, names, what):
    ref, _, _ = fam.ln_ref64(x, gamma, beta, eps)
    return fam.assert_families(y, ref, fam.ln_bound(x, gamma, beta, eps), names, y.dtype == BF, what)


ln_params = pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
c_params = pytest.mark.parametrize("C", LN_CS)
eps_params = pytest.mark.parametrize("eps", fam.EPS_VALUES)


# =========================================================================== LayerNorm, forward
@eps_params
@c_params
@ln_params
def test_layernorm_families(dtype, C, eps):
    """sdp_layernorm on dense rows, and on the image rows of a [B, R + P, C] token buffer."""
    x, names, g, b = ln_case(C, dtype)
    y = torch.full_like(x, float("nan"))
    sp.layernorm(sp.dense(x), g, b, eps, sp.dense(y), M_ROWS, C)
    judge_ln(y, x, g, b, eps, names, f"layernorm {DT_IDS[dtype == BF]} C={C} eps={eps}")
    B, R, P = 2, 3, M_ROWS // 2
    tok = torch.full((B, R + P, C), float("nan"), dtype=dtype, device=DEV)
    tok[:, R:] = x.view(B, P, C)
    y2 = torch.full_like(x, float("nan"))
    sp.layernorm(sp.Rows(tok.view(-1, C), C, P, R + P, R), g, b, eps, sp.dense(y2), M_ROWS, C)
    assert torch.equal(y2, y), "row-mapped rows differ from the dense ones"


@eps_params
@c_params
@ln_params
def test_rowstats_ln_apply_families(dtype, C, eps):
    x, names, g, b = ln_case(C, dtype)
    st = torch.full((M_ROWS, 2), float("nan"), device=DEV)
    sp.rowstats(sp.dense(x), eps, st, M_ROWS, C)
    what = f"rowstats {DT_IDS[dtype == BF]} C={C} eps={eps}"
    fam.assert_stats(st[:, 0], st[:, 1], x, eps, names, what)
    y = torch.full_like(x, float("nan"))
    sp.ln_apply(sp.dense(x), st, g, b, sp.dense(y), M_ROWS, C)
    judge_ln(y, x, g, b, eps, names, "ln_apply after " + what)


@eps_params
@c_params
@ln_params
def test_row_partials_ln_stats_families(dtype, C, eps):
    """The statistics by 64-column parts (Chan-merged), as the GEMM's LN fold takes them."""
    x, names, _, _ = ln_case(C, dtype)
    part = torch.full((M_ROWS, (C + 63) // 64, 2), float("nan"), device=DEV)
    sp.row_partials(sp.dense(x), M_ROWS, C, part)
    st = torch.full((M_ROWS, 2), float("nan"), device=DEV)
    sp.ln_stats(part, sp.dense(x), M_ROWS, C, eps, st)
    fam.assert_stats(st[:, 0], st[:, 1], x, eps, names, f"row_partials + ln_stats {DT_IDS[dtype == BF]} C={C} eps={eps}")


@eps_params
@c_params
@pytest.mark.parametrize("xdt,ydt", [(F32, F32), (BF, BF), (F32, BF)], ids=["fp32", "bf16", "mixed"])
def test_ln_fwd_families(xdt, ydt, C, eps):
    """sdp_ln_fwd and sdp_ln_fwd_mixed (fp32 rows, bf16 output): output and statistics."""
    x, names, g, b = ln_case(C, xdt)
    st = torch.full((M_ROWS, 2), float("nan"), device=DEV)
    y = torch.full((M_ROWS, C), float("nan"), dtype=ydt, device=DEV)
    sp.ln_fwd(sp.dense(x), eps, g, b, st, sp.dense(y), M_ROWS, C)
    what = f"ln_fwd {xdt}->{ydt} C={C} eps={eps}"
    fam.assert_stats(st[:, 0], st[:, 1], x, eps, names, what)
    judge_ln(y, x, g, b, eps, names, what)


@eps_params
@pytest.mark.parametrize("C", [768, 1032])  # (C <= 128 is refused: the caller runs the two passes)
@pytest.mark.parametrize("xdt,ydt,adt", [(F32, F32, F32), (BF, BF, BF), (BF, F32, BF)], ids=["fp32", "bf16", "mixed"])
def test_add_ln_fwd_families(xdt, ydt, adt, C, eps):
    """The families are on the sum: x and the residual are each half a family row (exact), so the
    stored y is the row and a = LN(y) is judged on it."""
    rows, names, g, b = ln_case(C, BF if BF in (xdt, ydt) else F32)
    half = rows.double() * 0.5
    x, r = half.to(xdt), half.to(ydt)
    y = torch.full((M_ROWS, C), float("nan"), dtype=ydt, device=DEV)
    a = torch.full((M_ROWS, C), float("nan"), dtype=adt, device=DEV)
    st = torch.full((M_ROWS, 2), float("nan"), device=DEV)
    assert sp.add_ln_fwd(sp.dense(x), sp.dense(y), sp.dense(a), M_ROWS, C, sp.dense(r), eps, g, b, st)
    assert torch.equal(y.double(), rows.double())
    what = f"add_ln_fwd {xdt}/{ydt}/{adt} C={C} eps={eps}"
    fam.assert_stats(st[:, 0], st[:, 1], y, eps, names, what)
    judge_ln(a, y, g, b, eps, names, what)
    assert not sp.add_ln_fwd(sp.dense(x[:, :96].contiguous()), sp.dense(y[:, :96].contiguous()),
                             sp.dense(a[:, :96].contiguous()), M_ROWS, 96, sp.dense(r[:, :96].contiguous()), eps,
                             g[:96].clone(), b[:96].clone(), st)


HEADS = [(2, 96), (4, 16), (2, 128)]


@functools.lru_cache(maxsize=None)
def head_case(H, hd, dtype, T=48):
    """qkv [T, 3 H hd]: the q and k heads are family rows of length hd, v is randn."""
    q, qn = fam.family_rows(T * H, hd, dtype, seed=300 + hd)
    k, kn = fam.family_rows(T * H, hd, dtype, seed=301 + hd)
    v = randn(T, H * hd, seed=302 + hd).to(dtype)
    qkv = torch.cat([q.view(T, H * hd).to(DEV), k.view(T, H * hd).to(DEV), v], 1).contiguous()
    gs = [(1.0 + 0.2 * randn(hd, seed=303 + hd + i)).float() for i in range(2)]
    bs = [(0.2 * randn(hd, seed=305 + hd + i)).float() for i in range(2)]
    return qkv, qn, kn, (gs[0], bs[0], gs[1], bs[1])


@eps_params
@pytest.mark.parametrize("H,hd", HEADS)
@ln_params
def test_qk_headnorm_families(dtype, H, hd, eps):
    """sdp_qk_headnorm (eval, in place) and the training head LayerNorm (sdp_ln_fwd over the head
    rows of the qkv buffer, as sdpnet_train.py addresses them)."""
    T, C = 48, H * hd
    qkv, qn, kn, (gq, bq, gk, bk) = head_case(H, hd, dtype)
    x = qkv.clone()
    sp.qk_headnorm(x, T, H, hd, gq, bq, gk, bk, eps)
    assert torch.equal(x[:, 2 * C:], qkv[:, 2 * C:])
    out = torch.full_like(qkv, float("nan"))
    sts = []
    for off, g, b in ((0, gq, bq), (H, gk, bk)):
        st = torch.full((T * H, 2), float("nan"), device=DEV)
        sp.ln_fwd(sp.Rows(qkv, hd, H, 3 * H, off), eps, g, b, st, sp.Rows(out, hd, H, 3 * H, off), T * H, hd)
        sts.append(st)
    for i, (names, g, b) in enumerate(((qn, gq, bq), (kn, gk, bk))):
        rows = qkv[:, i * C:(i + 1) * C].reshape(T * H, hd)
        what = f"{DT_IDS[dtype == BF]} {'qk'[i]} H={H} hd={hd} eps={eps}"
        judge_ln(x[:, i * C:(i + 1) * C].reshape(T * H, hd), rows, g, b, eps, names, "qk_headnorm " + what)
        judge_ln(out[:, i * C:(i + 1) * C].reshape(T * H, hd), rows, g, b, eps, names, "train head ln " + what)
        fam.assert_stats(sts[i][:, 0], sts[i][:, 1], rows, eps, names, "train head ln " + what)


@eps_params
@pytest.mark.parametrize("kern", [1, 2, 3])
@ln_params
def test_dwconv_ln_families(dtype, kern, eps):
    """sdp_dwconv with the LayerNorm folded in, (B, H, W, C, k) = (1, 8, 8, 96, 7): 64 family rows
    as pixels.  The bound of the LayerNorm'd pixel goes through the conv by the weights' absolute
    values; the conv itself adds 2 (k^2 + 2) 2^-24 sum |x^||w| (test_dwconv_mfma_budget).  In bf16
    tiers 1 and 3 stage the LayerNorm'd pixel in LDS as bf16 (include/sdpnet_hip.h, "bf16 rounding
    points"): there the pixel's bound grows by that rounding, ulp_bf16(|x^| + e) / 2; tier 3 also
    rounds the weights to bf16 before its MFMA, so its reference takes the rounded weights.  Tier 2
    keeps the pixel in fp32 registers."""
    B, H, W, C, k = 1, 8, 8, 96, 7
    x, names, g, be = ln_case(C, dtype)
    w = (randn(C, k, k, seed=400) * 0.2).float()
    b = randn(C, seed=401).float()
    st = torch.empty(M_ROWS, 2, device=DEV)
    sp.rowstats(sp.dense(x), eps, st, M_ROWS, C)
    y = torch.full_like(x, float("nan"))
    old = sp.lib().sdp_dwconv_set_kernel(kern)
    try:
        sp.dwconv(sp.dense(x), w.view(C, k * k).contiguous(), b, sp.dense(y), B, H, W, C, k, stats=st, ln_gamma=g,
                  ln_beta=be)
        torch.cuda.synchronize()
    finally:
        sp.lib().sdp_dwconv_set_kernel(old)
    xn, _, _ = fam.ln_ref64(x, g, be, eps)
    e_in = fam.ln_bound(x, g, be, eps)
    w64 = w.double()
    if dtype == BF and kern in (1, 3):
        e_in = e_in + 0.5 * bb.ulp_bf16(xn.abs() + e_in)
    if dtype == BF and kern == 3:
        w64 = bb.rne_bf16(w64)
    img = lambda t: t.view(B, H, W, C)  # noqa: E731
    ref = (conv64(img(xn), w64, k) + b.double()).view(M_ROWS, C)
    sabs = (conv64(img(xn.abs() + e_in), w64.abs(), k) + b.double().abs()).view(M_ROWS, C)
    e = conv64(img(e_in), w64.abs(), k).view(M_ROWS, C) + 2.0 * (k * k + 2) * 2.0 ** -24 * sabs
    # an output pixel mixes the families of its 7 x 7 neighbours: one figure for the tensor
    fam.assert_families(y, ref, e, ["mixed"] * M_ROWS, dtype == BF, f"dwconv ln tier {kern} {DT_IDS[dtype == BF]} eps={eps}")


# =========================================================================== LN-folded GEMM
# (K = 96 is no multiple of the fast kernels' 64-wide K tile: that shape runs the generic bf16 GEMM,
# whose LN fold is the same arithmetic; the selection is asserted either way)
@pytest.mark.parametrize("M,N,K,variant", [(128, 128, 96, 0), (300, 256, 768, 1)])
@pytest.mark.parametrize("kern", [9, 14])
def test_gemm_ln_fold_families(kern, M, N, K, variant):
    """sdp_fold_ln_weight + sdp_gemm_ln on family rows against the fp64 LN(x) . W^T + b, judged as
    test_fast_gemm_budget judges its ln_fold case (budget D = ulp / 2 + 2^-9 sum |t|, t the fold's
    own terms rstd x W', rstd mean colsum, cvec; margin 1.10), family by family.  The model is the
    fp64 fold with the weight rounded where the kernel rounds it (W' = bf16(W gamma)), rounded to
    bf16 once."""
    x, names = fam.family_rows(M, K, BF, seed=500 + K)
    x = x.to(DEV)
    w32 = (randn(N, K, seed=501) * 0.05).float()
    g, be, b = (1.0 + 0.2 * randn(K, seed=502)).float(), (0.2 * randn(K, seed=503)).float(), randn(N, seed=504).float()
    eps = 1e-5
    assert sp.gemm_variant(BF, M, N, K) == variant
    part = torch.empty(M, (K + 63) // 64, 2, device=DEV)
    sp.row_partials(sp.dense(x), M, K, part)
    st = torch.empty(M, 2, device=DEV)
    sp.ln_stats(part, sp.dense(x), M, K, eps, st)
    wf, colsum, cvec = sp.fold_ln_weight(w32, g, be, b, BF)
    y = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
    L = sp.lib()
    old = L.sdp_gemm_set_fast_kernel(kern)
    try:
        sp.gemm(sp.dense(x), wf, sp.dense(y), M, N, K, bias=cvec, ln=(st, colsum))
        torch.cuda.synchronize()
    finally:
        L.sdp_gemm_set_fast_kernel(old)
    x64 = x.double()
    xn, mean, rstd = fam.ln_ref64(x64, g, be, eps)
    ref = xn @ w32.double().t() + b.double()
    wf64 = wf.double()
    cs, cv = wf64.sum(1), be.double() @ w32.double().t() + b.double()
    model = bb.rne_bf16(rstd * ((x64 - mean) @ wf64.t()) + cv)
    terms = rstd * (x64.abs() @ wf64.abs().t() + mean.abs() * cs.abs()) + cv.abs()
    D = bb.budget_scale(ref, terms)
    fails = []
    for f, m in fam.family_masks(names, DEV).items():
        try:
            bb.assert_rms_vs_model(y[m], model[m], ref[m], D[m], 1.10, f"gemm_ln k{kern} {(M, N, K)} {f}")
        except AssertionError as ex:
            fails.append(str(ex))
    assert not fails, "; ".join(fails)


# =========================================================================== LayerNorm, backward
BWD_FAMILIES = ["offset32", "outlier", "tiny"]


def _stored(t, dtype):
    return t.to(dtype).double()


# ln_bwd_sm (C <= 128) / ln_bwd_k (C % 8 != 0) / ln_bwd_v8 with one and with three 8-wide passes; the
# mixed form exists for 16-byte rows only, the fused one for C > 128 as well
BWD_CASES = ([(s, C) for s in ("fp32", "bf16") for C in (96, 100, 768, 1032)]
             + [("mixed", C) for C in (96, 768, 1032)] + [("fused", C) for C in (768, 1032)])


@pytest.mark.parametrize("style,C", BWD_CASES)
def test_ln_bwd_families(style, C):
    """sdp_ln_bwd (fp32, bf16), sdp_ln_bwd_mixed (fp32 rows, bf16 dy) and sdp_ln_bwd_fused (bf16,
    with the branch-gradient output) on offset(32), outlier and tiny rows against fp64 autograd of
    the stored values.  grad_judge's rule, per tensor (dx, dgamma, dbeta): max error <= 4 x the max
    error of torch's fp32 autograd on the same rows, that result stored as the kernel stores its own
    (dx in the rows' dtype, the affine gradients in fp32)."""
    M, eps = 48, 1e-5
    xdt = F32 if style in ("fp32", "mixed") else BF
    dydt = F32 if style == "fp32" else BF
    x, names = fam.family_rows(M, C, xdt, seed=600 + C, families=BWD_FAMILIES)
    x = x.to(DEV)
    g = (1.0 + 0.2 * randn(C, seed=601)).float()
    b = (0.2 * randn(C, seed=602)).float()
    dy = randn(M, C, seed=603).to(dydt)
    st = torch.empty(M, 2, device=DEV)
    sp.rowstats(sp.dense(x), eps, st, M, C)
    dx = torch.full_like(x, float("nan"))
    emit = dict(out=torch.full((M, C), float("nan"), dtype=BF, device=DEV)) if style == "fused" else None
    dg, db = sp.ln_bwd(sp.dense(x), st, g, sp.dense(dy), sp.dense(dx), M, C, emit=emit)
    torch.cuda.synchronize()
    if emit is not None:
        assert torch.equal(emit["out"], dx)  # scale 1, no activation: the branch gradient is dx

    def grads(dt):
        xr = x.to(dt).clone().requires_grad_(True)
        gr, br = g.to(dt).clone().requires_grad_(True), b.to(dt).clone().requires_grad_(True)
        return torch.autograd.grad(F.layer_norm(xr, (C,), gr, br, eps), (xr, gr, br), dy.to(dt))

    ref = grads(torch.float64)
    t32 = grads(F32)
    fails = []
    for name, got, r, t, store in (("dx", dx, ref[0], t32[0], xdt), ("dgamma", dg, ref[1], t32[1], F32),
                                   ("dbeta", db, ref[2], t32[2], F32)):
        err = float((got.double() - r).abs().max())
        base = float((_stored(t, store) - r).abs().max())
        ratio = err / base if base > 0 else (0.0 if err == 0 else math.inf)
        print(f"RATIO ln_bwd {style} C={C} {name}: error {err:.3e}, torch fp32 {base:.3e}, ratio {ratio:.3f} (allowed 4)")
        if not ratio <= 4.0:
            fails.append(f"{name}: {ratio:.3f}")
    assert not fails, f"ln_bwd {style} C={C}: more than 4 x torch's fp32 error: {fails}"


# =========================================================================== fused q/k norm in attention
ATTN_CASES = [((1, 33, 2, 32), 4, 4), ((2, 200, 2, 96), 4, 4), ((1, 257, 2, 96), 3, 3), ((1, 288, 2, 64), 3, 3),
              ((1, 300, 2, 128), 5, 5), ((1, 64, 2, 96), 5, 5)]  # (shape, tier to select, variant it must give)


@functools.lru_cache(maxsize=None)
def attn_family_data(B, N, H, hd, eps, families=tuple(fam.FAMILIES)):
    """As test_gpu_bf16_budget.attn_data with the q/k norm on, the q and k heads being family rows."""
    C = H * hd
    s = 1000 * N + hd
    q, _ = fam.family_rows(B * N * H, hd, BF, seed=s, families=list(families))
    k, _ = fam.family_rows(B * N * H, hd, BF, seed=s + 1, families=list(families))
    v = randn(B * N, C, seed=s + 2) * bb.pow2((C,), -3, 3, s + 3, DEV)
    gq, gk = ((2.0 + 0.1 * randn(hd, seed=s + 4 + i)).float() for i in range(2))
    bq, bk = ((0.1 * randn(hd, seed=s + 6 + i)).float() for i in range(2))
    nrm = (gq, bq, gk, bk)
    qkv = torch.cat([q.view(B * N, C).to(DEV), k.view(B * N, C).to(DEV), v.to(BF)], 1).contiguous()
    q64, k64, v64 = qkv.double().view(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    ref, model, sabs, _, _, _ = bb.attention_ref_model(q64, k64, v64, 1.0 / math.sqrt(hd), nrm, eps)
    unperm = lambda t: t.permute(0, 2, 1, 3).reshape(B * N, C)  # noqa: E731
    return qkv, nrm, unperm(ref), unperm(model), unperm(sabs)


def run_attention(qkv, nrm, B, N, H, hd, eps, kern, want, q_rows=None):
    o = torch.full((B * N, H * hd), float("nan"), dtype=BF, device=DEV)
    old = sp.lib().sdp_attention_set_kernel(kern)
    try:
        v = sp.attention_variant(BF, N, H, hd)
        assert v == want, f"attention {(B, N, H, hd)} under tier {kern}: variant {v}, expected {want}"
        sp.attention(qkv.clone(), o, B, N, H, hd, qk_norm=nrm, eps=eps, q_rows=q_rows)
        torch.cuda.synchronize()
    finally:
        sp.lib().sdp_attention_set_kernel(old)
    return o


@pytest.mark.parametrize("shape,kern,want", ATTN_CASES, ids=[f"{s}-tier{k}" for s, k, _ in ATTN_CASES])
def test_attention_qk_norm_families(shape, kern, want):
    B, N, H, hd = shape
    assert shape == (1, 64, 2, 96) or ATTN_HOME[shape] == (kern, want)
    qkv, nrm, ref, model, sabs = attn_family_data(B, N, H, hd, 1e-5)
    o = run_attention(qkv, nrm, B, N, H, hd, 1e-5, kern, want)
    bb.assert_rms_vs_model(o, model, ref, bb.budget_scale(ref, sabs), 1.25, f"attention qk-norm families {shape} tier {kern}")


def test_attention_qk_norm_tiny_rows_eps():
    """eps = 1e-3 on tiny rows (variance 1e-4): a kernel that ignores its eps is off by a factor 3."""
    B, N, H, hd = 2, 200, 2, 96
    qkv, nrm, ref, model, sabs = attn_family_data(B, N, H, hd, 1e-3, families=("tiny",))
    o = run_attention(qkv, nrm, B, N, H, hd, 1e-3, 4, 4)
    bb.assert_rms_vs_model(o, model, ref, bb.budget_scale(ref, sabs), 1.25, "attention qk-norm tiny rows eps=1e-3")


def test_attention_rows_qk_norm_families_bit_equal():
    """sdp_attention_rows with q_rows = 4: the rows it writes are the full kernel's, bit for bit."""
    B, N, H, hd = 2, 200, 2, 96
    qkv, nrm, _, _, _ = attn_family_data(B, N, H, hd, 1e-5)
    full = run_attention(qkv, nrm, B, N, H, hd, 1e-5, 4, 4)
    part = run_attention(qkv, nrm, B, N, H, hd, 1e-5, 4, 4, q_rows=4)
    C = H * hd
    assert torch.equal(part.view(B, N, C)[:, :4], full.view(B, N, C)[:, :4])


# =========================================================================== losses and softmax
LOSS_B = 16
GS = 8.0


def close_loss(got, ref64, what):
    """The existing loss tests' tolerance (test_gpu_train_kernels.close at rel 1e-5)."""
    got, ref64 = float(got), float(ref64)
    assert math.isfinite(got), f"{what}: {got}"
    print(f"RATIO {what}: loss {got!r} ref {ref64!r} relative error {abs(got - ref64) / max(1e-6, abs(ref64)):.3e}")
    assert abs(got - ref64) <= 1e-5 * max(1e-6, abs(ref64)), f"{what}: {got!r} vs {ref64!r}"


def judge_grad(got, ref64, t32, names, what):
    """Per element: |got - ref| <= 4 x torch fp32's own error at that element, that error floored at
    2^-22 |ref| (an element torch happens to hit exactly still leaves four of its ulps); plus half a
    bf16 ulp of the reference for a bf16 result.  Prints the worst ratio of every logit family.

    Measured on an MI355X (profiles/input_families.md): with fp32 arithmetic throughout, 20 fp32
    gradient cases missed this by up to 10.6x -- where the gradient is a cancelling difference
    (softmax - smoothed target, the two distillation terms, P (dP - sum P dP)) or the logits span
    +-40 (l - max rounds at 3.8e-6 of the probability) -- because torch's error at one element is a
    random draw.  ce_k, distill_k and the fp32 softmax backward therefore form those differences
    in fp64 and round once: every fp32 case is now at 0.06 (0.25 at worst) of the bound."""
    got64, ref64 = got.double(), ref64.to(got.device)
    assert torch.isfinite(got64).all(), f"{what}: non-finite gradient"
    allowed = 4.0 * torch.maximum((t32.double().to(got.device) - ref64).abs(), 2.0 ** -22 * ref64.abs())
    if got.dtype == BF:
        allowed = allowed + 0.5 * bb.ulp_bf16(ref64.abs() + allowed)
    err = (got64 - ref64).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / allowed).amax(1)
    masks = fam.family_masks(names, r.device)
    per = {f: float(r[m].max()) for f, m in masks.items()}
    print(f"RATIO {what}: " + " ".join(f"{f}={v:.3f}" for f, v in per.items()))
    bad = {f: v for f, v in per.items() if not v <= 1.0}
    assert not bad, f"{what}: gradient elements outside their bound (worst error / bound per family): {bad}"


def soft_targets(B, K, seed):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randint(0, K, (B,), generator=g), torch.randint(0, K, (B,), generator=g)
    lam = torch.rand(B, 1, generator=g)
    return (lam * F.one_hot(a, K) + (1 - lam) * F.one_hot(b, K)).float(), a


def ref_and_t32(fn, logits):
    """(loss64, grad64, grad of the same torch expression in fp32) of GS * fn(z) on the stored logits."""
    out = []
    for dt in (torch.float64, F32):
        z = logits.detach().cpu().to(dt).requires_grad_(True)
        loss = fn(z)
        (gz,) = torch.autograd.grad(loss * GS, z)
        out.append((loss.detach(), gz))
    return out[0][0], out[0][1], out[1][1]


@pytest.mark.parametrize("eps,inf", [(0.0, False), (0.125, False), (0.0, True)], ids=["eps0", "eps0.125", "eps0-neginf"])
@pytest.mark.parametrize("K", [10, 1000])
@pytest.mark.parametrize("variant", ["plain", "ignore", "counted"])
@ln_params
def test_ce_loss_logit_families(dtype, variant, K, eps, inf):
    """sdp_ce_loss, sdp_ce_loss_ignore and sdp_ce_loss_counted.  -inf on classes the label does not
    name only without smoothing (with it the smoothed target gives those classes weight and the loss
    is +inf in torch too; soft targets likewise, so sdp_ce_loss_soft gets finite logits only)."""
    B = LOSS_B
    labels = (torch.arange(B) * 7 + 3) % K
    logits, names = fam.logit_rows(B, K, dtype, 700 + K, keep=labels if inf else None)
    ignore = -100
    if variant != "plain":
        labels = labels.clone()
        labels[[1, 7]] = ignore
    zl, lab = logits.to(DEV), labels.to(DEV)
    d = torch.full_like(zl, float("nan"))
    loss = torch.zeros(1, device=DEV)
    L = sp.lib()
    if variant == "plain":
        rc = L.sdp_ce_loss(sp.dcode(dtype), zl.data_ptr(), zl.stride(0), lab.data_ptr(), B, K, eps, GS, d.data_ptr(),
                           d.stride(0), loss.data_ptr(), None)
        assert rc == 0
    elif variant == "ignore":
        rc = L.sdp_ce_loss_ignore(sp.dcode(dtype), zl.data_ptr(), zl.stride(0), lab.data_ptr(), B, K, eps, GS, ignore,
                                  d.data_ptr(), d.stride(0), loss.data_ptr(), None)
        assert rc == 0
    else:
        sp.ce_loss(zl, lab, eps, GS, d, loss, ignore_index=ignore)
    torch.cuda.synchronize()
    l64, g64, g32 = ref_and_t32(lambda z: F.cross_entropy(z, labels, label_smoothing=eps, ignore_index=ignore), logits)
    what = f"ce_loss {variant} {DT_IDS[dtype == BF]} K={K} eps={eps} {'neginf' if inf else 'finite'}"
    close_loss(loss, l64, what)
    judge_grad(d, g64, g32, names, what)
    if not inf:  # an all-equal row: log K, and the exact softmax
        eq = [i for i, n in enumerate(names) if n == "equal" and labels[i] != ignore]
        nrows = int((labels != ignore).sum())
        tgt = F.one_hot(labels[eq], K).double() * (1 - eps) + eps / K
        want = GS / nrows * (1.0 / K - tgt)
        err = (d[eq].double().cpu() - want).abs()
        lim = 2.0 ** -22 * want.abs() + (0.5 * bb.ulp_bf16(want) if dtype == BF else 0.0)
        assert bool((err <= lim).all()), f"{what}: all-equal rows: softmax not 1 / K"


@pytest.mark.parametrize("eps", [0.0, 0.125])
@pytest.mark.parametrize("K", [10, 1000])
@ln_params
def test_ce_loss_soft_logit_families(dtype, K, eps):
    B = LOSS_B
    tgt, _ = soft_targets(B, K, 710 + K)
    logits, names = fam.logit_rows(B, K, dtype, 711 + K)
    zl = logits.to(DEV)
    d = torch.full_like(zl, float("nan"))
    loss = torch.zeros(1, device=DEV)
    sp.ce_loss_soft(zl, tgt.to(DEV), eps, GS, d, loss)
    torch.cuda.synchronize()
    l64, g64, g32 = ref_and_t32(lambda z: F.cross_entropy(z, tgt.to(z.dtype), label_smoothing=eps), logits)
    what = f"ce_loss_soft {DT_IDS[dtype == BF]} K={K} eps={eps}"
    close_loss(loss, l64, what)
    judge_grad(d, g64, g32, names, what)


@pytest.mark.parametrize("eps", [0.0, 0.125])
@pytest.mark.parametrize("K", [10, 1000])
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@ln_params
def test_bce_loss_logit_families(dtype, soft, K, eps):
    B = LOSS_B
    tgt, lab = soft_targets(B, K, 720 + K)
    logits, names = fam.logit_rows(B, K, dtype, 721 + K)
    zl = logits.to(DEV)
    d = torch.full_like(zl, float("nan"))
    loss = torch.zeros(1, device=DEV)
    if soft:
        sp.bce_loss_soft(zl, tgt.to(DEV), eps, GS, d, loss)
        t = tgt
    else:
        sp.bce_loss(zl, lab.to(DEV), eps, GS, d, loss)
        t = F.one_hot(lab, K).float()
    torch.cuda.synchronize()
    l64, g64, g32 = ref_and_t32(
        lambda z: F.binary_cross_entropy_with_logits(z, (t.double() * (1 - eps) + eps / K).to(z.dtype)), logits)
    what = f"bce_loss {'soft' if soft else 'hard'} {DT_IDS[dtype == BF]} K={K} eps={eps}"
    close_loss(loss, l64, what)
    judge_grad(d, g64, g32, names, what)


@pytest.mark.parametrize("K", [10, 1000])
@pytest.mark.parametrize("T", [0.5, 8.0])
@pytest.mark.parametrize("kind", ["soft", "hard"])
@pytest.mark.parametrize("base", ["ce", "bce"])
@ln_params
def test_distill_loss_logit_families(dtype, base, kind, T, K):
    """Student and teacher both from the logit families (the teacher's rows one family on)."""
    import distill_oracle as do
    B, alpha, eps = LOSS_B, 0.5, 0.125
    lab = (torch.arange(B) * 5 + 1) % K
    z, names = fam.logit_rows(B, K, dtype, 730 + K)
    t, _ = fam.logit_rows(B + 1, K, dtype, 731 + K)
    t = t[1:].contiguous()
    zl, tl = z.to(DEV), t.to(DEV)
    d = torch.full_like(zl, float("nan"))
    loss = torch.zeros(1, device=DEV)
    mode = (sp.DISTILL_BCE if base == "bce" else 0) | (sp.DISTILL_HARD if kind == "hard" else 0)
    sp.distill_loss(zl, tl, lab.to(DEV), eps, alpha, T, mode, GS, d, loss)
    torch.cuda.synchronize()
    l64, _, g64 = do.distill(z, t, lab, alpha=alpha, temperature=T, eps=eps, base=base, kind=kind, grad_scale=GS)
    # the same expression through autograd in fp32 (the yardstick of judge_grad)
    z32 = z.float().clone().requires_grad_(True)
    b32, d32 = _distill_parts32(z32, t.float(), lab, T, eps, base, kind)
    (g32,) = torch.autograd.grad(GS * ((1.0 - alpha) * b32 + alpha * d32), z32)
    what = f"distill_loss {base}/{kind} T={T} {DT_IDS[dtype == BF]} K={K}"
    close_loss(loss, l64, what)
    judge_grad(d, g64, g32, names, what)


def _distill_parts32(z, t, lab, T, eps, base, kind):
    """distill_oracle.parts in the dtype of z (fp32): torch's own arithmetic at that precision."""
    import distill_oracle as do
    B, K = z.shape
    yy = ((1.0 - eps) * F.one_hot(lab, K) + eps / K).to(z.dtype)
    if base == "ce":
        b = -(yy * torch.log_softmax(z, 1)).sum() / B
    else:
        b = F.binary_cross_entropy_with_logits(z, yy, reduction="sum") / (B * K)
    if kind == "soft":
        q = torch.softmax(t / T, 1)
        cross = torch.where(q > 0, q * (t - z) / T, torch.zeros_like(q)).sum(1)
        d = T * T * (cross - torch.logsumexp(t / T, 1) + torch.logsumexp(z / T, 1)).sum() / B
    else:
        d = -torch.log_softmax(z, 1).gather(1, do.teacher_label(t)[:, None]).sum() / B
    return b, d


@pytest.mark.parametrize("N", [53, 260])
@pytest.mark.parametrize("inf", [False, True], ids=["finite", "neginf"])
@ln_params
def test_softmax_logit_families(dtype, inf, N):
    """sdp_softmax_fwd, sdp_softmax_fwd_mask (an additive bias that moves every row by its own
    constant and -- neginf -- masks classes out) and sdp_softmax_bwd.  P per element against fp64 by
    judge_grad's rule; an all-equal row gives exactly the stored 1 / N; dS from the stored P and dP
    likewise."""
    rows, Npad = 32, (N + 7) // 8 * 8
    keep = (torch.arange(rows) * 5 + 2) % N
    S, names = fam.logit_rows(rows, N, F32, 740 + N, keep=keep if inf else None)
    Sp = torch.zeros(rows, Npad)
    Sp[:, :N] = S
    Sd = Sp.to(DEV)
    P = torch.full((rows, Npad), float("nan"), dtype=dtype, device=DEV)
    sp.softmax_fwd(Sd, P, None, rows, N, Npad, 1.0)
    torch.cuda.synchronize()
    ref = torch.softmax(S.double(), 1)
    t32 = torch.softmax(S, 1)
    what = f"softmax {DT_IDS[dtype == BF]} N={N} {'neginf' if inf else 'finite'}"
    judge_grad(P[:, :N], ref, t32, names, what + " fwd")
    assert bool((P[:, N:] == 0).all())
    eq = torch.tensor([n == "equal" for n in names])
    assert torch.equal(P[:, :N][eq.to(DEV)].cpu(), torch.full((int(eq.sum()), N), 1.0 / N).to(dtype)), "all-equal rows"
    # masked: rows = N x N of one head, bias = a per-row constant (cancels) and -inf off the kept set
    Sq, qn = fam.logit_rows(N, N, F32, 741 + N)
    bias = (torch.arange(N, dtype=torch.float32) % 7 - 3.0)[:, None].expand(N, N).clone()
    if inf:
        drop = (torch.rand(N, N, generator=torch.Generator().manual_seed(742)) < 0.5)
        drop[torch.arange(N), torch.arange(N)] = False
        bias[drop] = -math.inf
    Sqp = torch.zeros(N, Npad)
    Sqp[:, :N] = Sq
    Pm = torch.full((N, Npad), float("nan"), dtype=dtype, device=DEV)
    sp.softmax_fwd(Sqp.to(DEV), Pm, None, N, N, Npad, 1.0, mask=(bias.to(DEV), 0, 0, 1))
    torch.cuda.synchronize()
    judge_grad(Pm[:, :N], torch.softmax(Sq.double() + bias.double(), 1), torch.softmax(Sq + bias, 1), qn,
               what + " fwd_mask")
    # backward from the stored P
    dP = torch.zeros(rows, Npad, dtype=dtype, device=DEV)
    dP[:, :N] = randn(rows, N, seed=743).to(dtype)
    dS = torch.full((rows, Npad), float("nan"), dtype=dtype, device=DEV)
    sp.softmax_bwd(P, dP, dS, rows, N, Npad)
    torch.cuda.synchronize()
    P64, dP64 = P[:, :N].double(), dP[:, :N].double()
    ref_b = P64 * (dP64 - (P64 * dP64).sum(1, keepdim=True))
    P32, dP32 = P[:, :N].float(), dP[:, :N].float()
    t32_b = P32 * (dP32 - (P32 * dP32).sum(1, keepdim=True))
    judge_grad(dS[:, :N], ref_b, t32_b, names, what + " bwd")


@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("K", [10, 1000])
@ln_params
def test_logits_metrics_logit_families(dtype, K, ls):
    """Per-row CE, BCE row sum and top-1 hit; tolerance of test_logits_metrics_vs_torch against fp64."""
    B = LOSS_B
    lab = (torch.arange(B) * 3 + 1) % K
    x, names = fam.logit_rows(B, K, dtype, 750 + K)
    m = sp.logits_metrics(x.to(DEV), lab.to(DEV), ls).cpu().double()
    x64 = x.double()
    ce = F.cross_entropy(x64, lab, reduction="none")
    t = F.one_hot(lab, K).double() * (1 - ls) + ls / K
    bce = F.binary_cross_entropy_with_logits(x64, t, reduction="none").sum(1)
    e_ce, e_bce = (m[:, 0] - ce).abs(), (m[:, 1] - bce).abs()
    print(f"RATIO logits_metrics {DT_IDS[dtype == BF]} K={K} ls={ls}: ce worst {float((e_ce / (1e-5 + 1e-5 * ce.abs())).max()):.3f} "
          f"bce worst {float((e_bce / (1e-3 + 1e-5 * bce.abs())).max()):.3f} of the tolerance")
    assert bool((e_ce <= 1e-5 + 1e-5 * ce.abs()).all()), ("ce", names, e_ce)
    assert bool((e_bce <= 1e-3 + 1e-5 * bce.abs()).all()), ("bce", names, e_bce)
    # the first maximal index wins (torch.argmax on the stored values; equal rows: index 0)
    assert torch.equal(m[:, 2], (x64.argmax(1) == lab).double())


# =========================================================================== activations, every bf16 value
U23 = 2.0 ** -23       # one fp32 ulp, relative, at the bottom of a binade
FTZ = 2.0 ** -126      # a result below the smallest normal may be flushed to zero
SELU_A, SELU_S = 1.6732632423543772848, 1.0507009873554804934
ACT_CODES = list(range(8))


def act_ref64(code, x):
    """(act(x), act'(x)) in fp64, the definitions of common.h's apply_act / act_grad."""
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    if code == 0:
        return x, one
    if code == 1:
        return bb.gelu_erf64(x), bb.gelu_erf_grad64(x)
    if code == 2:
        return torch.relu(x), torch.where(x > 0, one, zero)
    if code == 3:
        t = torch.tanh(x)
        return t, 1.0 - t * t
    if code == 4:
        s = torch.sigmoid(x)
        return s, s * torch.sigmoid(-x)
    if code == 5:
        return torch.where(x >= 0, x, 0.01 * x), torch.where(x > 0, one, 0.01 * one)
    if code == 6:
        return (SELU_S * torch.where(x > 0, x, SELU_A * torch.expm1(x)),
                torch.where(x > 0, SELU_S * one, SELU_S * SELU_A * torch.exp(x)))
    a, k = 3.5, math.pi / 3.5
    mid = (x >= -a) & (x <= a)
    xm = torch.where(mid, x, zero)
    y = 0.5 * xm * (1.0 + xm / a + torch.sin(k * xm) / math.pi)
    g = 0.5 * (1.0 + 2.0 * xm / a + torch.sin(k * xm) / math.pi + xm * torch.cos(k * xm) / a)
    return torch.where(x < -a, zero, torch.where(x > a, x, y)), torch.where(x < -a, zero, torch.where(x > a, one, g))


def act_bound(code, x, y, g):
    """(e of act, e of act') per element: the absolute error an fp32 evaluation is allowed.
    none, relu: exact.  leaky: one rounding.  gelu (erf form): the 4.2e-7 / 3.0e-7 common.h documents
    for norm_cdf's Abramowitz & Stegun form, plus two roundings.  tanh, sigmoid, selu: libm's tanhf /
    expf / expm1f at 2 ulps and at most two more operations: 4 ulps of the result; their derivatives
    1 - t^2 and s (1 - s) carry the 4 ulps of t (twice: t^2) or s against a difference from 1:
    (1 + 8 t^2) and 6 s ulps.  kelu: 0.5 x (1 + x / a + sin(pi x / a) / pi) is a sum that cancels to a
    cubic zero at x = -a; every term is rounded at its own size, so the bound is 4 ulps of the sum
    of the absolute terms (the rounding of sin's argument, 2 ulps of |x / a|, counted with them),
    likewise for its derivative.  Results below the smallest normal may be flushed (FTZ)."""
    ax = x.abs()
    if code in (0, 2):
        e = eg = torch.zeros_like(x)
    elif code == 1:
        e, eg = 4.2e-7 + 2.0 * U23 * y.abs(), 3.0e-7 + 2.0 * U23 * g.abs()
    elif code == 3:
        e, eg = 4.0 * U23 * y.abs(), U23 * (1.0 + 8.0 * y * y)
    elif code == 4:
        e, eg = 4.0 * U23 * y.abs(), 6.0 * U23 * y
    elif code == 5:
        e, eg = U23 * y.abs(), U23 * g.abs()  # (0.01 is not an fp32 value)
    elif code == 6:
        e, eg = 4.0 * U23 * y.abs(), 4.0 * U23 * g.abs()
    else:
        a, k = 3.5, math.pi / 3.5
        mid = (ax <= a).double()
        u = ax / a
        s, c = torch.sin(k * x).abs() / math.pi, torch.cos(k * x).abs()
        e = mid * 4.0 * U23 * 0.5 * ax * (1.0 + 2.0 * u + s)
        eg = mid * 4.0 * U23 * 0.5 * (1.0 + 2.0 * u + s + u * c + 2.0 * u * (c + k * ax * s * math.pi))
    return e + FTZ, eg + FTZ


@functools.lru_cache(maxsize=None)
def act_inputs(dtype):
    """bf16: all 65,536 bit patterns as [512, 128].  fp32: the same values widened, the fp32
    neighbours of 0 and +-3.5, and 2^20 points on [-12, 12], padded with zeros to [., 128]."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)
    if dtype == BF:
        return bits.view(512, 128).to(DEV)
    near = []
    for c in (0.0, 3.5, -3.5):
        v = torch.tensor(c, dtype=F32)
        for _ in range(4):
            v = torch.nextafter(v, torch.tensor(math.inf))
            near.append(v.clone())
        v = torch.tensor(c, dtype=F32)
        for _ in range(4):
            v = torch.nextafter(v, torch.tensor(-math.inf))
            near.append(v.clone())
    x = torch.cat([bits.float(), torch.stack(near), torch.linspace(-12.0, 12.0, 1 << 20, dtype=torch.float64).float()])
    pad = (-x.numel()) % 128
    return torch.cat([x, torch.zeros(pad)]).view(-1, 128).to(DEV)


TORCH_ACT = {0: lambda x: x, 1: F.gelu, 2: torch.relu, 3: torch.tanh, 4: torch.sigmoid,
             5: lambda x: F.leaky_relu(x, 0.01), 6: F.selu}


def judge_act(got, x64, ref, e, dtype, what, nan_out=True, ref_inf=None, pre=None):
    """Finite inputs within e (+ half a bf16 ulp); NaN in gives NaN out (``nan_out``; a derivative
    only where the reference's comparison form gives NaN as well); at +-inf what ``ref_inf`` (torch's
    own function in fp64; default the reference) gives, where that is not NaN; a reference at or
    past the format's largest value (selu of the largest inputs) may come out as that value or as
    inf, and so may a result whose fp32 intermediate ``pre`` (the activation before a row scale) is."""
    got64 = got.double()
    nan_in, inf_in = torch.isnan(x64), torch.isinf(x64)
    fin = ~nan_in & ~inf_in
    must_nan = nan_in if nan_out else nan_in & torch.isnan(ref)
    assert bool(torch.isnan(got64[must_nan]).all()), f"{what}: NaN in did not give NaN out"
    rinf = ref if ref_inf is None else ref_inf
    chk = inf_in & ~torch.isnan(rinf)
    gi, ri = got64[chk], rinf[chk]
    tol = torch.where(torch.isinf(ri), torch.zeros_like(ri),
                      4.0 * U23 * ri.abs() + (0.5 * bb.ulp_bf16(ri) if dtype == BF else 0.0))
    ok = torch.where(torch.isinf(ri), gi == ri, (gi - ri).abs() <= tol)
    assert bool(ok.all()), f"{what}: at +-inf {gi.tolist()} expected {ri.tolist()}"
    g, r, ee = got64[fin], ref[fin], e[fin]
    xf = x64[fin]
    fmax = 3.3895313892515355e38 if dtype == BF else 3.4028234663852886e38
    over = r.abs() + ee >= fmax
    if pre is not None:
        over = over | (pre[fin].abs() >= 3.4028234663852886e38)
    assert bool(((g[over].abs() >= 0.99 * fmax) & (torch.sign(g[over]) == torch.sign(r[over]))).all()), \
        f"{what}: a result past the format's range is neither its largest value nor inf"
    g, r, ee, xf = g[~over], r[~over], ee[~over], xf[~over]
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite output on a finite input"
    bound = ee + 0.5 * bb.ulp_bf16(r.abs() + ee) if dtype == BF else ee
    err = (g - r).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    i = int(ratio.argmax())
    print(f"RATIO {what}: worst element at {float(ratio[i]):.3f} of its bound (x = {float(xf[i])!r}, "
          f"got {float(g[i])!r}, ref {float(r[i])!r})")
    assert float(ratio[i]) <= 1.0, (f"{what}: {int((ratio > 1).sum())} elements outside the bound; worst x = "
                                     f"{float(xf[i])!r}: got {float(g[i])!r} ref {float(r[i])!r} bound {float(bound[i]):.3e}")


@pytest.mark.parametrize("code", ACT_CODES)
@ln_params
def test_activations_on_every_bf16_value(dtype, code):
    """sdp_act, sdp_act_fwd, sdp_act_bwd (dy a power of two: the product is exact) and
    sdp_act_rowscale_add (row scales powers of two, at most 1) on every value."""
    x = act_inputs(dtype)
    M, N = x.shape
    x64 = x.double()
    y64, g64 = act_ref64(code, x64)
    e, eg = act_bound(code, x64, y64, g64)
    name = f"act {code} {DT_IDS[dtype == BF]}"
    t64 = TORCH_ACT[code](x64) if code in TORCH_ACT else y64  # (kelu is this project's own)
    y = torch.full_like(x, float("nan"))
    sp.act(x, y, code)
    judge_act(y, x64, y64, e, dtype, f"sdp_act {name}", ref_inf=t64)
    y2 = torch.full_like(x, float("nan"))
    sp.act_fwd(x, y2, M, N, code)
    judge_act(y2, x64, y64, e, dtype, f"sdp_act_fwd {name}", ref_inf=t64)
    dy64 = bb.pow2((M, N), -3, 3, 800, DEV) * torch.where(torch.arange(N, device=DEV) % 2 == 0, 1.0, -1.0)
    dz = torch.full_like(x, float("nan"))
    sp.act_bwd(x, dy64.to(dtype), dz, M, N, code)
    judge_act(dz, x64, dy64 * g64, dy64.abs() * eg, dtype, f"sdp_act_bwd {name}", nan_out=False)
    if code:
        sc = bb.pow2((M,), -3, 0, 801, DEV).float()
        y3 = torch.full_like(x, float("nan"))
        sp.rowscale_add(sp.dense(x), sp.dense(y3), M, N, scale=sc, act=code)
        s64 = sc.double()[:, None]
        judge_act(y3, x64, y64 * s64, e * s64, dtype, f"sdp_act_rowscale_add {name}", ref_inf=t64 * s64, pre=y64)


@pytest.mark.parametrize("kern", [9, 14])
def test_gemm_epilogue_gelu_fast_on_every_finite_bf16_value(kern):
    """The bf16 GEMM epilogue's GELU (common.h gelu_fast): every finite bf16 value times the
    identity, so the pre-activation is the value itself.  Against the fp64 tanh form within
    ulp_bf16 / 2 + (8 + 2 |u| t / (1 + t)) 2^-24 |y| (test_gpu_bf16_budget.act64: u = x (x^2 K2 + K)
    takes two fma and a mul, v_exp_f32 and v_rcp_f32 1 ulp each, one add, one mul -- 8 half-ulps --
    and the rounding of the exponent u scales with its size and reaches y through t = exp2(u) by
    t / (1 + t)) + FTZ + the overflow of t.  The distance to the erf form is held to common.h's
    4.7e-4 absolute (+ the half ulp of the bf16 output) and printed with the relative figure for
    |y| > 0.05 (0.22 % there, of the fp32 value)."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)
    x = bits[torch.isfinite(bits.float())].view(-1, 128).contiguous().to(DEV)
    M, N = x.shape
    assert M == 510 and sp.gemm_variant(BF, M, N, N) == 1
    w = torch.eye(N, dtype=BF, device=DEV)
    y = torch.full_like(x, float("nan"))
    L = sp.lib()
    old, oldg = L.sdp_gemm_set_fast_kernel(kern), L.sdp_gemm_set_exact_gelu(0)
    try:
        sp.gemm(sp.dense(x), w, sp.dense(y), M, N, N, act=1)
        torch.cuda.synchronize()
    finally:
        L.sdp_gemm_set_exact_gelu(oldg)
        L.sdp_gemm_set_fast_kernel(old)
    x64 = x.double()
    ref = bb.gelu_tanh64(x64)
    # t = exp2(u), y = x / (1 + t): the exponent's rounding moves t by 2 |u| 2^-24 relative and y by
    # t / (1 + t) of that (nothing once t has underflowed)
    u = (x64 * (x64 * x64 * 0.10294324471 + 2.3022081983)).abs()
    share = torch.sigmoid(-2.0 * math.sqrt(2.0 / math.pi) * (x64 + 0.044715 * x64 ** 3))
    # once u >= 128 (x <= -10.06) t is inf in fp32 and y = -0, the exact y being below |x| 2^-128
    e = (8.0 + 2.0 * u * share) * 2.0 ** -24 * ref.abs() + FTZ + torch.where(x64 < 0, x64.abs() * 2.0 ** -128, 0.0)
    judge_act(y, x64, ref, e, BF, f"gemm k{kern} gelu_fast")
    erf = bb.gelu_erf64(x64)
    d = (y.double() - erf).abs()
    big = erf.abs() > 0.05
    rel = (d / erf.abs())[big]
    lim = 4.7e-4 + 0.5 * bb.ulp_bf16(erf)  # the comment's figure is of the fp32 value; the output is bf16
    print(f"RATIO gemm k{kern} gelu_fast vs erf GELU: max abs {float(d.max()):.3e} at x = {float(x64.flatten()[d.argmax()])!r}; "
          f"max relative for |y| > 0.05 {float(rel.max()):.3e}; worst |d| / (4.7e-4 + ulp / 2) {float((d / lim).max()):.3f}")
    assert bool((d <= lim).all()), "gelu_fast is further from the erf GELU than common.h states"
