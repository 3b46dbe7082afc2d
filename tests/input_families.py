"""Input families for the kernel tests, their fp64 references and the bounds they are judged by
(test infrastructure; a plain module, not a conftest).

``randn`` inputs judged by ``max|err| <= tol * max|ref|`` cannot see three kinds of mistake:

* a LayerNorm variance taken as E[x^2] - mean^2: exact enough at zero mean and unit spread, lost
  to cancellation when a row's offset is far above its spread (``offset``, ``one_step``, ``flat``);
* an ``eps`` that is ignored, hard-coded or added after the square root: at unit variance 1e-5 and
  1e-6 differ by 5e-6 relative in the output, at spread 1e-2 (``tiny``) by 5 %;
* a loss or softmax that forgets the row maximum (``logit_rows``: common offset, dominant logit,
  all-equal rows, wide spread, -inf classes).

Rows of a mixed tensor take family ``i mod n`` so one launch covers all families, and every value
is representable in the dtype under test: the reference sees exactly what the kernel sees.

The LayerNorm bound (``ln_bound``) is that of a LayerNorm whose mean and variance are each a
correctly ordered fp32 sum of C terms (u = 2^-24, per element, nothing left out):

    e = |gamma| rstd C u max_row|x|  +  2 C u |y - beta|  +  2^-22 |y|

the mean's error (C u max|x|) scaled into the output, the relative error of rstd (a sum of C
squares: 2 C u on the variance, half of it on rstd, doubled for the sum order) on the normalised
value, and four roundings of the affine.  bf16 outputs add ulp_bf16(|y| + e) / 2 through
``bf16_budget.assert_elementwise``.  tests/test_input_families_selfcheck.py shows a sequential
two-pass fp32 model inside it for every family, and the one-pass and eps-ignoring models outside.
"""
import math

import torch

import bf16_budget as bb

U = 2.0 ** -24
OFFSETS = (8.0, 32.0, 128.0)
STEP_CONSTS = (1.0, 3.0, 10.0, 100.0)
FLAT_CONSTS = (0.0, 1.0, -3.0, 100.0)
FAMILIES = (["unit"] + [f"offset{int(r)}" for r in OFFSETS] + [f"one_step{int(c)}" for c in STEP_CONSTS]
            + ["flat", "outlier", "tiny", "huge"])
EPS_VALUES = (1e-6, 1e-5, 1e-3)


def _step(c, dtype):
    """One ulp of ``dtype`` at c (bf16), or c 2^-20 (fp32: a step the output still resolves)."""
    if dtype == torch.bfloat16:
        return float(bb.ulp_bf16(torch.tensor(c)))
    return c * 2.0 ** -20


def family_rows(M, C, dtype, seed, families=FAMILIES):
    """(x [M, C] in ``dtype`` on the CPU, [family name of row i]).  Row i is of family i mod n; the
    constants of ``one_step`` / ``flat`` and the position of the step cycle with i // n."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    z = torch.randn(M, C, generator=g, dtype=torch.float64)
    x = torch.empty(M, C, dtype=torch.float64)
    names = []
    n = len(families)
    for i in range(M):
        f, rep = families[i % n], i // n
        names.append(f)
        if f == "unit":
            x[i] = z[i]
        elif f.startswith("offset"):
            x[i] = float(f[6:]) + z[i]
        elif f.startswith("one_step"):
            c = float(f[8:])
            x[i] = c
            x[i, (7 * i + 3 + 31 * rep) % C] = c + _step(c, dtype)
        elif f == "flat":
            x[i] = FLAT_CONSTS[rep % len(FLAT_CONSTS)]
        elif f == "outlier":
            x[i] = z[i]
            x[i, (5 * i + 1) % C] *= 1000.0
        elif f == "tiny":
            x[i] = 1e-2 * z[i]
        elif f == "huge":
            x[i] = 3e4 * z[i]
        else:
            raise ValueError(f)
    return x.to(dtype), names


def family_masks(names, device="cpu"):
    """{family: bool row mask}, in order of first appearance."""
    out = {}
    for f in dict.fromkeys(names):
        out[f] = torch.tensor([n == f for n in names], device=device)
    return out


# --------------------------------------------------------------------------- LayerNorm
def ln_ref64(x, gamma, beta, eps):
    """fp64 LayerNorm over the last dim of the stored values: (y, mean [.., 1], rstd [.., 1])."""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean) * rstd
    if gamma is not None:
        y = y * gamma.double()
    if beta is not None:
        y = y + beta.double()
    return y, mean, rstd


def ln_bound(x, gamma, beta, eps):
    """The module docstring's e, per element (fp64), from the stored values."""
    x = x.double()
    C = x.shape[-1]
    y, _, rstd = ln_ref64(x, gamma, beta, eps)
    g = torch.ones(C, dtype=torch.float64, device=x.device) if gamma is None else gamma.double().abs()
    b = 0.0 if beta is None else beta.double()
    xmax = x.abs().amax(-1, keepdim=True)
    return g * rstd * (C * U) * xmax + 2.0 * C * U * (y - b).abs() + 2.0 ** -22 * y.abs()


def stat_bounds(x, eps):
    """(|d mean| bound [.., 1], relative rstd bound): C u max|x| and 2 C u."""
    x = x.double()
    C = x.shape[-1]
    return C * U * x.abs().amax(-1, keepdim=True), 2.0 * C * U


def family_ratios(got, ref64, e, names, bf16):
    """{family: worst |got - ref| / bound over its rows}; bound = e (+ ulp_bf16(|ref| + e) / 2)."""
    got, ref64 = got.double(), ref64.double()
    e = torch.as_tensor(e, dtype=torch.float64, device=ref64.device).expand_as(ref64)
    bound = e + (0.5 * bb.ulp_bf16(ref64.abs() + e) if bf16 else 0.0)
    r = (got - ref64).abs() / bound
    r = torch.where((got - ref64) == 0, torch.zeros_like(r), r)  # 0 / 0: an exact element
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))
    r = r.reshape(len(names), -1).amax(1)
    return {f: float(r[m.to(r.device)].max()) for f, m in family_masks(names).items()}


def assert_families(got, ref64, e, names, bf16, what=""):
    """Every element within its bound; prints the worst ratio of every family first (pytest -s).
    bf16 goes through bf16_budget.assert_elementwise (the same bound), fp32 is judged by e alone."""
    ratios = family_ratios(got, ref64, e, names, bf16)
    print(f"FAMILY {what}: " + " ".join(f"{f}={v:.3f}" for f, v in ratios.items()))
    if bf16:
        bb.assert_elementwise(got, ref64, e, what)
    bad = {f: v for f, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{what}: outside the bound (worst element / bound per family): {bad}"
    return ratios


def assert_stats(mean, rstd, x, eps, names, what=""):
    """mean, rstd ([M] or [M, 1]) against the fp64 statistics of x: |d mean| <= C u max|x| and
    |d rstd| / rstd <= 2 C u, per row."""
    _, m64, r64 = ln_ref64(x, None, None, eps)
    mb, rb = stat_bounds(x, eps)
    rm = ((mean.double().reshape(-1, 1) - m64).abs() / mb.clamp_min(1e-300)).reshape(-1)
    rm = torch.where(mean.double().reshape(-1) == m64.reshape(-1), torch.zeros_like(rm), rm)
    rr = ((rstd.double().reshape(-1, 1) - r64).abs() / r64 / rb).reshape(-1)
    masks = family_masks(names, rm.device)
    pm = {f: float(rm[m].max()) for f, m in masks.items()}
    pr = {f: float(rr[m].max()) for f, m in masks.items()}
    print(f"FAMILY {what} mean: " + " ".join(f"{f}={v:.3f}" for f, v in pm.items()))
    print(f"FAMILY {what} rstd: " + " ".join(f"{f}={v:.3f}" for f, v in pr.items()))
    bad = {f: (pm[f], pr[f]) for f in pm if not (pm[f] <= 1.0 and pr[f] <= 1.0)}
    assert not bad, f"{what}: statistics outside their bounds (mean, rstd ratios): {bad}"
    return pm, pr


# ------------------------------------------------------------- fp32 models (the self-check's)
def _seq_sum32(t):
    """Left-to-right fp32 sum over the last dim (the worst order a kernel could take)."""
    acc = torch.zeros(t.shape[:-1], dtype=torch.float32)
    for j in range(t.shape[-1]):
        acc = acc + t[..., j]
    return acc


def ln_model32(x, gamma, beta, eps, kind="two_pass"):
    """(y, mean, rstd) of an fp32 LayerNorm on the CPU, output in x's dtype.  kind: ``two_pass``
    (sequential mean, then sequential sum of squared deviations), ``one_pass`` (E[x^2] - mean^2,
    clamped at 0) or ``ignores_eps`` (two-pass with eps = 1e-5 whatever is passed)."""
    x32 = x.float()
    C = x32.shape[-1]
    inv = torch.tensor(1.0 / C, dtype=torch.float32)
    mean = _seq_sum32(x32) * inv
    if kind == "one_pass":
        var = (_seq_sum32(x32 * x32) * inv - mean * mean).clamp_min(0.0)
    else:
        d = x32 - mean[..., None]
        var = _seq_sum32(d * d) * inv
    eps32 = torch.tensor(1e-5 if kind == "ignores_eps" else eps, dtype=torch.float32)
    rstd = 1.0 / torch.sqrt(var + eps32)
    y = (x32 - mean[..., None]) * rstd[..., None] * gamma.float() + beta.float()
    return y.to(x.dtype), mean, rstd


# --------------------------------------------------------------------------- logits
LOGIT_FAMILIES = ["unit", "offset1000", "dominant", "equal", "spread40"]


def logit_rows(B, K, dtype, seed, keep=None):
    """(logits [B, K] in ``dtype`` on the CPU, [family of row i]); row i is of family i mod 5:
    3 randn; 1000 + 3 randn; randn with one logit 80 above the rest; all classes equal (0, 5, -7
    in turn); uniform in [-40, 40].  With ``keep`` (a [B] class index per row, or a [B, K] bool
    mask of classes that must stay finite) about half of the other classes of every row except the
    all-equal ones become -inf (the CE variants and the softmax accept that; nothing else gets it)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    z = torch.randn(B, K, generator=g, dtype=torch.float64)
    u = torch.rand(B, K, generator=g, dtype=torch.float64)
    x = torch.empty(B, K, dtype=torch.float64)
    names = []
    n = len(LOGIT_FAMILIES)
    for i in range(B):
        f, rep = LOGIT_FAMILIES[i % n], i // n
        names.append(f)
        if f == "unit":
            x[i] = 3.0 * z[i]
        elif f == "offset1000":
            x[i] = 1000.0 + 3.0 * z[i]
        elif f == "dominant":
            x[i] = z[i].clamp(-3.0, 3.0)
            x[i, (3 * i + 1) % K] = 83.0
        elif f == "equal":
            x[i] = (0.0, 5.0, -7.0)[rep % 3]
        else:
            x[i] = 80.0 * u[i] - 40.0
    if keep is not None:
        keep = torch.as_tensor(keep)
        km = torch.zeros(B, K, dtype=torch.bool)
        if keep.dtype == torch.bool:
            km = keep.clone()
        else:
            km[torch.arange(B), keep] = True
        drop = (torch.rand(B, K, generator=g) < 0.5) & ~km
        drop[torch.tensor([nm == "equal" for nm in names])] = False
        x[drop] = -math.inf
    return x.to(dtype), names
