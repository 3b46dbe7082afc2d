"""Rounding-budget checks for the bf16 fast-path kernels, and the fp64 rounding models they share.

The bf16 kernels take bf16 operands, accumulate in fp32 and round to bf16 at a few documented
points (include/sdpnet_hip.h, "bf16 rounding points").  Judging them by "max error <= 1e-2 of the
largest output" leaves about five bf16 ulps of the largest element for every element; the two
checks here leave what the arithmetic allows:

* ``assert_elementwise``: every element within ``e + ulp/2`` of the fp64 reference, ``e`` being the
  caller's derived bound of the fp32 arithmetic (worst case, so it is slack for long sums);
* ``assert_rms_vs_model``: the RMS of the error in units of a per-element budget ``D`` at most
  ``margin`` times the same figure of the *rounding model* -- the fp64 reference rounded to bf16
  (to nearest even) at exactly the points where the kernel rounds.  This is the sharp check: an
  output that is truncated, scaled by 0.3 %, or rounded once more than declared moves it by 2x or
  more (tests/test_budget_selfcheck.py).

Everything is plain torch on whatever device the inputs live on (the self-check runs on the CPU).
"""
import math

import torch

BF16_MIN_NORMAL_EXP = -126


def ulp_bf16(a):
    """Spacing of bf16 at magnitude |a| (fp64): 2^(floor(log2 |a|) - 7), floored at the smallest
    normal (below it the spacing is constant)."""
    a = torch.as_tensor(a).double().abs().clamp_min(2.0 ** BF16_MIN_NORMAL_EXP).contiguous()
    # through the exponent field (exact on every device; a is a normal double after the clamp):
    # floor(log2 a) = field - 1023, and 2^n is the double with field n + 1023
    ex = (a.view(torch.int64) >> 52) & 0x7FF
    return ((ex - 7) << 52).view(torch.float64)


def rne_bf16(x):
    """fp64 -> nearest bf16 value (ties to even), returned as fp64.  Not through torch's
    double -> float -> bfloat16 casts, which round twice."""
    x = x.double()
    u = ulp_bf16(x)
    return torch.round(x / u) * u  # x / u is exact (power of two); torch.round is half-to-even


def trunc_bf16(x):
    """fp64 -> bf16 by dropping the low bits (the faulty variants of the self-check)."""
    x = x.double()
    u = ulp_bf16(x)
    return torch.trunc(x / u) * u


def budget_scale(ref64, sum_abs_terms):
    """D = ulp_bf16(ref) / 2 + 2^-9 * sum_j |t_j|, t_j the fp64 terms whose sum is the element."""
    return 0.5 * ulp_bf16(ref64) + 2.0 ** -9 * sum_abs_terms.double()


def budget_rms(got, ref64, D):
    """RMS over all elements of (got - ref64) / D."""
    r = (got.double() - ref64.double()) / D.double()
    return float(torch.sqrt((r * r).mean()))


def assert_elementwise(got, ref64, e, what=""):
    """Every element: |got - ref64| <= e + ulp_bf16(|ref64| + e) / 2 (no share left out)."""
    got, ref64 = got.double(), ref64.double()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    e = torch.as_tensor(e, dtype=torch.float64, device=ref64.device).expand_as(ref64)
    bound = e + 0.5 * ulp_bf16(ref64.abs() + e)
    err = (got - ref64).abs()
    over = err > bound
    print(f"BUDGET {what}: worst element at {float((err / bound).max()):.3f} of its bound")
    if bool(over.any()):
        i = int(torch.argmax(err / bound))
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape))
        g, r, b = (float(t.reshape(-1)[i]) for t in (got, ref64, bound))
        raise AssertionError(f"{what}: {int(over.sum())} of {err.numel()} elements outside the budget; worst at "
                             f"{idx}: got {g!r} ref {r!r} |err| {abs(g - r):.4e} bound {b:.4e}")


def assert_rms_vs_model(got, model, ref64, D, margin, what=""):
    """budget_rms(got) <= margin * budget_rms(model); prints both and their ratio (pytest -s)."""
    assert torch.isfinite(got.double()).all(), f"{what}: non-finite output"
    rk, rm = budget_rms(got, ref64, D), budget_rms(model, ref64, D)
    ratio = rk / rm if rm > 0 else (0.0 if rk == 0 else math.inf)
    print(f"BUDGET {what}: kernel {rk:.4f} model {rm:.4f} ratio {ratio:.3f} (margin {margin})")
    assert rk <= margin * rm, f"{what}: budget_rms {rk:.4f} > {margin} x model {rm:.4f} (ratio {ratio:.3f})"
    return rk, rm, ratio


def pow2(shape, lo, hi, seed, device="cpu"):
    """Powers of two 2^lo .. 2^hi, drawn uniformly in the exponent (seeded, made on the CPU)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    ex = torch.randint(lo, hi + 1, shape, generator=g)
    return torch.ldexp(torch.ones(shape, dtype=torch.float64), ex).to(device)


# ------------------------------------------------------------------ activations (fp64)
GELU_LIPSCHITZ = 1.13  # max |gelu'| = 1.1289 (erf form; the tanh form's is within 1e-3 of it)


def gelu_tanh64(x):
    """The header's tanh form: x * sigmoid(2 sqrt(2/pi) (x + 0.044715 x^3)) = 0.5 x (1 + tanh(..))."""
    return x * torch.sigmoid(2.0 * math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))


def gelu_erf64(x):
    return 0.5 * x * (1.0 + torch.special.erf(x / math.sqrt(2.0)))


def gelu_erf_grad64(x):
    return 0.5 * (1.0 + torch.special.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


# ------------------------------------------------------------------ eval attention (fp64)
def head_ln64(x, g, b, eps, unbiased=False):
    mu = x.mean(-1, keepdim=True)
    var = x.var(-1, unbiased=unbiased, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g.double() + b.double()


def attention_element_bound(q, k, sabs, scale):
    """Element bound e of flash attention without the q/k norm (q, k exact bf16 values).
    The fp32 score error ds <= 2 hd 2^-24 scale sum_d |q_d k_d| moves every softmax weight by at
    most a factor e^(2 ds).  P rounds into the numerator only, by at most 2^-8 relative: half a bf16
    ulp at the bottom of a binade (2^-9 is the figure at the top; a correctly rounded emulation
    exceeds a bound built on it, test_budget_selfcheck.py).  P V accumulates N terms; the row sum,
    exp2 / rcp (1 ulp) and the running-max rescales are a few more fp32 operations (2^-18 covers
    32 of them)."""
    N, hd = q.shape[-2], q.shape[-1]
    ds = (2.0 * hd * 2.0 ** -24 * scale * (q.abs() @ k.abs().transpose(-1, -2))).amax(-1, keepdim=True)
    return (2.0 ** -8 + 2.0 * ds + 2.0 * (N + 8) * 2.0 ** -24 + 2.0 ** -18) * sabs


def attention_ref_model(q, k, v, scale, norm=None, eps=1e-5):
    """q, k, v: fp64 [..., N, hd] holding bf16 values.  Returns (ref, model, sum_abs_terms, w, qn, kn):
    ref = softmax(scale qn kn^T) v exactly; model = the same with the eval kernels' roundings
    (csrc/attention.hip): qn, kn (the head LayerNorm, biased variance) rounded to bf16, P =
    exp(s - rowmax) rounded to bf16 in the numerator only, the output rounded to bf16;
    sum_abs_terms = sum_j w_j |v_j|."""
    qn, kn = q, k
    if norm is not None:
        gq, bq, gk, bk = norm
        qn, kn = head_ln64(q, gq, bq, eps), head_ln64(k, gk, bk, eps)
    w = torch.softmax(qn @ kn.transpose(-1, -2) * scale, -1)
    ref = w @ v
    sabs = w @ v.abs()
    qh, kh = (rne_bf16(qn), rne_bf16(kn)) if norm is not None else (qn, kn)
    s = qh @ kh.transpose(-1, -2) * scale
    p = torch.exp(s - s.amax(-1, keepdim=True))
    model = rne_bf16((rne_bf16(p) @ v) / p.sum(-1, keepdim=True))
    return ref, model, sabs, w, qn, kn
