"""The input families and the LayerNorm bound (input_families.py) judged on the CPU: three fp32
LayerNorm models -- a sequential two-pass one, the one-pass E[x^2] - mean^2 one and one that
ignores its eps -- against the fp64 reference on the same stored values.  The bound must pass the
first on every family and fail the other two where their arithmetic is wrong: the evidence that
test_gpu_input_families.py can fail.  No mutated kernel is built or run on a GPU."""
import math

import pytest
import torch

import bf16_budget as bb
import input_families as fam

DTYPES = [torch.float32, torch.bfloat16]
CS = [64, 96, 768, 1032]
M = 48  # four rows of every family


def _case(C, dtype):
    x, names = fam.family_rows(M, C, dtype, seed=100 + C)
    g = torch.Generator().manual_seed(C)
    gamma = (1.0 + 0.2 * torch.randn(C, generator=g)).float()
    beta = (0.2 * torch.randn(C, generator=g)).float()
    return x, names, gamma, beta


def _ratios(x, names, gamma, beta, eps, kind):
    y, mean, rstd = fam.ln_model32(x, gamma, beta, eps, kind)
    ref, _, _ = fam.ln_ref64(x, gamma, beta, eps)
    e = fam.ln_bound(x, gamma, beta, eps)
    return fam.family_ratios(y, ref, e, names, x.dtype == torch.bfloat16), (y, ref, e, mean, rstd)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_rows_are_stored_values_of_every_family(dtype):
    x, names = fam.family_rows(M, 96, dtype, seed=1)
    assert x.dtype == dtype and set(names) == set(fam.FAMILIES)
    masks = fam.family_masks(names)
    x64 = x.double()
    assert bool((x64[masks["flat"]].amax(1) == x64[masks["flat"]].amin(1)).all())
    for c in fam.STEP_CONSTS:
        rows = x64[masks[f"one_step{int(c)}"]]
        step = float(bb.ulp_bf16(torch.tensor(c))) if dtype == torch.bfloat16 else c * 2.0 ** -20
        hi = float(torch.tensor(c + step, dtype=torch.float64).to(dtype))  # (fp32: 100 (1 + 2^-20) rounds)
        assert hi > c and abs(hi - (c + step)) <= c * 2.0 ** -24
        assert bool(((rows == c).sum(1) == 95).all()) and bool(((rows == hi).sum(1) == 1).all())
        assert len({int(p) for p in rows.argmax(1)}) > 1  # the position moves
    assert float(x64[masks["offset128"]].mean()) == pytest.approx(128.0, abs=0.2)
    assert float(x64[masks["outlier"]].abs().amax()) > 50.0
    assert float(x64[masks["tiny"]].abs().amax()) < 0.06 and float(x64[masks["huge"]].abs().amax()) > 3e4


@pytest.mark.parametrize("eps", fam.EPS_VALUES)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_two_pass_model_is_inside_the_bound_on_every_family(dtype, C, eps):
    x, names, gamma, beta = _case(C, dtype)
    r, (y, ref, e, mean, rstd) = _ratios(x, names, gamma, beta, eps, "two_pass")
    print(f"two-pass {dtype} C={C} eps={eps}: " + " ".join(f"{f}={v:.3f}" for f, v in r.items()))
    fam.assert_families(y, ref, e, names, dtype == torch.bfloat16, f"two-pass model C={C}")
    fam.assert_stats(mean, rstd, x, eps, names, f"two-pass model C={C}")


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_one_pass_model_is_outside_the_bound(dtype, C):
    """16 rows of every family.  fp32: offset(32) and offset(128) at every C (1.3x to 22x the bound).
    bf16: one_step at c = 10 and 100 at every C (2.9x to 425x; c = 3 leaves it at C <= 768), and
    offset(128) from C = 96 on (1.3x to 6.4x; at C = 64 the half ulp of the bf16 output is still
    the larger share and the row stays at 0.96).  one_step at c = 1 cannot fail: 1 and (1 + 2^-7)^2
    sum exactly in fp32.  unit and tiny rows -- all that randn inputs offer -- stay inside."""
    x, names = fam.family_rows(16 * len(fam.FAMILIES), C, dtype, seed=100 + C)
    _, _, gamma, beta = _case(C, dtype)
    r, (y, ref, e, _, _) = _ratios(x, names, gamma, beta, 1e-5, "one_pass")
    print(f"one-pass {dtype} C={C}: " + " ".join(f"{f}={v:.3f}" for f, v in r.items()))
    if dtype == torch.bfloat16:
        must = ["one_step10", "one_step100"] + (["offset128"] if C >= 96 else []) + (["one_step3"] if C <= 768 else [])
    else:
        must = ["offset32", "offset128"]
    for f in must:
        assert r[f] > 1.0, (f, r[f])
    assert r["unit"] <= 1.0 and r["tiny"] <= 1.0  # what randn-only tests see
    with pytest.raises(AssertionError, match="outside"):
        fam.assert_families(y, ref, e, names, dtype == torch.bfloat16, "one-pass model")


@pytest.mark.parametrize("eps", [1e-6, 1e-3])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_model_that_ignores_eps_fails_tiny(dtype, C, eps):
    x, names, gamma, beta = _case(C, dtype)
    r, (y, ref, e, mean, rstd) = _ratios(x, names, gamma, beta, eps, "ignores_eps")
    print(f"ignores-eps {dtype} C={C} eps={eps}: " + " ".join(f"{f}={v:.3f}" for f, v in r.items()))
    assert r["tiny"] > 1.0, r
    with pytest.raises(AssertionError, match="rstd"):
        fam.assert_stats(mean, rstd, x, eps, names, "ignores-eps model")


def test_unit_rows_do_not_see_eps():
    """Why the families are needed: on randn rows 1e-5 against 1e-6 moves the output by less than
    the fp32 tolerance of the existing tests (2e-5 of the largest output)."""
    x, names, gamma, beta = _case(96, torch.float32)
    unit = fam.family_masks(names)["unit"]
    a, _, _ = fam.ln_ref64(x[unit], gamma, beta, 1e-5)
    b, _, _ = fam.ln_ref64(x[unit], gamma, beta, 1e-6)
    assert float((a - b).abs().max()) < 2e-5 * float(a.abs().max())
    tiny = fam.family_masks(names)["tiny"]
    a, _, _ = fam.ln_ref64(x[tiny], gamma, beta, 1e-5)
    b, _, _ = fam.ln_ref64(x[tiny], gamma, beta, 1e-6)
    assert float((a - b).abs().max()) > 1e-2 * float(a.abs().max())


def test_logit_rows():
    K = 10
    tgt = torch.arange(16) % K
    x, names = fam.logit_rows(16, K, torch.float32, 3)
    assert set(names) == set(fam.LOGIT_FAMILIES) and bool(torch.isfinite(x).all())
    m = {f: torch.tensor([n == f for n in names]) for f in fam.LOGIT_FAMILIES}
    assert bool((x[m["equal"]].amax(1) == x[m["equal"]].amin(1)).all())
    assert float(x[m["offset1000"]].min()) > 950.0
    top2 = x[m["dominant"]].double().topk(2, 1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) >= 80.0
    assert float(x[m["spread40"]].abs().max()) <= 40.0 and float(x[m["spread40"]].abs().max()) > 20.0
    xi, _ = fam.logit_rows(16, K, torch.bfloat16, 3, keep=tgt)
    assert bool(torch.isfinite(xi[torch.arange(16), tgt]).all()) and bool(torch.isinf(xi).any())
    assert bool(torch.isfinite(xi[m["equal"]]).all())
    # an all-equal row: log K and the exact softmax
    ce = torch.nn.functional.cross_entropy(x[m["equal"]].double(), tgt[m["equal"]], reduction="none")
    assert float((ce - math.log(K)).abs().max()) < 1e-12
