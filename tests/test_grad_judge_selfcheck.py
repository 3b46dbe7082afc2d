"""CPU self-check of tests/grad_judge.py: the per-tensor gradient rules judged on the oracle itself.

The fp64 oracle is the reference, the fp32 oracle the candidate, on the ``train_cf`` gradient
fixture's inputs and on the ``s_base`` forward fixture's.  (i) the fp32 oracle passes the fp32
rule; (ii) an all-zero conv-block LayerNorm gradient fails it -- and passes the model-wide-floor
expression the rule replaces, copied below as it stood in tests/test_train.py; (iii) one
q_proj.weight gradient scaled by 1.01 fails; (iv) the CPU-autocast-bf16 gradients fail.
"""
import json
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import grad_judge as gj
import synth


def _inputs(name):
    import model as ours
    if name.startswith("train_"):
        meta, arr = gu.load_case(name)
        y = torch.from_numpy(arr["labels"])
        xseed = meta["xseed"]
    else:
        meta = json.load(open(os.path.join(gu.GOLDEN, "MANIFEST.json")))[name]
        y = torch.arange(meta["batch"]) % 7
        xseed = meta["xseed"]
    cfg = dict(meta["config"], ffn_dropout=0.0, attn_dropout=0.0)
    torch.manual_seed(0)
    m = ours.MainModel.from_dict(**cfg)
    sd = synth.synth_state_dict(m, meta["wseed"])
    x = synth.synth_images(xseed, meta["batch"], meta["image"])
    names = [k for k, _ in m.named_parameters()]
    return cfg, sd, x, y, meta["num_registers"], names


_CACHE = {}


def _grads(name):
    """(cfg, parameter names, fp64 / fp32 / CPU-autocast oracle gradients), computed once per case."""
    if name not in _CACHE:
        cfg, sd, x, y, nreg, names = _inputs(name)
        g = {}
        for key, kw in (("f64", dict(dtype=torch.float64)), ("f32", dict()), ("ac", dict(autocast=True))):
            _, g[key] = gj.oracle_grads(cfg, sd, x, y, nreg, **kw)
            assert set(names) <= set(g[key]), key
        _CACHE[name] = (cfg, names, g)
    return _CACHE[name]


# the expression being replaced (tests/test_train.py before this rule): error over
# max(|ref|max, 1e-3 * the model's largest gradient)
def _old_rel(got, ref, floor=0.0):
    return float(np.abs(got - ref).max()) / max(1e-12, float(np.abs(ref).max()), floor)


def _old_floor(ref, names):
    return 1e-3 * max(float(np.abs(ref[k]).max()) for k in names)


def _old_fp32_passes(got, ref, names):
    fl = _old_floor(ref, names)
    return all(_old_rel(got[k], ref[k], fl) <= 1e-4 for k in names)


CASES = ["train_cf", "s_base"]


@pytest.mark.parametrize("name", CASES)
def test_fp32_oracle_passes_the_fp32_rule(name):
    cfg, names, g = _grads(name)
    rows, exempt = gj.fp32_report(g["f32"], g["f64"], names)
    print(name, "worst", [(k, f"{r:.2e}") for r, _, _, k in rows[:3]], "smallest tensor / largest",
          min(gj.amax(g["f64"][k]) for k in names if not k.endswith(gj.EXEMPT_SUFFIX))
          / max(gj.amax(g["f64"][k]) for k in names))
    assert len(exempt) == gj.qv_layers(cfg) == 3
    gj.assert_fp32(g["f32"], g["f64"], gj.qv_layers(cfg), names, name)
    # the exemption is needed and is the only one: the exact gradient of k_norm.bias is zero
    for k in exempt:
        assert gj.amax(g["f64"][k]) <= 1e-12 * max(gj.amax(g["f64"][n]) for n in names), k


@pytest.mark.parametrize("name", CASES)
def test_zeroed_layernorm_gradient_fails_the_rule_and_passed_the_old_floor(name):
    cfg, names, g = _grads(name)
    ln = [k for k in names if "conv_blocks." in k and k.endswith("layer_norm_1.gamma")]
    assert ln
    victim = min(ln, key=lambda k: gj.amax(g["f64"][k]))
    bad = dict(g["f32"])
    bad[victim] = np.zeros_like(bad[victim])
    fails = gj.fp32_failures(bad, g["f64"], gj.qv_layers(cfg), names)
    assert [k for *_, k in fails] == [victim]
    assert fails[0][0] >= 0.99 / gj.FP32_TOL  # the error is the whole tensor
    assert _old_fp32_passes(g["f32"], g["f64"], names)
    # the replaced expression: the floor turns this 100 % error into ...
    fl = _old_floor(g["f64"], names)
    old = _old_rel(bad[victim], g["f64"][victim], fl)
    rac = _old_rel(g["ac"][victim], g["f64"][victim], fl)
    print(name, victim, "old floor expression judges the zeroed tensor at", old)
    if name == "train_cf":
        # ... 2e-5 where the tensor is 2e-8 of the head weight's gradient: it passed the old fp32 test
        assert _old_fp32_passes(bad, g["f64"], names), "the replaced floor rule should have let this through"
    else:
        # ... 3e-4 on s_base (the tensor is 3e-7 of the largest): over the old fp32 1e-4, still 3000x understated
        assert old <= 1e-3
    assert old <= 2 * rac + 4e-2  # and it passed the old bf16 budget on both


@pytest.mark.parametrize("name", CASES)
def test_one_percent_scale_error_fails_the_rule(name):
    cfg, names, g = _grads(name)
    victim = [k for k in names if k.endswith("q_proj.weight")][0]
    bad = dict(g["f32"])
    bad[victim] = bad[victim] * 1.01
    fails = gj.fp32_failures(bad, g["f64"], gj.qv_layers(cfg), names)
    assert [k for *_, k in fails] == [victim]


@pytest.mark.parametrize("name", CASES)
def test_autocast_gradients_fail_the_fp32_rule_and_pass_the_bf16_rule_against_themselves(name):
    cfg, names, g = _grads(name)
    fails = gj.fp32_failures(g["ac"], g["f64"], gj.qv_layers(cfg), names)
    assert len(fails) >= len(names) // 2, (len(fails), len(names))
    # bf16 rule: autocast judged against itself sits at 1 / 4 of the budget, a 5x error misses it
    rows = gj.bf16_report(g["ac"], g["f64"], g["ac"], names)
    assert all(abs(r - 1.0 / gj.BF16_FACTOR) < 1e-12 for r, *_ in rows)
    far = {k: g["f64"][k] + 5.0 * (g["ac"][k] - g["f64"][k]) for k in names}
    assert len(gj.bf16_failures(far, g["f64"], g["ac"], names)) == len(names)
    assert not gj.bf16_failures(g["f32"], g["f64"], g["ac"], names)


def test_statistical_form_thresholds():
    ok = {"a": [(1.4, 1.0)] * 8, "b": [(0.5, 1.0)] * 5 + [(2.0, 1.0)] * 3}
    assert gj.statistical(ok) == []
    bad = gj.statistical({"median": [(1.6, 1.0)] * 8, "mean": [(1.0, 1.0)] * 7 + [(10.0, 1.0)]})
    assert sorted(k for *_, k in bad) == ["mean", "median"]
