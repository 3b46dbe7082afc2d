"""GPU: the MXFP8 switch on the model (MainModel.mx_fp8 -> sdpnet_hip.mx_fp8 -> layers._mlp_mx ->
mx_quant_rows / gemm_mx), on the small golden configurations; pattern of test_gpu_low_latency.py.

Off (the default) nothing may change: no call reaches the MX kernels and the logits are bit-equal
to those of a model object that never had the attribute.  On, the MLP pairs of ConvMixer and
EncoderLayer run block-scaled; accuracy is judged against references, not against the code under
test: err_hip^2 <= (1.25 err_emul)^2 + err_bf16^2 on the rms logit errors against the fp64 oracle
(err_emul: tests/mx_oracle.py's fp64 MX forward; measured values: profiles/mx_fp8.md)."""
import copy
import statistics

import pytest
import torch

import golden_util as gu
import mx_oracle as mo
import sdpnet_engine
import sdpnet_hip as sp
import synth
from test_gpu_low_latency import get_model as _get_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
SMALL = "s_c256_h2"
CASES = [SMALL, "m_cf_b2"]


def get_model(name):
    out = _get_model(name)
    out[0].__dict__.pop("mx_fp8", None)
    return out


@pytest.fixture
def mx_calls(monkeypatch):
    calls = {"gemm": [], "quant": []}
    real_g, real_q = sp.gemm_mx, sp.mx_quant_rows

    def gemm(x, w, M, N, K, **kw):
        calls["gemm"].append((M, N, K, kw.get("out_mx") is not None))
        return real_g(x, w, M, N, K, **kw)

    def quant(x, M, K, **kw):
        calls["quant"].append((M, K, kw.get("stats") is not None))
        return real_q(x, M, K, **kw)
    monkeypatch.setattr(sp, "gemm_mx", gemm)
    monkeypatch.setattr(sp, "mx_quant_rows", quant)
    return calls


def rms(a, b):
    return float((a.double().cpu() - b.double().cpu()).pow(2).mean().sqrt())


@pytest.mark.parametrize("name", CASES)
def test_routing(name, mx_calls):
    m, meta, arr, x, _ = get_model(name)
    nr = meta["num_registers"]
    xb = x.to(DEV).to(BF)
    assert not hasattr(m, "mx_fp8")
    y_never = m(xb, num_registers=nr)                 # before the attribute ever existed on the object
    assert mx_calls == {"gemm": [], "quant": []}      # unset: today's kernels, all of them
    m.mx_fp8 = False
    with sp.mx_fp8():                                 # the model's own setting wins over an outer block
        y_false = m(xb, num_registers=nr)
    assert mx_calls == {"gemm": [], "quant": []}
    m.mx_fp8 = True
    y_on = m(xb, num_registers=nr)
    assert len(mx_calls["gemm"]) >= 2 and len(mx_calls["quant"]) >= 1     # (fails without the feature)
    assert not sp.mx_fp8_enabled()                    # the switch does not leak out of the forward
    ups = [c for c in mx_calls["gemm"] if c[3]]
    assert len(ups) * 2 == len(mx_calls["gemm"])      # pairs: MX hidden out, then bf16 out
    assert any(q[2] for q in mx_calls["quant"])       # the stream rows go in with their LN statistics
    m.mx_fp8 = None
    y_none = m(xb, num_registers=nr)
    assert torch.equal(y_never, y_false) and torch.equal(y_never, y_none)
    assert y_on.dtype == BF and torch.isfinite(y_on.float()).all() and not torch.equal(y_on, y_never)


def test_environment_variable_is_the_default_and_train_fp32_are_never_routed(mx_calls, monkeypatch):
    m, meta, _, x, _ = get_model(SMALL)
    xb = x.to(DEV).to(BF)
    monkeypatch.setenv("SDPNET_MX_FP8", "1")
    m(xb)
    n = len(mx_calls["gemm"])
    assert n >= 2
    monkeypatch.setenv("SDPNET_MX_FP8", "0")
    m(xb)
    assert len(mx_calls["gemm"]) == n
    monkeypatch.delenv("SDPNET_MX_FP8")
    m.mx_fp8 = True
    m.train()                                         # train mode never looks at the switch
    try:
        m(xb.float())
    finally:
        m.eval()
    assert len(mx_calls["gemm"]) == n
    xd = x.to(DEV)                                    # fp32: never routed, bit-equal on / off
    y_on = m(xd)
    m.mx_fp8 = False
    y_off = m(xd)
    assert len(mx_calls["gemm"]) == n
    assert y_on.dtype == torch.float32 and torch.equal(y_on, y_off)


@pytest.mark.parametrize("name", CASES)
def test_accuracy_against_the_fp64_references(name):
    """err_hip, err_bf16: rms logit error of the MX / default HIP forward against the fp64 oracle;
    err_emul: that of the fp64 MX emulation.  Kernel and emulation MX noise are draws of one
    distribution (seed spread ~0.02), the bf16 noise of the untouched layers adds in quadrature;
    1.25 lies between that spread and the >= 1.5 x of a truncating quantiser (test_mx_host.py)."""
    m, meta, _, x0, sd = get_model(name)
    cfg, nr = meta["config"], meta["num_registers"]
    seeds = [None] if name != SMALL else [100 + i for i in range(5)]
    hip, bf, emul = [], [], []
    for seed in seeds:
        x = x0 if seed is None else synth.synth_images(seed, meta["batch"], meta["image"])
        ref = mo.forward_mx(x, sd, cfg, nr, None, None)
        emul.append(rms(mo.forward_mx(x, sd, cfg, nr), ref))
        xb = x.to(DEV).to(BF)
        m.mx_fp8 = False
        bf.append(rms(m(xb, num_registers=nr), ref))
        m.mx_fp8 = True
        hip.append(rms(m(xb, num_registers=nr), ref))
    m.mx_fp8 = None
    eh, eb, ee = (statistics.mean(v) for v in (hip, bf, emul))
    print(f"MXMODEL {name}: err_hip {eh:.4e}  err_bf16 {eb:.4e}  err_emul {ee:.4e}  "
          f"bound {((1.25 * ee) ** 2 + eb ** 2) ** 0.5:.4e}  (seeds {len(seeds)})")
    assert eh ** 2 <= (1.25 * ee) ** 2 + eb ** 2, (eh, eb, ee)


def test_two_streams_equal_one(mx_calls):
    import model as ours
    meta, _ = gu.load_case("xxs_cf_b4")
    torch.manual_seed(0)
    m = ours.MainModel.from_dict(**meta["config"])
    m.load_state_dict(synth.synth_state_dict(m, meta["wseed"]))
    m = m.to(DEV).eval()
    m.mx_fp8 = True
    x = synth.synth_images(7, 64, 64).to(DEV).to(BF)
    m.num_streams = 1
    y1 = m(x)
    n1 = len(mx_calls["gemm"])
    m.num_streams = 2
    y2 = m(x)
    assert n1 >= 2 and len(mx_calls["gemm"]) == 3 * n1
    assert torch.isfinite(y1.float()).all() and torch.equal(y1, y2)


def test_graphed_forward_replays_the_eager_forward_and_recaptures_on_the_switch(mx_calls):
    m, meta, _, x, _ = get_model(SMALL)
    nr = meta["num_registers"]
    m.mx_fp8 = True
    xa = x.to(DEV).to(BF)
    xb = synth.synth_images(11, meta["batch"], meta["image"]).to(DEV).to(BF)
    gf = sdpnet_engine.GraphedForward(m, xa, num_registers=nr)
    assert len(mx_calls["gemm"]) >= 2                 # what was captured is the MX forward
    for xi in (xa, xb):
        assert torch.equal(gf(xi).clone(), m(xi, num_registers=nr))
    assert gf.captures == 1
    m.mx_fp8 = False                                  # the setting changed: captured again
    got = gf(xa).clone()
    assert gf.captures == 2 and torch.equal(got, m(xa, num_registers=nr))
    m.mx_fp8 = None


def test_mx_weights_follow_a_fused_optimizer_step():
    """After one fused AdamW.step() the MX forward equals, bit for bit, that of a never-run twin
    loaded with the stepped weights: the cached MX weight copies were rebuilt."""
    import sdpnet_train
    m0, meta, _, x, _ = get_model(SMALL)
    nr = meta["num_registers"]
    m = copy.deepcopy(m0)
    m.mx_fp8 = True
    xa = x.to(DEV).to(BF)
    before = m(xa, num_registers=nr)
    opt = sdpnet_train.AdamW(m.parameters(), lr=1e-2, weight_decay=0.0)
    g = torch.Generator(device="cpu").manual_seed(3)
    for p in m.parameters():
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    opt.step()
    got = m(xa, num_registers=nr)
    import model as ours
    torch.manual_seed(0)
    twin = ours.MainModel.from_dict(**meta["config"])
    twin.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    twin = twin.to(DEV).eval()
    twin.mx_fp8 = True
    assert torch.equal(got, twin(xa, num_registers=nr))
    assert not torch.equal(got, before)


def test_ineligible_width_keeps_the_default_path(mx_calls):
    """embedding_dim 96 (K % 128 != 0): zero MX calls, bit-equal to the default."""
    import model as ours
    meta, _ = gu.load_case("s_c96_h8")
    torch.manual_seed(0)
    m = ours.MainModel.from_dict(**meta["config"])
    sd, x = gu.build_inputs(meta, m)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    xb = x.to(DEV).to(BF)
    y_off = m(xb, num_registers=meta["num_registers"])
    m.mx_fp8 = True
    y_on = m(xb, num_registers=meta["num_registers"])
    assert mx_calls == {"gemm": [], "quant": []}
    assert torch.equal(y_on, y_off)
