"""GPU: the low-latency switch on the model (MainModel.low_latency -> sdpnet_hip.low_latency ->
gemm_splitk) and sdpnet_engine.GraphedForward, on the small golden configurations.

Off (the default) nothing may change: no call reaches gemm_splitk.  On, bf16 GEMMs that
gemm_split_plan takes run on the split-K kernel -- the same rounding points as the default path,
another fp32 summation order -- fp32 forwards stay bit-identical, and the logits do not depend on
how the batch is cut into sub-batch streams (the K-slices are a function of (N, K) alone)."""
import statistics

import numpy as np
import pytest
import torch

import golden_util as gu
import sdpnet_engine
import sdpnet_hip as sp
import sdpnet_oracle as orc
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
BF16_TOL = 1e-2
SMALL = "s_c256_h2"    # embedding_dim 256, two blocks, 112-px images
CASES = [SMALL, "m_cf_b2"]

_MODELS = {}


def get_model(name):
    """(model on the GPU in eval mode, meta, arrays, images, state dict) of a golden case; one cached."""
    if name not in _MODELS:
        import model as ours
        meta, arr = gu.load_case(name)
        torch.manual_seed(0)
        m = ours.MainModel.from_dict(**meta["config"])
        sd, x = gu.build_inputs(meta, m)
        m.load_state_dict(sd)
        m = m.to(DEV).eval()
        _MODELS.clear()
        _MODELS[name] = (m, meta, arr, x, sd)
    m = _MODELS[name][0]
    m.low_latency = None
    m.num_streams = None
    return _MODELS[name]


@pytest.fixture
def splitk_calls(monkeypatch):
    calls = []
    real = sp.gemm_splitk

    def counted(x, w, y, M, N, K, bm, splits, **kw):
        calls.append((M, N, K, bm, splits))
        return real(x, w, y, M, N, K, bm, splits, **kw)
    monkeypatch.setattr(sp, "gemm_splitk", counted)
    return calls


@pytest.mark.parametrize("name", CASES)
def test_routing_and_golden_tolerance(name, splitk_calls):
    m, meta, arr, x, _ = get_model(name)
    xb = x.to(DEV).to(BF)
    y_off = m(xb, num_registers=meta["num_registers"])
    assert splitk_calls == []                         # unset: today's kernels, all of them
    m.low_latency = False
    with sp.low_latency():                            # the model's own setting wins over an outer block
        m(xb, num_registers=meta["num_registers"])
    assert splitk_calls == []
    m.low_latency = True
    y_on = m(xb, num_registers=meta["num_registers"])
    assert len(splitk_calls) >= 1                     # (fails without the feature)
    assert not sp.low_latency_enabled()               # the switch does not leak out of the forward
    for M, N, K, bm, splits in splitk_calls:
        assert sp.gemm_split_plan(M, N, K, sp._cus(torch.device(DEV, torch.cuda.current_device()))) == (bm, splits)
    assert y_on.dtype == BF
    err_on = np.abs(y_on.float().cpu().numpy() - arr["logits"]).max()
    err_off = np.abs(y_off.float().cpu().numpy() - arr["logits"]).max()
    print(f"LOWLAT {name}: bf16 max|err| vs golden  off {err_off:.3e}  on {err_on:.3e}  "
          f"({len(splitk_calls)} split-K GEMMs)")
    assert err_on <= BF16_TOL, f"{name}: low-latency bf16 logits max abs err {err_on:.3e}"


def test_environment_variable_is_the_default(splitk_calls, monkeypatch):
    m, meta, _, x, _ = get_model(SMALL)
    xb = x.to(DEV).to(BF)
    monkeypatch.setenv("SDPNET_LOW_LATENCY", "1")
    m(xb)
    n = len(splitk_calls)
    assert n >= 1
    monkeypatch.setenv("SDPNET_LOW_LATENCY", "0")
    m(xb)
    assert len(splitk_calls) == n
    m.train()                                         # train mode never looks at the switch
    try:
        m.low_latency = True
        m(xb.float())
    finally:
        m.eval()
    assert len(splitk_calls) == n


def test_error_against_the_oracle_is_the_default_paths():
    """Both paths round to bf16 at the same points and differ in fp32 summation order only, so their
    errors against the fp32 oracle are draws of one distribution.  Five input seeds: the allowed
    ratio of the mean errors is 1 + 2 s, s the default path's own seed-to-seed spread (standard
    deviation over mean of its five errors) -- what one more draw of the default path itself may
    differ from its mean by, twice over.  Measured values: profiles/low_latency.md."""
    m, meta, _, _, sd = get_model(SMALL)
    cfg = meta["config"]
    off, on = [], []
    for seed in range(5):
        x = synth.synth_images(100 + seed, meta["batch"], meta["image"])
        ref = orc.forward(x, sd, cfg).float().numpy()
        xb = x.to(DEV).to(BF)
        m.low_latency = False
        off.append(float(np.abs(m(xb).float().cpu().numpy() - ref).max()))
        m.low_latency = True
        on.append(float(np.abs(m(xb).float().cpu().numpy() - ref).max()))
    m.low_latency = None
    s = statistics.stdev(off) / statistics.mean(off)
    ratio = statistics.mean(on) / statistics.mean(off)
    print("LOWLAT oracle errors off " + " ".join(f"{e:.3e}" for e in off))
    print("LOWLAT oracle errors on  " + " ".join(f"{e:.3e}" for e in on))
    print(f"LOWLAT mean ratio on/off {ratio:.3f}, default-path spread s {s:.3f}, allowed {1 + 2 * s:.3f}")
    assert max(on) <= BF16_TOL
    assert ratio <= 1 + 2 * s, (ratio, s, off, on)


@pytest.mark.parametrize("name", CASES)
def test_fp32_is_never_routed(name, splitk_calls):
    m, meta, _, x, _ = get_model(name)
    xd = x.to(DEV)
    y_off = m(xd, num_registers=meta["num_registers"])
    m.low_latency = True
    y_on = m(xd, num_registers=meta["num_registers"])
    assert splitk_calls == []
    assert y_on.dtype == torch.float32 and torch.equal(y_on, y_off)


def test_two_streams_equal_one(splitk_calls):
    """B = 64 on 64-px images (a 4 x 4 patch grid, the smallest the suite runs these kernels on),
    SdP-Net-XXS: one stream of 64 images against two of 32.  Every planned GEMM has its K-slices
    from (N, K) alone and its workspace from the allocator of the stream it runs on."""
    import model as ours
    meta, _ = gu.load_case("xxs_cf_b4")
    torch.manual_seed(0)
    m = ours.MainModel.from_dict(**meta["config"])
    m.load_state_dict(synth.synth_state_dict(m, meta["wseed"]))
    m = m.to(DEV).eval()
    m.low_latency = True
    x = synth.synth_images(7, 64, 64).to(DEV).to(BF)
    m.num_streams = 1
    y1 = m(x)
    n1 = len(splitk_calls)
    m.num_streams = 2
    y2 = m(x)
    assert n1 >= 1 and len(splitk_calls) == 3 * n1    # the same GEMMs, once per stream
    assert torch.isfinite(y1.float()).all()
    assert torch.equal(y1, y2)
    y2b = m(x)                                        # and again: streams reuse each other's workspaces
    assert torch.equal(y2b, y2)


def test_graphed_forward_replays_the_eager_forward(splitk_calls):
    m, meta, _, x, _ = get_model(SMALL)
    m.low_latency = True
    xa = x.to(DEV).to(BF)
    xb = synth.synth_images(11, meta["batch"], meta["image"]).to(DEV).to(BF)
    gf = sdpnet_engine.GraphedForward(m, xa, num_registers=meta["num_registers"])
    assert len(splitk_calls) >= 1                     # what was captured is the low-latency forward
    for xi in (xa, xb):
        ya = gf(xi).clone()
        assert torch.equal(ya, m(xi, num_registers=meta["num_registers"]))
    assert gf.captures == 1
    assert gf(xb) is gf(xa)                           # the static logits, overwritten by every call
    ya = gf(xa).clone()

    # a write torch's version counters do not show + invalidate(): the next call re-captures
    p = [mod for mod in m.output_head.modules() if isinstance(mod, torch.nn.Linear)][-1].weight
    try:
        p.data.mul_(1.5)
        sdpnet_engine.invalidate(m)
        want = m(xa, num_registers=meta["num_registers"])
        got = gf(xa)
        assert gf.captures == 2
        assert torch.equal(got, want)
        assert not torch.equal(got, ya)               # (the change is visible in the logits at all)
    finally:
        p.data.div_(1.5)
        sdpnet_engine.invalidate(m)

    for bad in (xa[:1], xa.float(), xa[:, :, :-16]):
        with pytest.raises(ValueError):
            gf(bad)


def test_graphed_forward_follows_a_fused_optimizer_step():
    import copy
    import sdpnet_train
    m0, meta, _, x, _ = get_model(SMALL)
    m = copy.deepcopy(m0)
    m.low_latency = True
    xa = x.to(DEV).to(BF)
    gf = sdpnet_engine.GraphedForward(m, xa, num_registers=meta["num_registers"])
    before = gf(xa).clone()
    opt = sdpnet_train.AdamW(m.parameters(), lr=1e-2, weight_decay=0.0)
    g = torch.Generator(device="cpu").manual_seed(3)
    for p in m.parameters():
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    opt.step()
    got = gf(xa)
    assert gf.captures == 2
    assert torch.equal(got, m(xa, num_registers=meta["num_registers"]))
    assert not torch.equal(got, before)


def test_torch_compile_reaches_the_split_k_kernel(splitk_calls):
    m, meta, _, x, _ = get_model(SMALL)
    xb = x.to(DEV).to(BF)
    m.low_latency = True
    want = m(xb)
    n = len(splitk_calls)
    assert n >= 1
    cm = torch.compile(m, fullgraph=True)
    got = cm(xb)
    assert len(splitk_calls) == 2 * n                 # the compiled forward took the same route
    assert torch.equal(got, want)
    m.low_latency = False                             # and the setting is read per call, compiled too
    off = cm(xb)
    assert len(splitk_calls) == 2 * n
    m.low_latency = None
    assert torch.equal(off, m(xb))
