"""The plan of the training forward (sdpnet_train._plan) and its three drivers, on the CPU.

The eager forward (train_forward), the whole-model tape (tape_forward) and the per-layer ops'
body (layer_forward) all walk the same plan.  Here the four sub-layer Functions' forwards are
replaced by recording stubs, so no kernel runs: what is compared is which Function is called on
which module, with which geometry, dtype, parameters and seed, in which order.
"""
import pytest
import torch

import model as ours
import sdpnet_train as st
from test_compile import XXS

KINDS = {st._EmbedFn: "embed", st._MixerFn: "mixer", st._EncoderFn: "enc", st._HeadFn: "head"}


def _model(**kw):
    cfg = dict(XXS)
    cfg.update(kw)
    return ours.MainModel(**cfg).train()


def _ids(params):
    return [None if p is None else id(p) for p in params]


@pytest.mark.parametrize("conv_embedding", [False, True])
@pytest.mark.parametrize("conv_first", [True, False])
def test_plan_facts(conv_first, conv_embedding):
    m = _model(conv_first=conv_first, conv_embedding=conv_embedding)
    plan = st._plan(m, (2, 3, 64, 64), 3, torch.bfloat16)
    # geometry: 64 / 16 = 4 x 4 patches, registers [:3 + 1] -> 4 rows, 20 token rows of width 64
    assert (plan.B, plan.R, plan.Hp, plan.Wp, plan.N, plan.C) == (2, 4, 4, 4, 20, 64)
    assert plan.dt == torch.bfloat16 and plan.sdt == torch.float32  # fp32 residual stream
    assert st._plan(m, (2, 3, 64, 64), 3, torch.float32).sdt == torch.float32
    assert st._plan(m, (5, 3, 32, 48), 0, torch.float32)[:6] == (5, 1, 2, 3, 7, 64)

    steps = plan.steps
    nmix = len(m.blocks[0].conv_blocks)
    assert len(steps) == 1 + len(m.blocks) * (nmix + 1) + 2
    block = ["mixer"] * nmix + ["enc"] if conv_first else ["enc"] + ["mixer"] * nmix
    assert [s.kind for s in steps] == ["embed"] + block * len(m.blocks) + ["enc", "head"]
    assert [(s.kind, s.mod) for s in steps] == st.train_layers(m)
    mods = [m] + [x for blk in m.blocks
                  for x in ([*blk.conv_blocks, blk.t_block] if conv_first else [blk.t_block, *blk.conv_blocks])]
    assert [s.mod for s in steps] == mods + [m.final_block.t_block, m.output_head]
    for s in steps:
        assert KINDS[s.fn] == s.kind
        assert s.rng == (s.kind in ("enc", "head")) and s.lead == (5 if s.rng else 4)
        assert _ids(s.params) == _ids(st.layer_params(m, s.kind, s.mod))
        assert s.geo == {"embed": (2, 4, 4, 4, 3, torch.float32), "mixer": (2, 4, 4, 4), "enc": (2, 20),
                         "head": (2, 4, 16, 20, 64)}[s.kind]

    # every parameter of the model is an input of exactly one step
    seen = [i for s in steps for i in _ids(s.params) if i is not None]
    assert len(seen) == len(set(seen))
    assert set(seen) == {id(p) for p in m.parameters()}

    # the parameter lists keep their Nones where the Functions unpack them
    for s in steps:
        if s.kind == "enc":
            assert _ids(s.params) == _ids(st._enc_params(s.mod)) and len(s.params) == 16
        if s.kind == "head":
            assert _ids(s.params) == _ids(st._head_params(s.mod)) and len(s.params) == 6
    eh_ew = steps[0].params[1:3]
    assert all(p is None for p in eh_ew) if conv_embedding else all(p is not None for p in eh_ew)


def test_plan_none_pattern_without_qk_norm_and_with_simple_head():
    m = _model(normalize_qv=False, simple_mlp_output=True)
    steps = st._plan(m, (1, 3, 64, 64), 3, torch.float32).steps
    for s in steps:
        if s.kind == "enc":
            assert [p is None for p in s.params] == [False] * 5 + [True] * 4 + [False] * 7
    assert [p is None for p in steps[-1].params] == [False, False, False, True, True, True]  # bias=False head
    seen = [i for s in steps for i in _ids(s.params) if i is not None]
    assert len(seen) == len(set(seen)) and set(seen) == {id(p) for p in m.parameters()}


def test_plan_refuses_a_grid_larger_than_the_table():
    m = _model()  # max_image_size [14, 14]
    st._plan(m, (1, 3, 14 * 16, 14 * 16), 3, torch.float32)
    with pytest.raises(RuntimeError, match=r"image grid 15x14 exceeds max_image_size \[14, 14\]"):
        st._plan(m, (1, 3, 15 * 16, 14 * 16), 3, torch.float32)
    with pytest.raises(RuntimeError, match=r"image grid 14x15 exceeds max_image_size \[14, 14\]"):
        st._plan(m, (1, 3, 14 * 16, 15 * 16), 3, torch.float32)
    for drive in (lambda: st.tape_forward(m, torch.zeros(1, 3, 240, 224), 3, torch.float32),
                  lambda: st.layer_forward(m, 0, torch.zeros(1, 3, 240, 224), 3, torch.float32)):
        with pytest.raises(RuntimeError, match="exceeds max_image_size"):
            drive()
    assert m._sdp_session is None


# ------------------------------------------------------------------ the three drivers
def _stub(monkeypatch, log, ncls, fail_at=None, wprep=None):
    """Replace the four Functions' forwards by stubs that log their call and return a tensor of
    the real forward's shape and dtype."""
    def make(fn, kind):
        def forward(ctx, tok, geo, mod, dt, *rest):
            if len(log) == fail_at:
                raise ValueError("stub failure")
            assert st._WPREP is wprep  # the prepared weights are valid inside every step
            rng, params = (rest[0], rest[1:]) if kind in ("enc", "head") else (None, rest)
            log.append((kind, id(mod), geo, dt, tok.dtype, tuple(tok.shape), _ids(params),
                        None if rng is None else rng.next()))
            if kind == "embed":
                B, R, Hp, Wp, _, sdt = geo
                return torch.zeros(B * (R + Hp * Wp), params[0].shape[0], dtype=sdt)
            if kind == "head":
                return torch.zeros(geo[0], ncls, dtype=dt)
            return torch.zeros_like(tok)
        monkeypatch.setattr(fn, "forward", staticmethod(forward))
    for fn, kind in KINDS.items():
        make(fn, kind)


def _drive(m, how, x, dt):
    if how == "tape":
        logits, tape = st.tape_forward(m, x, 3, dt)
        assert len(tape) == len(st.train_layers(m))
        return logits
    if how == "eager":
        return st.train_forward(m, x, 3)
    t = x
    for i in range(len(st.train_layers(m))):
        assert (m.__dict__.get("_sdp_session") is None) == (i == 0)
        t, _ = st.layer_forward(m, i, t, 3, dt)
    return t


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("conv_first", [True, False])
def test_drivers_make_the_same_calls(conv_first, dt, monkeypatch):
    m = _model(conv_first=conv_first, ffn_dropout=0.2, attn_dropout=0.2)
    monkeypatch.setattr(st, "compute_dtype", lambda x, module: dt)
    x = torch.zeros(2, 3, 64, 64, dtype=dt)  # already in dt: no cast kernel
    logs = {}
    for how in ("tape", "layer", "eager"):
        log = logs[how] = []
        _stub(monkeypatch, log, 10)
        torch.manual_seed(11)
        out = _drive(m, how, x, dt)
        assert tuple(out.shape) == (2, 10) and out.dtype == dt
        assert m.__dict__.get("_sdp_session") is None and st._WPREP is None
        assert torch.randint(0, 2 ** 62, (1,)).item() == _next_draw_after_one(11)  # one draw per forward
    assert len(logs["tape"]) == 9
    assert logs["tape"] == logs["layer"] == logs["eager"]
    assert [c[0] for c in logs["tape"]] == [k for k, _ in st.train_layers(m)]
    assert [c[1] for c in logs["tape"]] == [id(mod) for _, mod in st.train_layers(m)]
    seeds = [c[7] for c in logs["tape"] if c[7] is not None]
    assert len(seeds) == 4 and len(set(seeds)) == 4  # one rng shared by the encoders and the head


def _next_draw_after_one(seed):
    g = torch.Generator().manual_seed(seed)
    torch.randint(0, 2 ** 62, (1,), generator=g)
    return torch.randint(0, 2 ** 62, (1,), generator=g).item()


@pytest.mark.parametrize("how", ["tape", "layer", "eager"])
def test_a_failing_middle_layer_closes_the_session_and_clears_the_weights(how, monkeypatch):
    m = _model()
    bufs = {}
    monkeypatch.setattr(st, "compute_dtype", lambda x, module: torch.float32)
    monkeypatch.setattr(st, "_prep_weights", lambda model, dt: bufs)
    log = []
    _stub(monkeypatch, log, 10, fail_at=4, wprep=bufs)
    with pytest.raises(ValueError, match="stub failure"):
        _drive(m, how, torch.zeros(2, 3, 64, 64), torch.float32)
    assert len(log) == 4
    assert m.__dict__.get("_sdp_session") is None and st._WPREP is None
    if how == "layer":  # the forward is over: a later layer op has no session to run in
        with pytest.raises(RuntimeError, match="training layer op run outside a forward"):
            st.layer_forward(m, 5, torch.zeros(40, 64), 3, torch.float32)
