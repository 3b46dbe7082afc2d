"""Alignment harness: hand a kernel an operand whose base address or row stride is off the
alignment its vector path needs, inside a guard-banded allocation, and judge what came back.

Almost every entry point of the C ABI chooses between a vector kernel (8-B / 16-B accesses,
LDS-DMA, whole-line epilogues) and an element-wise or generic one by an alignment predicate
written at the launch site.  The other kernel tests leave the vector tier only through odd
*shapes*; here the shape stays one the vector tier takes and only the address moves:

  * ``shifted(dense, byte_shift, ld)`` is a view of the logical [M, C] matrix whose
    ``data_ptr()`` is congruent to ``byte_shift`` (mod 16) and whose row stride is ``ld``.  It
    lies in one allocation filled with ``placement.SENTINEL`` (a NaN pattern): the padding
    columns, ``guard_rows`` rows before and after, and the bytes in front.  An access of any width
    a kernel here uses therefore stays inside mapped memory.
  * ``findings(view)`` names every non-sentinel element outside the logical ones (a store that
    spilled) and every non-finite logical element (a read of the guard band poisons the result:
    the sentinel is a NaN; a dropped store leaves it behind).
  * ``judge(...)`` holds a call to the contract: it returns 0 with a correct result and nothing
    else touched, or it is refused and no output byte was written.  ``TABLE`` says, per entry
    point and operand, which perturbations apply and which of them the library refuses.

No GPU call happens at import; the same code runs on CPU tensors (test_alignment_selfcheck.py),
which is the evidence that test_gpu_alignment.py can fail.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import torch

from placement import SENTINEL

BF, F32 = torch.bfloat16, torch.float32
GUARD_ROWS = 2
TAIL = 8  # sentinel elements after the last guard row


# --------------------------------------------------------------------------- the perturbations
@dataclass(frozen=True)
class Case:
    """One perturbation of one operand: its base moved by ``shift`` bytes (``"elem"``: one
    element of its type) or its row stride grown by ``delta`` elements."""
    shift: object = 0     # "elem", or bytes
    delta: int = 0

    def bytes_for(self, dtype: torch.dtype) -> int:
        return _es(dtype) if self.shift == "elem" else int(self.shift)

    @property
    def id(self) -> str:
        return f"ld+{self.delta}" if self.delta else f"base+{self.shift}"


BASE = (Case(shift="elem"), Case(shift=4), Case(shift=8))
STRIDE = (Case(delta=1), Case(delta=2), Case(delta=4))
FLAT = (Case(shift=4), Case(shift=8), Case(shift=12))   # offsets inside a flat fp32 buffer
CASES = BASE + STRIDE
ALL = "all"   # every operand moved by one element at once
# base + elem / 4 / 8 crosses every pointer test `% 4`, `% 8`, `% 16` bytes for 2-B and 4-B
# elements; ld + 1 / 2 / 4 crosses every stride test `ld % 2`, `% 4`, `% 8` elements.


def _es(dtype: torch.dtype) -> int:
    return torch.empty(0, dtype=dtype).element_size()


def applicable(case: Case, dtype: torch.dtype) -> bool:
    """A 4-B shift of an fp32 operand is its one-element shift: listed once (as "elem")."""
    return not (case.shift == 4 and _es(dtype) == 4)


# --------------------------------------------------------------------------- placing an operand
def blank(M: int, C: int, dtype: torch.dtype, device, byte_shift: int = 0, ld: Optional[int] = None,
          guard_rows: int = GUARD_ROWS) -> torch.Tensor:
    """An [M, C] view as ``shifted`` gives, the logical elements holding the sentinel too (an
    output: a store the kernel dropped shows as a non-finite element)."""
    itype, sent = SENTINEL[dtype]
    es = _es(dtype)
    ld = C if ld is None else ld
    assert M > 0 and 0 < C <= ld and byte_shift % es == 0 and 0 <= byte_shift < 16
    lead = ((byte_shift - guard_rows * ld * es) % 16) // es     # sentinel elements in front
    total = lead + (M + 2 * guard_rows) * ld + TAIL
    ibuf = torch.full((total,), sent, dtype=itype, device=device)
    assert ibuf.data_ptr() % 16 == 0
    v = torch.as_strided(ibuf.view(dtype), (M, C), (ld, 1), lead + guard_rows * ld)
    assert v.data_ptr() % 16 == byte_shift and v.stride(0) == ld
    return v


def shifted(dense: torch.Tensor, byte_shift: int, ld: Optional[int] = None,
            guard_rows: int = GUARD_ROWS) -> torch.Tensor:
    """A copy of the logical matrix ``dense`` ([M, C], or a vector [C] taken as one row) at
    ``byte_shift`` (mod 16) with row stride ``ld``, sentinel all around."""
    vec = dense.dim() == 1
    d2 = dense.reshape(1, -1) if vec else dense
    assert d2.dim() == 2
    v = blank(d2.shape[0], d2.shape[1], dense.dtype, dense.device, byte_shift, ld, 0 if vec else guard_rows)
    v.copy_(d2)
    return v[0] if vec else v


def place(dense: torch.Tensor, case: Optional[Case], ld: Optional[int] = None, out: bool = False) -> torch.Tensor:
    """``dense`` under one perturbation (None: aligned, row stride ``ld``).  ``ld`` is the
    aligned row stride (default: C); a stride case adds its delta to it."""
    vec = dense.dim() == 1
    C = dense.shape[-1]
    ld = C if ld is None else ld
    shift = case.bytes_for(dense.dtype) if case is not None else 0
    delta = case.delta if case is not None else 0
    assert not (vec and delta), "a vector has no row stride"
    if out:
        assert not vec
        return blank(dense.shape[0], C, dense.dtype, dense.device, shift, ld + delta)
    return shifted(dense, shift, None if vec else ld + delta)


# --------------------------------------------------------------------------- what was touched
def _storage_ints(view: torch.Tensor) -> torch.Tensor:
    """The whole allocation behind ``view`` as integers of its element size."""
    itype, _ = SENTINEL[view.dtype]
    st = view.untyped_storage()
    n = st.nbytes() // _es(view.dtype)
    return torch.empty(0, dtype=itype, device=view.device).set_(st, 0, (n,), (1,))


def _logical_index(view: torch.Tensor) -> torch.Tensor:
    idx = torch.full((), view.storage_offset(), dtype=torch.int64, device=view.device)
    for size, stride in zip(view.shape, view.stride()):
        idx = idx.unsqueeze(-1) + torch.arange(size, device=view.device) * stride
    return idx.reshape(-1)


def findings(view: torch.Tensor, limit: int = 4) -> List[Tuple[str, str]]:
    """(kind, message) for every non-sentinel element outside the logical elements of ``view``
    ("stray") and every non-finite logical element ("poisoned")."""
    _, sent = SENTINEL[view.dtype]
    flat, idx = _storage_ints(view), _logical_index(view)
    out: List[Tuple[str, str]] = []
    bad = (~torch.isfinite(view)).nonzero()
    if bad.numel():
        pos = tuple(bad[0].tolist())
        out.append(("poisoned", f"{bad.shape[0]} non-finite logical element(s), the first at {pos}: a read outside "
                                f"the operand (the sentinel is a NaN) or a store that never arrived"))
    saved = flat[idx].clone()
    flat[idx] = sent
    try:
        if int(flat.min()) != sent or int(flat.max()) != sent:
            first = view.storage_offset()
            ld = view.stride(0) if view.dim() == 2 else max(1, view.numel())
            for e in (flat != sent).nonzero().flatten()[:limit].tolist():
                rel = e - first
                where = (f"row {rel // ld} column {rel % ld} of the view (C = {view.shape[-1]}, ld = {ld})"
                         if rel >= 0 else f"{-rel} element(s) before the view")
                out.append(("stray", f"element {e} of the allocation written outside the operand: {where}"))
    finally:
        flat[idx] = saved
    return out


def untouched(view: torch.Tensor) -> bool:
    """Every element of the allocation, logical ones included, still holds the sentinel."""
    _, sent = SENTINEL[view.dtype]
    flat = _storage_ints(view)
    return int(flat.min()) == sent and int(flat.max()) == sent


# --------------------------------------------------------------------------- the contract
RAN, REFUSED = "ran", "refused"


def judge(what: str, refused: bool, inputs: Dict[str, Tuple[torch.Tensor, torch.Tensor]],
          outputs: Dict[str, torch.Tensor], verify: Callable[[], None], expect: Optional[str] = None,
          inouts: Optional[Dict[str, Tuple[torch.Tensor, torch.Tensor]]] = None) -> str:
    """Hold one call to the contract and return its outcome.

    ``inputs``: name -> (view handed to the kernel, the dense original); ``outputs``: name ->
    view from ``blank``; ``inouts``: name -> (view, its contents before the call) for operands
    updated in place.  ``verify`` compares the logical outputs with the reference (it raises).
      * ran (``refused`` false): no operand has a stray or poisoned element, the inputs are
        unchanged, and ``verify`` passes;
      * refused: every output allocation is all sentinel, every in-place operand and input is
        bit for bit what it was.
    ``expect`` pins which of the two the table promises."""
    inouts = inouts or {}
    errs: List[str] = []
    for name, (v, dense) in inputs.items():   # an input may hold non-finite values of its own (a -inf mask)
        errs += [f"input {name}: {m}" for k, m in findings(v) if k == "stray"]
        if not torch.equal(v.reshape(dense.shape), dense):
            errs.append(f"input {name} was modified")
    if refused:
        for name, v in outputs.items():
            if not untouched(v):
                errs.append(f"output {name} was written although the call was refused")
        for name, (v, before) in inouts.items():
            if not torch.equal(v, before) or [f for f in findings(v) if f[0] == "stray"]:
                errs.append(f"in-place operand {name} was written although the call was refused")
    else:
        for name, v in outputs.items():
            errs += [f"output {name}: {m}" for _, m in findings(v)]
        for name, (v, _) in inouts.items():
            errs += [f"in-place operand {name}: {m}" for _, m in findings(v)]
    assert not errs, f"{what}: " + "; ".join(errs)
    if not refused:
        verify()
    outcome = REFUSED if refused else RAN
    assert expect is None or outcome == expect, f"{what}: the call {outcome}, the table promises {expect}"
    return outcome


# --------------------------------------------------------------------------- what is covered
@dataclass
class Entry:
    """One row of the coverage table.  ``operands``: name -> the perturbations applied to it;
    ``refuses``: (operand, case id) pairs the library refuses (every other case must return 0; a
    one-element shift is also matched by its byte count); ``left_out``: operand -> why it is not
    perturbed."""
    name: str
    operands: Dict[str, Sequence[Case]]
    refuses: Sequence[Tuple[str, str]] = ()
    left_out: Dict[str, str] = field(default_factory=dict)
    wide: str = ""   # what the vector tier dereferences wider than one element, and its predicate

    def cases(self, dtypes: Dict[str, torch.dtype]) -> List[Tuple[str, object]]:
        """(operand, case) pairs for operands of the given types, then the all-operands case."""
        out = [(op, c) for op, cs in self.operands.items() if op in dtypes for c in cs if applicable(c, dtypes[op])]
        return out + [(ALL, Case(shift="elem"))]

    def expect(self, op: str, case: Case, dtype: Optional[torch.dtype] = None) -> str:
        ids = {case.id}
        if dtype is not None and case.shift == "elem":
            ids.add(f"base+{_es(dtype)}")    # a refusal listed by its byte count
        return REFUSED if any((op, i) in self.refuses for i in ids) else RAN


M_ = CASES            # a matrix operand: base and stride
P_ = BASE             # a pointer without a row stride of its own
LIB = "allocated by the library's own callers (sdpnet_engine / sdpnet_train workspaces), never a user tensor"
SAME = "one implementation with sdp_attention (attention_impl), where it is perturbed"

TABLE: Dict[str, Entry] = {e.name: e for e in [
    Entry("sdp_layernorm", dict(X=M_, Y=M_, gamma=P_, beta=P_),
          wide="layernorm_rows: X, Y rows as 4-element vectors, gamma / beta as f32x4; launch_ln tests X, Y, "
               "gamma, beta % 16, ldx, ldy, C % 4; otherwise layernorm_rows_scalar"),
    Entry("sdp_gemm", dict(X=M_, W=M_, Y=M_, R=M_, bias=P_),
          wide="gemm_bf16_8ph: X, W by 16-B LDS-DMA chunks; Y, R 8-B (kernel 9) or whole 16-B lines (kernel 14); "
               "bias f32x4.  gemm_impl tests each; otherwise gemm_generic (element loads, 8-B stores only "
               "where the address allows)"),
    Entry("sdp_gemm_ln", dict(X=M_, W=M_, Y=M_, R=M_, bias=P_, ln_stats=P_, ln_colsum=P_, part=P_),
          refuses=[("ln_colsum", "base+4"), ("ln_colsum", "base+8")],
          wide="as sdp_gemm; ln_stats read and part written as float2 by the fast epilogues (ln_stats % 8 sends "
               "the call to gemm_generic, which reads two floats; part % 8 leaves the partials to "
               "sdp_row_partials); ln_colsum f32x4: refused unless 16-B aligned (sdpnet_hip.h), it is the "
               "library's own fold_ln_weight output"),
    Entry("sdp_rowstats", dict(X=M_, stats=P_),
          wide="rowstats_k: X rows as 4-element vectors when X % 16 and ldx % 4 allow, element loads otherwise; "
               "stats written one float at a time"),
    Entry("sdp_row_partials", dict(X=M_, part=P_), wide="element loads; part written one float at a time"),
    Entry("sdp_ln_stats", dict(part=P_, stats=P_), wide="part read and stats written one float at a time"),
    Entry("sdp_qk_headnorm", dict(QKV=M_, gq=P_, bq=P_, gk=P_, bk=P_), wide="element accesses only"),
    Entry("sdp_dwconv", dict(X=M_, Y=M_, stats=P_, ln_gamma=P_, ln_beta=P_, weight=P_, bias=P_),
          wide="dwconv3_mfma / dwconv2_nhwc: X, Y rows by 16 B, stats as float2, bias as f32x4 (tier 2); sdp_dwconv "
               "tests each (v16, bias % 16) and falls to dwconv_ln_nhwc, whose 16-B loads, 4-element stores and "
               "f32x4 bias each have an element form chosen by launch_dw; gamma, beta, weight are element reads"),
    Entry("sdp_attention", dict(QKV=M_, O=M_, q_gamma=P_, q_beta=P_, k_gamma=P_, k_beta=P_, mask=P_),
          wide="flash kernels: QKV rows by 16 B (LDS-DMA in attn_fa4 / attn_fs), O by 8 B, q / k gamma / beta as "
               "f32x4 (frag_norm); attention_impl tests QKV % 16, ld_qkv % 8, O % 8, ld_o % 4 and the four norm "
               "vectors % 16, else qk_headnorm + attn_generic (element accesses; mask is only read there)"),
    Entry("sdp_attention_rows", dict(QKV=M_, O=M_), wide="as sdp_attention (one implementation)",
          left_out=dict(q_gamma=SAME, q_beta=SAME, k_gamma=SAME, k_beta=SAME, mask=SAME)),
    Entry("sdp_act", dict(X=P_, Y=P_), wide="element accesses only (flat array)"),
    Entry("sdp_cast", dict(X=P_, Y=P_), wide="element accesses only (flat array)"),
    Entry("sdp_copy_rows", dict(src=M_, dst=M_),
          wide="copy_rows16_k moves uint4; sdp_copy_rows tests both bases % 16 and C, both ld, both group "
               "strides in 16-B units, else broadcast_rows_k (element accesses)"),
    Entry("sdp_patchify", dict(img=P_, out=P_),
          wide="patchify_strip_k reads pixel pairs and writes column pairs (4 B / 8 B); sdp_patchify tests img "
               "and out for the pair size (p, Wi, Kpad even keep every row on it), else patchify_rows_k"),
    Entry("sdp_adamw / sdp_grad_sumsq_parts / sdp_ema_update", dict(tensors=FLAT),
          wide="adamw_k, sumsq_parts_k: element accesses; ema_k: f32x4 only when out, a, b of the tensor are all "
               "16-B aligned (tested in the kernel).  Driven through sdpnet_train.AdamW / sp.ema_update on views "
               "of flat buffers, not through sweep()"),
]}

# ---- training side and the GEMMs without a slower form (tests/test_gpu_alignment_train.py)
SIX = ("base+elem", "base+2", "base+4", "base+8", "ld+1", "ld+2", "ld+4")   # every case misaligns a 16-B row
V16 = ("base+elem", "base+4", "base+8")                                     # an fp32 vector off 16 B
ROW8 = ("base+elem", "base+2", "base+4", "ld+1", "ld+2")                     # a bf16 row off 8 B / ld % 4


def _ref(**ops):
    return [(op, cid) for op, ids in ops.items() for cid in ids]


_TRAIN = [
    Entry("sdp_act_fwd", dict(Z=M_, Y=M_), wide="act_fwd_v8: 8 elements (16 B bf16, 2 x 16 B fp32) of Z and Y; "
          "sdp_act_fwd tests Z, Y % 16, ldz, ldy, N % 8, else act_fwd_k"),
    Entry("sdp_act_bwd", dict(Z=M_, DY=M_, DZ=M_), wide="act_bwd_v8 as act_fwd_v8 on Z, DY, DZ; else act_bwd_k"),
    Entry("sdp_rowscale_add", dict(X=M_, R=M_, Y=M_, scale=P_),
          wide="rowscale_v8: 8 elements of X, R, Y (tested with their ld); scale one float per row; else rowscale_k"),
    Entry("sdp_act_rowscale_add", dict(X=M_, R=M_, Y=M_, scale=P_), wide="as sdp_rowscale_add"),
    Entry("sdp_rowscale_add_dropout", dict(X=M_, R=M_, Y=M_, scale=P_), refuses=_ref(X=SIX, R=SIX, Y=SIX),
          wide="rowscale_v8 only: hipErrorNotSupported for X, R, Y off 16-B rows (header); sdpnet_hip.rowscale_add "
               "then runs sdp_act_fwd / sdp_rowscale_add as two passes"),
    Entry("sdp_rowscale_add_mixed", dict(X=M_, R=M_, Y=M_, scale=P_), refuses=_ref(X=SIX, R=SIX, Y=SIX),
          wide="rowscale_v8 only: hipErrorInvalidValue for X, R, Y off 16-B rows (header); the operands are "
               "sdpnet_train's own activation buffers"),
    Entry("sdp_seg_colsum", dict(X=M_, out=M_), wide="seg_colsum_v4 / colsum_wide_f32: 4-element loads of X, f32x4 "
          "stores of out; tested with ldx, ldo, C % 4; else seg_colsum_k"),
    Entry("sdp_ln_apply", dict(X=M_, Y=M_, stats=P_, gamma=P_, beta=P_), wide="element accesses only"),
    Entry("sdp_ln_fwd", dict(X=M_, Y=M_, gamma=P_, beta=P_, stats=P_),
          refuses=_ref(X=SIX, Y=SIX, gamma=V16, beta=V16, stats=("base+elem", "base+4")),
          wide="ln_fwd_sm / ln_fwd_v8: 8 elements of X and Y, gamma / beta as 2 x f32x4, stats as float2; no element "
               "form: hipErrorInvalidValue; sdpnet_train._ln_fwd_rows falls back to sdp_rowstats + sdp_ln_apply"),
    Entry("sdp_add_ln_fwd", dict(X=M_, R=M_, Y=M_, A=M_, gamma=P_, beta=P_, scale=P_, stats=P_),
          refuses=_ref(X=SIX, R=SIX, Y=SIX, A=SIX, gamma=V16, beta=V16, stats=("base+elem", "base+4")),
          wide="add_ln_fwd_v8 as ln_fwd_v8 plus R and A rows: hipErrorNotSupported; sdpnet_hip.add_ln_fwd returns "
               "False and sdpnet_train runs the two passes",
          left_out=dict(reg_src=LIB, reg_dst0=LIB, reg_dst1=LIB)),
    Entry("sdp_ln_bwd", dict(X=M_, DY=M_, ADD=M_, DX=M_, stats=P_, gamma=P_, part=P_),
          wide="ln_bwd_sm / ln_bwd_v8: 8 elements of X, DY, ADD, DX, gamma as f32x4 (all in `vec`); stats and the "
               "partials one float at a time; else ln_bwd_k",
          left_out=dict(gpart=LIB, aff=LIB, ticket=LIB, O2=LIB, Z=LIB)),
    Entry("sdp_softmax_fwd", dict(S=M_, P=P_, Pd=P_, mask=P_),
          wide="softmax_fwd_r: f32x4 of S, 4-element stores of P, Pd (one ldp for both: tested with lds, Npad % 4); "
               "mask one float at a time; else softmax_fwd_k"),
    Entry("sdp_softmax_bwd", dict(P=M_, DPd=M_, DS=M_), wide="softmax_bwd_r: 4-element accesses of P, DPd, DS; else "
          "softmax_bwd_k"),
    Entry("sdp_nchw_to_rows", dict(X=P_, Y=M_), wide="element accesses only (LDS tile transpose)"),
    Entry("sdp_rows_to_nchw", dict(X=M_, Y=P_), wide="element accesses only"),
    Entry("sdp_group_mean", dict(X=M_, out=M_), wide="element accesses only"),
    Entry("sdp_nchw_add_table", dict(X=P_, table=P_), wide="element accesses only"),
    Entry("sdp_transpose", dict(X=M_, Y=M_), wide="element accesses only"),
    Entry("sdp_unpatchify", dict(rows=P_, img=P_), wide="element accesses only"),
    Entry("sdp_gemm_flex", dict(A=M_, B=M_, C=M_), wide="gemm_flex_bf16: bf16x8 loads per operand where base, ld and "
          "batch strides are 8-element aligned (va / vb), element loads otherwise; C element stores; fp32 scalar"),
    Entry("sdp_gemm_train_epi", dict(X=M_, W=M_, Y=M_, Y2=M_, Z=M_, bias=P_),
          refuses=_ref(X=SIX, W=SIX, Y=SIX, Y2=SIX, Z=SIX, bias=V16),
          wide="gemm_bf16_8ph with the whole-line epilogue only: hipErrorNotSupported; sdpnet_hip.gemm_train_epi "
               "returns False and the caller runs sdp_gemm + sdp_act_fwd / _bwd"),
    Entry("sdp_gemm_splitk", dict(X=M_, W=M_, Y=M_, R=M_, bias=P_, ws=P_),
          refuses=_ref(X=SIX, W=SIX, Y=ROW8, R=ROW8, bias=V16, ws=V16),
          wide="gemm_bf16_splitk: 16-B chunks of X, W, 8-B vectors of Y, R, f32x4 bias / ln_colsum, float2 ln_stats "
               "/ part, 16-B workspace: hipErrorInvalidValue (header); sdpnet_hip.gemm asks _splitk_aligned first",
          left_out=dict(ln_stats="not run: covered only by reading the predicate (gemm.hip, sdp_gemm_splitk: % 8); the "
                                 "statistics are sdp_ln_stats' output in sdpnet_engine's own buffer",
                        ln_colsum="not run, predicate read (% 16); " + LIB, part="not run, predicate read (% 8); " + LIB)),
    Entry("sdp_attn_train_fwd", dict(qkv=M_, o=M_, lse=P_), refuses=_ref(qkv=SIX, o=ROW8 + ("ld+4",)),
          wide="attn_fwd_k: bf16x8 loads of qkv rows, bf16x4 stores of o (ldo % 8 asked); lse one float per row; "
               "hipErrorInvalidValue; every operand is sdpnet_train's own buffer"),
    Entry("sdp_attn_train_bwd", dict(qkv=M_, o=M_, dO=M_, lse=P_, delta=P_, dq=M_, dk=M_, dv=M_),
          refuses=_ref(qkv=SIX, o=SIX, dO=SIX, dq=ROW8, dk=ROW8, dv=ROW8),
          wide="attn_bwd_q_k / attn_bwd_kv_k: bf16x8 loads of qkv, o, dO, 8-B stores of dq, dk, dv; lse, delta one "
               "float per row; hipErrorInvalidValue"),
    Entry("sdp_dw_wgrad", dict(A=M_, DY=M_, part=P_), wide="dw_wgrad_k: bf16x8 staging loads chosen in the kernel (A, "
          "DY % 16, lda, lddy % 8), element loads otherwise; the slabs one float at a time"),
    Entry("sdp_gemm_wgrad", dict(A=M_, B=M_, C=M_),
          refuses=_ref(A=SIX, B=SIX, C=("base+elem", "base+4", "base+8", "ld+1", "ld+2")),
          wide="gemm_wgrad_8ph: dY and X by 16-B chunks, f32x4 stores into the slabs C + s * split_stride: "
               "hipErrorNotSupported for A, B, C off 16 B / lda, ldb % 8 / ldc % 4, hipErrorInvalidValue for "
               "split_stride % 4; sdpnet_train._wgrad then takes sdp_gemm_flex",
          left_out=dict(zrow=LIB)),
    Entry("sdp_ln_fwd_mixed", dict(X=M_, Y=M_, gamma=P_, beta=P_, stats=P_),
          refuses=_ref(X=SIX, Y=SIX, gamma=V16, beta=V16, stats=("base+elem", "base+4")),
          wide="ln_fwd_impl: as sdp_ln_fwd"),
    Entry("sdp_ln_bwd_mixed", dict(X=M_, DY=M_, ADD=M_, DX=M_, stats=P_, gamma=P_, part=P_),
          refuses=_ref(X=SIX, DY=SIX, ADD=SIX, DX=SIX, gamma=V16),
          wide="ln_bwd_impl: mixed dtypes exist on ln_bwd_sm / ln_bwd_v8 only: hipErrorInvalidValue once `vec` fails"),
    Entry("sdp_ln_bwd_fused", dict(X=M_, DY=M_, ADD=M_, DX=M_, Z=M_, O2=M_, stats=P_, gamma=P_, scale=P_, part=P_),
          refuses=_ref(X=SIX, DY=SIX, ADD=SIX, DX=SIX, Z=SIX, O2=SIX, gamma=V16),
          wide="ln_bwd_v8 with the branch-gradient output: `vec` plus Z, O2 % 16 and ldz, ldo2 % 8, else "
               "hipErrorNotSupported; sdpnet_hip.ln_bwd runs the separate passes",
          left_out=dict(gpart=LIB, aff=LIB, ticket=LIB, reg_src=LIB, reg_dst=LIB)),
    Entry("sdp_mx_quant_rows", dict(X=M_, stats=P_), refuses=_ref(X=SIX, stats=("base+elem", "base+4")),
          wide="quant_rows: 16-B input vectors (bf16: ldx % 8), float2 stats, 8-B byte stores, 4-B scale words: "
               "hipErrorInvalidValue; Q and S (uint8) are shifted by hand in the test",
          left_out=dict(Q="uint8, no NaN sentinel: shifted by hand in the test", S="as Q")),
    Entry("sdp_mx_quant_rows[fp32]", dict(X=M_, stats=P_),
          refuses=_ref(X=("base+elem", "base+8", "ld+1", "ld+2"), stats=("base+elem", "base+4")),
          wide="as the bf16 form; an fp32 row stride needs ldx % 4 only, so ld + 4 runs"),
    Entry("sdp_gemm_mx", dict(bias=P_, R=M_, Y=M_, part=P_),
          refuses=_ref(bias=V16, R=ROW8, Y=ROW8, part=("base+elem", "base+4")),
          wide="gemm_mx: 16-B rows of Xq / Wq, 4-B scale rows, 8-B vectors of Y / R, f32x4 bias, float2 partials: "
               "hipErrorInvalidValue",
          left_out=dict(Xq="uint8: shifted by hand in the test", Xs="as Xq", Wq="as Xq", Ws="as Xq", Yq=LIB, Ys=LIB)),
] + [Entry(n, dict(logits=M_, targets=M_, teacher=M_, dlogits=M_), wide="element accesses only")
     for n in ("sdp_ce_loss", "sdp_ce_loss_soft", "sdp_bce_loss", "sdp_bce_loss_soft", "sdp_distill_loss")] + [
    Entry("sdp_logits_metrics", dict(logits=M_), wide="element accesses only"),
]
TABLE.update({e.name: e for e in _TRAIN})

# Entry points no test perturbs (profiles/alignment.md).
NOT_COVERED = (
    "sdp_train_batch_aug (test_gpu_augment.py has its unaligned case)",
)
