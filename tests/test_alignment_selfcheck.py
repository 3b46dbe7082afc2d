"""The alignment harness (alignment.py) judged on CPU tensors: a torch emulation of a row kernel
y = 2 x in four versions, addressed by bytes the way a kernel addresses.  The harness must pass
the correct one under every perturbation and flag each of the three wrong ones with a message that
names what it saw -- the evidence that test_gpu_alignment.py can fail.  No mutated kernel is built
or run on a GPU."""
import pytest
import torch

import alignment as al

DTYPES = [torch.bfloat16, torch.float32]
M, C = 5, 24     # 48-B (bf16) / 96-B (fp32) rows: whole 16-B granules when the base is aligned


def _flat(view):
    n = view.untyped_storage().nbytes() // view.element_size()
    return torch.empty(0, dtype=view.dtype).set_(view.untyped_storage(), 0, (n,), (1,))


def fake_kernel(x: torch.Tensor, y: torch.Tensor, bug: str = "") -> int:
    """y = 2 x row by row on byte addresses inside the two allocations; returns 0, or non-zero for a
    refusal.  ``bug``: "trunc_read" reads each row from its address rounded down to 16 B (a vector
    load whose low address bits are dropped); "granule_write" stores whole 16-B granules around
    each row; "late_refusal" refuses an unaligned operand after it has written half of the rows;
    "refuse" is a correct kernel that refuses an unaligned operand before it writes."""
    es = x.element_size()
    fx, fy = _flat(x), _flat(y)
    unaligned = any((t.storage_offset() * es) % 16 or (t.stride(0) * es) % 16 for t in (x, y))
    if bug == "refuse" and unaligned:
        return 1
    for r in range(x.shape[0]):
        if bug == "late_refusal" and unaligned and r == x.shape[0] // 2:
            return 1
        sb = (x.storage_offset() + r * x.stride(0)) * es
        db = (y.storage_offset() + r * y.stride(0)) * es
        if bug == "trunc_read":
            sb -= sb % 16
        row = fx[sb // es: sb // es + x.shape[1]] * 2
        if bug == "granule_write":
            lo, hi = db - db % 16, -(-(db + x.shape[1] * es) // 16) * 16
            fy[lo // es: hi // es] = 0
        fy[db // es: db // es + x.shape[1]] = row
    return 0


def run(dtype, bug, xcase=None, ycase=None, expect=None):
    g = torch.Generator().manual_seed(3)
    dense = torch.randn(M, C, generator=g).to(dtype)
    x = al.place(dense, xcase, ld=C + 8)
    y = al.place(dense, ycase, ld=C + 8, out=True)
    rc = fake_kernel(x, y, bug)

    def verify():
        assert torch.equal(y, dense * 2), "wrong result"
    return al.judge(f"fake[{bug or 'correct'}]", rc != 0, {"x": (x, dense)}, {"y": y}, verify, expect)


def misaligns(dtype, *cases):
    """Does any of the cases put a row off a 16-B boundary?  (ld + 4 fp32 elements does not.)"""
    es = torch.empty(0, dtype=dtype).element_size()
    return any(c is not None and (c.bytes_for(dtype) if not c.delta else c.delta * es) % 16 for c in cases)


PERTURBED = [(c, None) for c in al.CASES] + [(None, c) for c in al.CASES] + [(al.BASE[0], al.BASE[0])]
IDS = [f"x:{a.id}" if b is None else f"y:{b.id}" if a is None else "all" for a, b in PERTURBED]


@pytest.mark.parametrize("dtype", DTYPES)
def test_shifted_views_have_the_promised_shape(dtype):
    es = torch.empty(0, dtype=dtype).element_size()
    dense = torch.arange(M * C).reshape(M, C).to(dtype)
    for case in al.CASES:
        v = al.place(dense, case, ld=C + 8)
        assert v.data_ptr() % 16 == (case.bytes_for(dtype) if not case.delta else 0)
        assert v.stride() == (C + 8 + case.delta, 1) and torch.equal(v, dense)
        flat = _flat(v)
        assert torch.isnan(flat[: v.storage_offset()]).all()                       # guard rows in front
        assert torch.isnan(flat[v.storage_offset() + C: v.storage_offset() + v.stride(0)]).all()   # padding columns
        assert torch.isnan(flat[v.storage_offset() + (M - 1) * v.stride(0) + C:]).all()            # guard rows behind
        assert v.storage_offset() >= al.GUARD_ROWS * v.stride(0)
        assert flat.numel() - (v.storage_offset() + M * v.stride(0)) >= al.GUARD_ROWS * v.stride(0)
        assert not al.findings(v)
    assert {c.bytes_for(dtype) for c in al.BASE} == {es, 4, 8}
    vec = al.place(dense[0], al.BASE[0])
    assert vec.shape == (C,) and vec.data_ptr() % 16 == es and not al.findings(vec)
    out = al.place(dense, al.BASE[2], out=True)
    assert al.untouched(out) and [k for k, _ in al.findings(out)] == ["poisoned"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("xcase,ycase", [(None, None)] + PERTURBED, ids=["aligned"] + IDS)
def test_correct_kernel_passes(dtype, xcase, ycase):
    assert run(dtype, "", xcase, ycase, expect=al.RAN) == al.RAN


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("xcase,ycase", PERTURBED, ids=IDS)
def test_clean_refusal_passes(dtype, xcase, ycase):
    assert run(dtype, "refuse", expect=al.RAN) == al.RAN
    if not misaligns(dtype, xcase, ycase):
        return
    assert run(dtype, "refuse", xcase, ycase) == al.REFUSED
    with pytest.raises(AssertionError, match="the table promises ran"):
        run(dtype, "refuse", xcase, ycase, expect=al.RAN)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bug", ["trunc_read", "granule_write", "late_refusal"])
def test_broken_kernels_pass_when_aligned(dtype, bug):
    """Each fault is invisible on aligned operands: what the rest of the suite sees."""
    assert run(dtype, bug) == al.RAN


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", al.CASES, ids=lambda c: c.id)
def test_truncated_read_address_is_seen(dtype, case):
    """x off a 16-B boundary: the rows come from lower addresses -- the elements in front, or the
    sentinel (a NaN, so the output is poisoned)."""
    if not misaligns(dtype, case):
        assert run(dtype, "trunc_read", xcase=case) == al.RAN
        return
    with pytest.raises(AssertionError, match="non-finite logical element|wrong result"):
        run(dtype, "trunc_read", xcase=case)
    assert run(dtype, "trunc_read", ycase=case) == al.RAN      # only the read side is wrong


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", al.CASES, ids=lambda c: c.id)
def test_whole_granule_store_is_seen(dtype, case):
    if not misaligns(dtype, case):
        assert run(dtype, "granule_write", ycase=case) == al.RAN
        return
    with pytest.raises(AssertionError, match="output y: element .* written outside the operand") as e:
        run(dtype, "granule_write", ycase=case)
    if case.delta == 0:
        assert "before the view" in str(e.value)               # the granule starts below the base
    else:
        assert "column" in str(e.value)                        # a padding (guard) column of a row
    assert run(dtype, "granule_write", xcase=case) == al.RAN   # only the write side is wrong


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("xcase,ycase", PERTURBED, ids=IDS)
def test_refusal_after_a_partial_write_is_seen(dtype, xcase, ycase):
    if not misaligns(dtype, xcase, ycase):
        assert run(dtype, "late_refusal", xcase, ycase) == al.RAN
        return
    with pytest.raises(AssertionError, match="output y was written although the call was refused"):
        run(dtype, "late_refusal", xcase, ycase)


def test_a_modified_input_and_a_changed_inplace_operand_are_seen():
    dense = torch.ones(M, C)
    x = al.place(dense, al.BASE[0])
    x[1, 1] = 2.0
    with pytest.raises(AssertionError, match="input x was modified"):
        al.judge("t", False, {"x": (x, dense)}, {}, lambda: None)
    io = al.place(dense, al.BASE[0])
    before = io.clone()
    io[0, 0] = 3.0
    with pytest.raises(AssertionError, match="in-place operand io was written although"):
        al.judge("t", True, {}, {}, lambda: None, inouts={"io": (io, before)})
    assert al.judge("t", False, {}, {}, lambda: None, inouts={"io": (io, before)}) == al.RAN


def test_the_table_names_operands_and_cases():
    assert al.TABLE, "the coverage table is empty"
    for e in al.TABLE.values():
        assert e.operands and e.wide, e.name
        for op, cid in e.refuses:
            # a one-element shift may be listed by its byte count (2 or 4)
            assert op in e.operands and cid in {c.id for c in al.CASES} | {"base+2", "base+4"}, (e.name, op, cid)
        for op, why in e.left_out.items():
            assert op not in e.operands and why, (e.name, op)
