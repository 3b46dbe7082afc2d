"""Far-placement harness: put a small logical [M, C] matrix at chosen byte offsets inside one
big allocation, behind a row map, and check what a kernel touched.

The row map (grp, gstride, off) of ``sdpnet_hip.Rows`` makes far placement cheap: a handful of
groups with a large ``gstride`` touches a few hundred KB of data, yet puts rows on both sides of
byte marks such as 2^31 and 2^32 (where 32-bit offset arithmetic wraps or changes sign) and of
the 2^31-element mark.  Everything outside the logical elements -- the padding columns
(ld > C), the rows between the groups, the rows before the first and after the last group --
holds a sentinel:

  * the sentinel is a NaN bit pattern, so a kernel that reads outside its operand poisons its
    result, and a store the hardware range check dropped (a too-short buffer descriptor) leaves
    a non-finite logical element behind;
  * ``findings()`` compares every element outside the logical ones with the sentinel (integer
    min / max over the whole buffer: no full-size temporaries), and names what it saw.

No GPU call happens at import; the same code runs on CPU tensors with scaled-down marks
(test_placement_selfcheck.py), which is the evidence that the GPU tests can fail.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch

import sdpnet_hip as sp

# dtype -> (integer view type, sentinel as that integer).  Both are NaNs with a recognisable
# payload: non-finite as a number, and no kernel produces this exact pattern by arithmetic.
SENTINEL = {torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FA5A5A5)}

OFF = 3    # rows before the first group (off > 0)
TAIL = 3   # rows after the last group


class Placement:
    """One allocation of ``total_rows`` x ``ld`` elements holding the logical [M, C] matrix at
    physical rows (m // grp) * gstride + off + m % grp, sentinel everywhere else."""

    def __init__(self, M: int, C: int, dtype: torch.dtype, device, grp: int, gstride: int, off: int, ld: int,
                 total_rows: int, marks: Sequence[int] = ()):
        assert M > 0 and 0 < C <= ld and grp > 0 and off > 0
        self.M, self.C, self.dtype, self.grp, self.gstride, self.off, self.ld = M, C, dtype, grp, gstride, off, ld
        self.total_rows, self.marks = total_rows, tuple(marks)
        self.itype, self.sent = SENTINEL[dtype]
        self.es = torch.empty(0, dtype=dtype).element_size()
        self.groups = (M + grp - 1) // grp
        assert self.groups == 1 or gstride >= grp, "groups overlap"
        assert (self.groups - 1) * gstride + off + (M - 1) % grp < total_rows
        self.ibuf = torch.full((total_rows, ld), self.sent, dtype=self.itype, device=device)
        self.t = self.ibuf.view(dtype)
        assert self.t.data_ptr() % 16 == 0
        m = torch.arange(M, device=device)
        self.prow = (m // grp) * gstride + off + m % grp

    # ---- construction
    @classmethod
    def far(cls, C: int, dtype: torch.dtype, marks: Sequence[int], device, grp: int = 64, sub: int = 1,
            M: Optional[int] = None, ld: Optional[int] = None) -> "Placement":
        """Groups ``base = gcd(marks) / sub`` bytes apart (less a few rows), so that the group
        numbered mark / base straddles each mark with rows on both sides; ``M`` defaults to whole
        groups up to the one on the largest mark."""
        m = cls.far_map(C, dtype, marks, grp, sub, M, ld)
        p = cls(m["M"], C, dtype, device, grp, m["gstride"], OFF, m["ld"], m["total_rows"], marks)
        p.require_straddles()
        return p

    @staticmethod
    def far_map(C: int, dtype: torch.dtype, marks: Sequence[int], grp: int = 64, sub: int = 1,
                M: Optional[int] = None, ld: Optional[int] = None) -> dict:
        """The numbers of far(): M, ld, gstride and total_rows (no allocation)."""
        es = torch.empty(0, dtype=dtype).element_size()
        ld = ld if ld is not None else default_ld(C)
        rowb = ld * es
        base = math.gcd(*marks) // sub
        jmax = max(mk // base for mk in marks)
        short = max(OFF + 1, (grp + 2) // (2 * jmax))   # rows by which gstride falls short of base
        gstride = base // rowb - short
        G = jmax + 1
        M = M if M is not None else G * grp
        assert (M + grp - 1) // grp == G, "M must reach the group on the largest mark"
        return dict(M=M, ld=ld, gstride=gstride, total_rows=(G - 1) * gstride + OFF + (M - 1) % grp + 1 + TAIL)

    @classmethod
    def near(cls, C: int, dtype: torch.dtype, device, grp: int = 64, groups: int = 5, M: Optional[int] = None,
             ld: Optional[int] = None) -> "Placement":
        """The twin of a far placement: same grp / off / ld / group count, groups 5 rows apart."""
        ld = ld if ld is not None else default_ld(C)
        M = M if M is not None else groups * grp
        G = (M + grp - 1) // grp
        gstride = grp + 5
        total = (G - 1) * gstride + OFF + (M - 1) % grp + 1 + TAIL
        return cls(M, C, dtype, device, grp, gstride, OFF, ld, total)

    def twin(self, C: int, dtype: torch.dtype, ld: Optional[int] = None) -> "Placement":
        """Another per-row buffer on the same physical rows (LN partials next to a GEMM output)."""
        return Placement(self.M, C, dtype, self.t.device, self.grp, self.gstride, self.off,
                         ld if ld is not None else C, self.total_rows)

    # ---- the operand
    @property
    def rows(self) -> sp.Rows:
        return sp.Rows(self.t, self.ld, self.grp, self.gstride, self.off)

    @property
    def nbytes(self) -> int:
        return self.total_rows * self.ld * self.es

    def row_byte(self, m: int) -> int:
        """Byte offset of logical row m from the start of the allocation."""
        return ((m // self.grp) * self.gstride + self.off + m % self.grp) * self.ld * self.es

    def scatter(self, dense: torch.Tensor) -> "Placement":
        assert tuple(dense.shape) == (self.M, self.C) and dense.dtype == self.dtype
        self.t[self.prow, :self.C] = dense
        return self

    def gather(self) -> torch.Tensor:
        return self.t[self.prow, :self.C]

    def view(self) -> torch.Tensor:
        """The logical matrix as a strided tensor (groups of one row: row stride gstride * ld), for
        the kernels that take a pointer and a row stride instead of a row map."""
        assert self.grp == 1
        return torch.as_strided(self.t, (self.M, self.C), (self.gstride * self.ld, 1), self.off * self.ld)

    def crossed(self) -> List[int]:
        """The marks that have logical rows on both sides."""
        first, last = self.row_byte(0), self.row_byte(self.M - 1)
        return [mk for mk in self.marks if first < mk <= last]

    def require_straddles(self):
        rowb = self.ld * self.es
        for mk in self.marks:
            hit = [g for g in range(self.groups)
                   if self.row_byte(g * self.grp) + rowb <= mk <= self.row_byte(min(self.M, (g + 1) * self.grp) - 1)]
            assert hit, f"no group straddles the mark at byte {mk}"
        assert self.row_byte(self.M - 1) + (1 + TAIL) * rowb == self.nbytes

    # ---- what did the kernel touch
    def dropped(self) -> List[Tuple[str, str]]:
        """Logical rows that still hold the sentinel: stores that were dropped or went elsewhere."""
        rows = (self.ibuf[self.prow, :self.C] == self.sent).any(1).nonzero().flatten().tolist()
        if not rows:
            return []
        b = self.row_byte(rows[0])
        past = [mk for mk in self.marks if b + self.ld * self.es > mk]
        where = f"beyond the mark at byte {max(past)}" if past else "below every mark"
        return [("dropped", f"{len(rows)} logical row(s) {rows[0]}..{rows[-1]} still hold the sentinel (stores "
                            f"dropped or sent elsewhere); the first starts at byte {b}, {where}")]

    def strays(self, limit: int = 4) -> List[Tuple[str, str]]:
        """Elements outside the logical ones that no longer hold the sentinel."""
        saved = self.ibuf[self.prow, :self.C].clone()
        self.ibuf[self.prow, :self.C] = self.sent
        try:
            if int(self.ibuf.min()) == self.sent and int(self.ibuf.max()) == self.sent:
                return []
            out: List[Tuple[str, str]] = []
            step = max(1, (1 << 24) // self.ld)
            for r0 in range(0, self.total_rows, step):
                chunk = self.ibuf[r0:r0 + step]
                if int(chunk.min()) == self.sent and int(chunk.max()) == self.sent:
                    continue
                for r, c in (chunk != self.sent).nonzero()[:limit].tolist():
                    out.append(self._classify(r0 + r, c))
                if len(out) >= limit:
                    break
            return out[:limit]
        finally:
            self.ibuf[self.prow, :self.C] = saved

    def _classify(self, p: int, c: int) -> Tuple[str, str]:
        at = f"physical row {p} column {c} (byte {(p * self.ld + c) * self.es})"
        g = min(max((p - self.off) // self.gstride, 0), self.groups - 1) if self.gstride else 0
        r = p - g * self.gstride - self.off
        glen = min(self.grp, self.M - g * self.grp)
        if 0 <= r < glen:
            return "padding", f"padding column written: {at}, logical row {g * self.grp + r}, C = {self.C}"
        if p < self.off:
            return "before", f"row before the first group written: {at}, {self.off - p} row(s) before the operand"
        if g == self.groups - 1 and r >= glen:
            return "past_end", f"row past the end written: {at}, {r - glen + 1} row(s) after the last logical row"
        return "between", f"row between groups written: {at}, {r - glen + 1} row(s) after the end of group {g}"

    def findings(self, written: bool) -> List[Tuple[str, str]]:
        return (self.dropped() if written else []) + self.strays()

    def check(self, what: str, written: bool = False):
        """Raise unless every element outside the logical ones holds the sentinel (and, for an
        output, no logical row still does)."""
        f = self.findings(written)
        assert not f, f"{what}: " + "; ".join(msg for _, msg in f)

    def assert_untouched(self, what: str = "operand"):
        self.check(what, written=False)


def default_ld(C: int) -> int:
    """ld > C with the alignment the fast paths need (ld % 8 == 0)."""
    return (C + 7) // 8 * 8 + 8


def marks_for(dtype: torch.dtype, first: int = 1 << 31) -> List[int]:
    """``first`` bytes, 2 * ``first`` bytes and ``first`` elements: with the default, 2^31 bytes, 2^32
    bytes and 2^31 elements (bf16: 2^32 bytes again; fp32: 8 GiB)."""
    es = torch.empty(0, dtype=dtype).element_size()
    return sorted({first, 2 * first, first * es})
