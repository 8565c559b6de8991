"""The edges of the bf16 matrix-core GEMM (vissm_gemm_bf16) and its split-bf16 form (vissm_gemm_bf16x3), held per
element where tests/test_gpu_lvfeat.py / test_gpu_svfeat.py hold a norm over the matrix.

Bound.  bf16 x bf16 products are exact in fp32 and each accumulation commits at most one rounding of relative size
2^-23 whatever the matrix core's rounding mode, so against ref = the float64 product of the same bf16 operands
    |C - ref|[m][n] <= (K + split) 2^-23 (|A| |B|)[m][n]
(split: the partials' fixed-order sum).  The x3 form computes A_hi B_hi + A_hi B_lo + A_lo B_hi: ref is the float64
sum of those three products and 3 K stands for K, so the dropped lo lo term is not charged to the kernel.  A bf16
epilogue adds one bf16 rounding, 2^-8 of the value (2^-16 for the x3 plane pair), to the bound carried through the
epilogue's function (ELU and x elu'(y) have slope at most one).

Shapes: a 3 x 4 grid of tiles (the XCD renumbering with a remainder mod 8 and more than one tile column), exact
tiles with one and two K steps, single rows / columns, K in {0, 1, 7, 8, 33} (no step, less than a chunk, one past a
step), more splits than K steps, bf16 outputs whose rows start off the 16-byte grid (ldc = N + 1, and an odd one),
in all four operand layouts.  C starts as NaN: an unwritten element shows, and the padding must stay NaN."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from viforssms_amd import _lib  # noqa: E402
from viforssms_amd.ops import gemm_bf16, gemm_bf16x3  # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
NAN = float("nan")
EPS = 2.0 ** -23
WORST = {}


def _r8(n):
    return (n + 7) // 8 * 8


def _operand(rows, cols, g):
    """fp32 [rows][ld] (at least one row, ld a multiple of 8): random in [:rows, :cols], NaN elsewhere (never read)"""
    x = torch.full((max(rows, 1), max(_r8(cols), 8)), NAN, device=DEV)
    x[:rows, :cols] = torch.randn(rows, cols, generator=g, device=DEV) * 0.5
    return x


def _split(x):
    hi = x.to(BF)
    return hi, (x - hi.float()).to(BF)


class Case:
    """operands of one (M, N, K, layout) in both forms, the float64 references and the magnitude products"""

    def __init__(self, M, N, K, akm, bkm):
        g = torch.Generator(device=DEV).manual_seed(M * 7 + N * 3 + K * 11 + 2 * akm + bkm)
        self.M, self.N, self.K, self.akm, self.bkm = M, N, K, akm, bkm
        A = _operand(K, M, g) if akm else _operand(M, K, g)
        B = _operand(K, N, g) if bkm else _operand(N, K, g)
        self.lda, self.ldb = A.shape[1], B.shape[1]
        self.A, self.B = _split(A), _split(B)
        am = lambda t: (t[:K, :M].t() if akm else t[:M, :K]).double()
        bm = lambda t: (t[:K, :N] if bkm else t[:N, :K].t()).double()
        Ah, Al, Bh, Bl = am(self.A[0]), am(self.A[1]), bm(self.B[0]), bm(self.B[1])
        self.ref = {False: Ah @ Bh, True: Ah @ Bh + Ah @ Bl + Al @ Bh}
        self.mag = {False: Ah.abs() @ Bh.abs(),
                    True: Ah.abs() @ Bh.abs() + Ah.abs() @ Bl.abs() + Al.abs() @ Bh.abs()}

    def run(self, x3, C, ldc, epi=_lib.GEMM_F32, aux=None, split=1):
        if x3:
            gemm_bf16x3(self.M, self.N, self.K, self.A[0], self.A[1], self.lda, self.akm, self.B[0], self.B[1],
                        self.ldb, self.bkm, C, ldc, epi, aux, split)
        else:
            gemm_bf16(self.M, self.N, self.K, self.A[0], self.lda, self.akm, self.B[0], self.ldb, self.bkm, C, ldc,
                      epi, aux, split)
        torch.cuda.synchronize()

    def acc_bound(self, x3, split):
        return ((3 if x3 else 1) * self.K + split) * EPS * self.mag[x3]


def _hold(group, what, got, ref, bound):
    """every element within its bound (exactly equal where the bound is zero); records the largest error / bound"""
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(got.double()).all()), (what, "not finite: an element was not written")
    bad = err > bound
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    assert not bool(bad.any()), (what, f"{int(bad.sum())} elements beyond the bound, worst error / bound {ratio:.3g}")
    if float(bound.max()) > 0:
        WORST[group] = max(WORST.get(group, 0.0), ratio)
    return ratio


def _planes(x3, M, ldc):
    """NaN-filled bf16 output: [M][ldc], or the x3 form's plane pair [2][M][ldc] (the lo plane M ldc elements on)"""
    return torch.full((2, M, ldc) if x3 else (1, M, ldc), NAN, device=DEV, dtype=BF)


def _value(Y, N):
    return Y[:, :, :N].double().sum(0)


SHAPES = [(300, 400, 40), (128, 128, 32), (256, 128, 64), (1, 1, 1), (1, 200, 9), (200, 1, 9),
          (37, 45, 0), (37, 45, 1), (37, 45, 7), (37, 45, 8), (37, 45, 33)]


@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "x3"])
@pytest.mark.parametrize("akm", [False, True], ids=["a_rowmajor", "a_kmajor"])
@pytest.mark.parametrize("bkm", [False, True], ids=["b_colmajor", "b_kmajor"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_edges(x3, akm, bkm, M, N, K):
    c = Case(M, N, K, akm, bkm)
    ref, tag = c.ref[x3], "x3" if x3 else "bf16"
    # fp32 epilogue, unsplit and split (3; and 8 at K = 40: more splits than K steps)
    for split in (1, 3) + ((8,) if K == 40 else ()):
        C = torch.full((M, N), NAN, device=DEV)
        c.run(x3, C, N, split=split)
        r = _hold(f"{tag} fp32", ("fp32", split), C, ref, c.acc_bound(x3, split))
        if K == 0:
            assert int(torch.count_nonzero(C)) == 0
    print(f"[gemm-edges] {tag} fp32 {(M, N, K, akm, bkm)}: error / bound {r:.3f}")
    # bf16 epilogues into rows that start off the 16-byte grid: ldc = N + 1, and an odd ldc where N + 1 is even
    rnd = 2.0 ** -16 if x3 else 2.0 ** -8
    for ldc in sorted({N + 1, (N + 1) | 1}):
        Y = _planes(x3, M, ldc)
        c.run(x3, Y, ldc, _lib.GEMM_ELU_BF16)
        elu = torch.where(ref > 0, ref, torch.expm1(ref))
        y = _value(Y, N)
        r1 = _hold(f"{tag} elu", ("elu", ldc), y, elu, c.acc_bound(x3, 1) + rnd * elu.abs())
        assert bool(torch.isnan(Y[:, :, N:].float()).all()), ("elu padding written", ldc)
        Z = _planes(x3, M, ldc)
        c.run(x3, Z, ldc, _lib.GEMM_DELU_BF16, aux=Y)
        f = torch.where(y < 0, y + 1, torch.ones_like(y))
        dref = ref * f
        r2 = _hold(f"{tag} delu", ("delu", ldc), _value(Z, N), dref, c.acc_bound(x3, 1) * f.abs() + rnd * dref.abs())
        assert bool(torch.isnan(Z[:, :, N:].float()).all()), ("elu' padding written", ldc)
        if K == 0:   # exact zeros, in every plane
            assert int(torch.count_nonzero(Y[:, :, :N].float())) == 0 and int(torch.count_nonzero(Z[:, :, :N].float())) == 0
        print(f"[gemm-edges] {tag} ldc {ldc}: elu error / bound {r1:.3f}, elu' {r2:.3f}")
    print("[gemm-edges] worst error / bound so far:", {k: round(v, 3) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "x3"])
def test_gemm_aligned_bf16_epilogue_per_element(x3):
    """the 16-byte store path (ldc a multiple of 8) at the 3 x 4 tile grid, per element like the rest"""
    M, N, K = 300, 400, 40
    c = Case(M, N, K, False, True)
    ref, ldc, rnd = c.ref[x3], _r8(N) + 8, 2.0 ** -16 if x3 else 2.0 ** -8
    Y = _planes(x3, M, ldc)
    c.run(x3, Y, ldc, _lib.GEMM_ELU_BF16)
    elu = torch.where(ref > 0, ref, torch.expm1(ref))
    _hold(f"{'x3' if x3 else 'bf16'} elu", "elu aligned", _value(Y, N), elu, c.acc_bound(x3, 1) + rnd * elu.abs())
    assert bool(torch.isnan(Y[:, :, N:].float()).all())
