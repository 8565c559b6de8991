"""The flow kernels at the C ABI, element by element, over the dispatch matrix: every output tensor of
vissm_flow_fwd / vissm_flow_bwd (through ops.MAFlowFn) and of vissm_flow_ar_elbo_fused (ops.ar_last_flow_fused)
against the independent float64 reference tests/flow_ref.py, one case per dispatch row of flow_api.hip at the
smallest shape where the row can still go wrong, then one-factor edges.

CASES / FUSED_CASES below are the table (data: tests/test_flow_ref.py imports them for its CPU power test).  The
base shape: B = 19 (two sample groups, the second partial with an odd count: a ghost partner in the two-sample
kernels), Lh = 40 (two full 16-position tiles and one of 8), chunk_tiles = 1 (three t-chunks at k <= 16; the kernels
raise it to the halo minimum above), H = 50, n_logsig = Lout - 3.

Per case: the dispatch (ops.kernel_precision and _lib.flow_geometry against the table's expectation), every output's
error figure (flow_ref.measure) under its bar, two runs bitwise equal, every output element written (outputs are
prefilled with NaN) and no padding read or written (u, du_next and the outputs lie at a pitch with NaN padding).

Bars: kernels that compute in exact-class arithmetic (fp32, bf16x3, every fallback) are held to the project's fp32
bars, 1e-4 on forward tensors and 1e-3 on gradients; bf16 / bf16x2 (and the fused flow's bf16x2_bf16) to
EMUL_SAFETY x the envelope of flow_ref's rounding model over EMUL_REALISATIONS realisations + the fp32 bar."""
import contextlib
import dataclasses
import functools
import json
import os
from typing import Optional
from unittest import mock

import pytest
import torch

from tests import flow_ref as FR
from tests.parity_util import EMUL_REALISATIONS, EMUL_SAFETY
from viforssms_amd import _lib
from viforssms_amd.ops import FlowShape, MAFlowFn, ar_fused_supported, ar_last_flow_fused, kernel_precision

DEV = torch.device("cuda", 0)
PREC = {"fp32": _lib.VISSM_PREC_FP32, "bf16": _lib.VISSM_PREC_BF16, "bf16x3": _lib.VISSM_PREC_BF16X3,
        "bf16x2": _lib.VISSM_PREC_BF16X2, "bf16x2_bf16": _lib.VISSM_PREC_BF16X2_BF16}
# the rounding mode (oracle.precision_model.MODES) of a precision the kernels compute in; None: exact-class
MODE = {"fp32": None, "bf16x3": None, "bf16": "bf16", "bf16x2": "bf16x2", "bf16x2_bf16": "bf16x2f"}


@dataclasses.dataclass(frozen=True)
class Case:
    row: str                 # the dispatch row ("4"; "4eH": an edge in H on row 4's base case; "F": the fused flow)
    prec: str                # the precision asked for
    nh: int
    bn: bool
    s2: bool
    swap: bool
    n_win: int
    k: int
    runs: str                # the precision the kernels compute in: prec, or "fp32" for a fallback
    H: int = 50
    B: int = 19
    Lh: int = 40
    ct: int = 1
    nls: Optional[int] = None    # n_logsig; None: Lout - 3
    du: bool = True              # False: u without requires_grad (du = NULL on the flow5 kernels)
    fold: int = 0                # theta_rank of the theta fold (0: no factors passed)
    fused: bool = False
    seed: int = 1

    @property
    def s(self):
        return 2 if self.s2 else 1

    @property
    def Lout(self):
        return self.s * self.Lh

    @property
    def L(self):
        return self.Lout + self.k

    @property
    def n_logsig(self):
        if self.fused:
            return self.Lout - 1
        return max(0, self.Lout - 3) if self.nls is None else self.nls

    @property
    def id(self):
        t = f"r{self.row}-{self.prec}-nh{self.nh}{'-bn' if self.bn else ''}-s{self.s}{'x' if self.swap else ''}" \
            f"-w{self.n_win}-k{self.k}"
        if self.H != 50:
            t += f"-H{self.H}"
        if self.B != 19:
            t += f"-B{self.B}"
        if self.Lh != 40:
            t += f"-Lh{self.Lh}"
        if self.ct != 1:
            t += f"-ct{self.ct}"
        if self.nls is not None:
            t += f"-nls{self.nls}"
        if not self.du:
            t += "-nodu"
        if self.fold:
            t += f"-fold{self.fold}"
        return t

    def shape(self) -> FlowShape:
        return FlowShape(B=self.B, L=self.L, k=self.k, H=self.H, n_hidden=self.nh, bn=self.bn, stride2=self.s2,
                         swap_out=self.swap, n_logsig=self.n_logsig, n_win=self.n_win, precision=PREC[self.prec],
                         chunk_tiles=self.ct, pad_out=not self.fused)

    def cfg(self) -> dict:
        return dict(k=self.k, n_hidden=self.nh, bn=self.bn, stride2=self.s2, swap_out=self.swap,
                    n_logsig=self.n_logsig)


def _table():
    T = []

    def add(row, prec, nh, bn, ss, n_win, k, runs=None, **kw):
        T.append(Case(str(row), prec, nh, bool(bn), bool(ss[0]), bool(ss[1]), n_win, k, runs or prec, **kw))

    # 1: fp32, no hidden layer (flow_v4)
    for ss, k in [((0, 0), 1), ((1, 1), 8), ((0, 0), 8), ((1, 1), 1)]:
        add(1, "fp32", 0, 0, ss, 1, k)
    # 2: fp32, one hidden layer (flow_v4), with BN / stride 2 / swap
    for bn, ss, nw, k in [(0, (0, 0), 1, 8), (1, (1, 1), 1, 20), (0, (1, 0), 3, 64), (1, (0, 0), 3, 8),
                          (0, (1, 1), 1, 64), (1, (1, 0), 1, 20)]:
        add(2, "fp32", 1, bn, ss, nw, k)
    # 3: fp32, two to four hidden layers (flow_v2)
    for nh, bn, ss, nw, k in [(2, 0, (0, 0), 1, 6), (2, 1, (1, 1), 3, 20), (3, 0, (0, 0), 1, 20),
                              (3, 1, (1, 1), 1, 50), (3, 0, (1, 1), 3, 6), (4, 1, (0, 0), 1, 50),
                              (4, 0, (1, 1), 1, 6), (4, 1, (1, 1), 3, 20)]:
        add(3, "fp32", nh, bn, ss, nw, k)
    # 4: bf16 AR, k <= 8: fwd2 / bwd2 (du), flow_v5f (no du), with and without the theta fold
    for k, du, fold in [(1, 1, 0), (1, 0, 3), (5, 1, 5), (5, 0, 0), (8, 1, 0), (8, 1, 3), (8, 0, 0), (8, 0, 5)]:
        add(4, "bf16", 1, 0, (0, 0), 1, k, du=bool(du), fold=fold)
    # 5: bf16 AR, 8 < k <= 32: fwd2, one-sample backward JB 1, 2; fold at k <= 16
    for k, du, fold in [(9, 1, 0), (9, 1, 3), (16, 1, 5), (17, 1, 0), (32, 1, 0), (16, 0, 0)]:
        add(5, "bf16", 1, 0, (0, 0), 1, k, du=bool(du), fold=fold)
    # 6: bf16 AR, k > 32: fwd_kernel / bwd_kernel JB 3, 4
    for k, du in [(33, 1), (48, 1), (49, 1), (64, 1), (48, 0)]:
        add(6, "bf16", 1, 0, (0, 0), 1, k, du=bool(du))
    # 7: bf16 AR, several windows: one-sample kernels, S = 1 backward
    for k, du in [(8, 1), (20, 1), (8, 0)]:
        add(7, "bf16", 1, 0, (0, 0), 3, k, du=bool(du))
    # 8: bf16, one hidden layer with BN / stride 2 / swap: the one-sample Row<1, .., 1>
    for bn, ss, nw, k in [(1, (0, 0), 1, 8), (1, (1, 1), 1, 20), (1, (1, 0), 3, 8), (0, (1, 1), 1, 8),
                          (0, (1, 0), 1, 20), (0, (1, 1), 3, 20), (1, (1, 1), 3, 20)]:
        add(8, "bf16", 1, bn, ss, nw, k)
    add(8, "bf16", 1, 1, (1, 1), 1, 8, du=False)
    # 9: bf16, three hidden layers, k <= 24: flow_v5n (bwd2n, padded dcon rows)
    for bn, ss, k, du in [(1, (1, 1), 4, 1), (1, (1, 1), 16, 1), (1, (1, 0), 17, 1), (1, (1, 1), 24, 1),
                          (0, (0, 0), 16, 1), (0, (1, 1), 24, 1), (1, (0, 0), 4, 1), (1, (1, 1), 16, 0)]:
        add(9, "bf16", 3, bn, ss, 1, k, du=bool(du))
    # 10: bf16, three hidden layers, 24 < k <= 32: the base unit (fwd2<.., 3, 2, ..>, one-sample backward)
    for bn, ss, k in [(1, (1, 1), 25), (1, (0, 0), 28), (0, (1, 1), 32), (0, (0, 0), 25), (1, (1, 1), 32)]:
        add(10, "bf16", 3, bn, ss, 1, k)
    add(10, "bf16", 3, 1, (1, 1), 1, 28, du=False)
    # 11: bf16, three hidden layers, k > 32 at stride 1: flow_v5s (diagonal du sum, JB 3, 4)
    for bn, k, du in [(1, 33, 1), (1, 48, 1), (1, 50, 1), (1, 64, 1), (0, 50, 1), (0, 33, 1), (1, 50, 0)]:
        add(11, "bf16", 3, bn, (0, 0), 1, k, du=bool(du))
    # 12: bf16, three hidden layers, stride 2 above k = 32: the one-sample Row<3, ..>
    for k, du in [(33, 1), (64, 1), (48, 0)]:
        add(12, "bf16", 3, 1, (1, 1), 1, k, du=bool(du))
    # 13: bf16, three hidden layers, two windows: the one-sample Row<3, ..>, S = 1
    for ss, k in [((1, 1), 6), ((0, 0), 20), ((1, 1), 50), ((0, 0), 50)]:
        add(13, "bf16", 3, 1, ss, 2, k)
    add(13, "bf16", 3, 1, (1, 1), 2, 20, du=False)
    # 14: bf16x3, one hidden layer: Row<1, .., 3>
    for bn, ss, nw, k, du in [(0, (0, 0), 1, 8, 1), (0, (0, 0), 1, 16, 1), (0, (0, 0), 1, 17, 1),
                              (0, (0, 0), 3, 32, 1), (1, (1, 1), 1, 8, 1), (1, (0, 0), 1, 32, 1),
                              (0, (1, 1), 3, 17, 1), (1, (1, 1), 3, 16, 1), (0, (0, 0), 1, 8, 0)]:
        add(14, "bf16x3", 1, bn, ss, nw, k, du=bool(du))
    # 15: bf16x2 AR, k <= 8: the two-sample split-weight kernels (lofold)
    for k, du, fold in [(5, 1, 0), (5, 0, 3), (8, 1, 3), (8, 0, 0), (8, 1, 0)]:
        add(15, "bf16x2", 1, 0, (0, 0), 1, k, du=bool(du), fold=fold)
    # 16: bf16x2, one hidden layer beyond the two-sample backward: Row<1, .., 2>
    for bn, ss, nw, k in [(0, (0, 0), 1, 9), (0, (0, 0), 1, 16), (0, (0, 0), 1, 32), (1, (1, 1), 1, 9),
                          (1, (0, 0), 3, 16), (0, (1, 1), 3, 32), (0, (0, 0), 3, 9)]:
        add(16, "bf16x2", 1, bn, ss, nw, k)
    add(16, "bf16x2", 1, 0, (0, 0), 1, 16, du=False)
    # 17: fallbacks: a reduced precision asked for beyond flow5's shapes runs the exact-fp32 kernels
    for prec, nh, bn, ss, k, H in [("bf16", 0, 0, (0, 0), 8, 50), ("bf16", 2, 1, (1, 1), 8, 50),
                                   ("bf16", 4, 0, (0, 0), 8, 50), ("bf16x3", 2, 0, (0, 0), 8, 50),
                                   ("bf16x2", 0, 0, (1, 1), 8, 50), ("bf16x3", 1, 0, (0, 0), 33, 50),
                                   ("bf16x2", 1, 0, (0, 0), 33, 50), ("bf16", 1, 0, (0, 0), 8, 51),
                                   ("bf16", 3, 1, (1, 1), 8, 64), ("bf16x3", 1, 1, (0, 0), 8, 64)]:
        add(17, prec, nh, bn, ss, 1, k, runs="fp32", H=H)

    # single-factor edges on rows 2, 4, 9 and 11
    base = {2: ("fp32", 1, 0, (0, 0), 1, 8), 4: ("bf16", 1, 0, (0, 0), 1, 8), 9: ("bf16", 3, 1, (1, 1), 1, 16),
            11: ("bf16", 3, 1, (0, 0), 1, 50)}

    def edge(tag, r, **kw):
        add(f"{r}e{tag}", *base[r], **kw)

    for r in (2, 4, 9, 11):
        for H in (1, 15, 16, 17, 48, 49) + ((51, 63, 64) if r == 2 else ()):     # above kMaxH = 50: the fp32 rows only
            edge("H", r, H=H)
        for B in (1, 2, 16, 17, 33):
            edge("B", r, B=B)
        for Lh in (1, 15, 16, 17, 33):
            edge("L", r, Lh=Lh)
        edge("C", r, ct=0)
    # n_logsig: 0, 1 (odd: under stride 2 it counts one head position, as 2 would), Lout, and the first counted output
    # exactly on a t-chunk boundary (row 2: output 32 of 40, the fp32 tile; row 4: output 16 of 40; row 9, stride 2:
    # output 32 of 80, whose first counted head position is output 33; row 11 has one chunk: k = 50 needs four tiles).
    # The base shape's Lout - 3 is odd too.
    for r, ns in [(2, (0, 1, 40, 8)), (4, (0, 1, 40, 24)), (9, (0, 1, 80, 48)), (11, (0, 1, 40))]:
        for n in ns:
            edge("N", r, nls=n)
    return T


def _fused_table():
    T = []

    def add(prec, k, M=46, ct=1, B=19, n_win=1, fold=0):
        T.append(Case("F", prec, 1, False, False, False, n_win, k, prec, B=B, Lh=M + 1, ct=ct, fold=fold, fused=True))

    for k in (1, 8, 9, 32):
        add("bf16", k)
    for M in (14, 15, 16, 31):
        add("bf16", 8, M=M)
    add("bf16", 8, ct=0)
    add("bf16", 8, B=2)
    add("bf16", 8, n_win=3)
    add("bf16", 8, fold=3)
    add("bf16", 9, fold=5)
    for kw in (dict(k=8), dict(k=32), dict(k=8, M=15), dict(k=9, n_win=3), dict(k=8, ct=0)):
        add("bf16x3", **kw)
    for kw in (dict(k=1), dict(k=8), dict(k=8, M=16), dict(k=8, fold=3), dict(k=5, B=2)):
        add("bf16x2", **kw)
    for kw in (dict(k=1), dict(k=8), dict(k=8, M=31), dict(k=5, fold=5), dict(k=8, ct=0)):
        add("bf16x2_bf16", **kw)
    return T


# seeds for which a case's inputs meet the input conditions and the power conditions of tests/test_flow_ref.py
# (the default 1 elsewhere)
SEEDS = {"r2eH-fp32-nh1-s1-w1-k8-H1": 19, "r4eH-bf16-nh1-s1-w1-k8-H1": 19, "r11eL-bf16-nh3-bn-s1-w1-k50-Lh1": 2,
         # one unit per layer: a pre-activation w elu(z) + b seldom takes both signs at the prescribed scales
         "r9eH-bf16-nh3-bn-s2x-w1-k16-H1": 3039, "r11eH-bf16-nh3-bn-s1-w1-k50-H1": 4794}


def _seeded(cases):
    out = []
    for c in cases:
        out.append(dataclasses.replace(c, seed=SEEDS.get(c.id, 1)))
    assert len({c.id for c in out}) == len(out)
    return out


CASES = _seeded(_table())
FUSED_CASES = _seeded(_fused_table())
NEW_ROWS = ("1", "2", "3", "8", "14", "16", "17")     # rows no test ran before: test functions of their own


# ---------------------------------------------------------------------------------------------------------------
# inputs, reference and bars (CPU, float64; shared with tests/test_flow_ref.py)
# ---------------------------------------------------------------------------------------------------------------
def make_inputs(c: Case) -> dict:
    """Drawn in float64 on the CPU and rounded to fp32 (returned as float64 holding fp32 values): the kernels and
    the reference see the same numbers."""
    g = torch.Generator().manual_seed(1000 * c.seed + 7)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g, dtype=torch.float64) * sc).float().double()
    B, H, k, nh = c.B, c.H, c.k, c.nh
    d = {"u": r(B, c.L), "C": r(c.n_win, c.Lh, H, sc=0.3)}
    d["win"] = (torch.arange(B) % c.n_win).int() if c.n_win > 1 else None
    if c.fold:
        R = c.fold
        d["theta_x"], d["w_theta"], d["b_theta"] = r(B, R), r(R, H, sc=0.2 / R ** 0.5), r(H, sc=0.05)
        d["theta_term"] = (d["theta_x"] @ d["w_theta"] + d["b_theta"]).float().double()
    else:
        d["theta_term"] = r(B, H, sc=0.2)
    d["w_eps"], d["w_hid"], d["b_hid"] = r(k, H, sc=0.3), r(nh, H, H, sc=0.15), r(nh, H, sc=0.1)
    d["bn_g"] = (1 + r(nh, H, sc=0.1)).float().double() if c.bn else None
    d["bn_b"] = r(nh, H, sc=0.1) if c.bn else None
    d["w_head"], d["b_head"] = r(H, 2, sc=0.2), r(2, sc=0.1)
    if c.fused:
        M = c.Lout - 1
        d["theta"] = torch.stack([r(B, sc=0.3) + 1.0,
                                  (torch.rand(B, generator=g, dtype=torch.float64) * 0.8).float().double(),
                                  r(B, sc=0.2).abs() + 0.5], 1)
        d["obs"] = r(c.n_win, M)
        d["obs_bin"] = (torch.rand(c.n_win, M, generator=g) < 0.3).double()
        d["scale"] = 5000.0 / M
    else:
        d["du_next"], d["dlogsig"] = r(B, c.Lout), r(B)
    return d


def weights(d: dict) -> list:
    return [d[n] for n in FR.WEIGHTS]


def reference(c: Case, d: dict, **over) -> dict:
    """flow_ref's outputs of the case under the current rounding switches; over: replaced inputs / cfg entries (the
    power test's mutations)."""
    d = {**d, **{n: v for n, v in over.items() if n in d}}
    cfg = {**c.cfg(), **{n: v for n, v in over.items() if n not in d}}
    if c.fused:
        out = FR.fused_ref(d["u"], d["C"], d["win"], d["theta_term"], d["theta"], d["obs"], d["obs_bin"], 1.0,
                           d["scale"], weights(d), **cfg)
    else:
        out = FR.flow_ref_all(d["u"], d["C"], d["win"], d["theta_term"], weights(d), d["du_next"], d["dlogsig"],
                              **cfg)
    if not c.du:
        out.pop("du")
    return out


@functools.lru_cache(maxsize=None)
def reference_and_bars(c: Case):
    """(inputs, exact reference outputs, bar per output tensor)"""
    d = make_inputs(c)
    mode = MODE[c.runs]
    if mode is None:
        ref = reference(c, d)
        return d, ref, FR.exact_bars(ref)
    bars, ref = FR.emulated_bars(lambda: reference(c, d), mode, list(reference(c, d)), EMUL_SAFETY, EMUL_REALISATIONS)
    return d, ref, bars


def expected_geometry(c: Case, which: int) -> dict:
    """The launch geometry the case is meant to walk: tiles of 16 head positions on the bf16 matrix-core kernels (15
    produced positions in the fused flow), of 32 on the exact-fp32 kernels; groups of 16 samples, of 1 in a backward
    over several windows; a t-chunk of chunk_tiles tiles, at least the halo's ceil(ceil(k / s) / tile); chunk_tiles
    = 0: as many chunks as the halo minimum allows, up to the launch's target of work items."""
    flow5 = c.runs != "fp32"
    tile = 15 if which == 2 else 16 if flow5 else 32
    S = 1 if (which >= 1 and c.n_win > 1) else 16
    cdiv = lambda a, b: (a + b - 1) // b
    groups, tiles = cdiv(c.B, S), cdiv(c.Lh, tile)
    ch_min = max(1, cdiv(cdiv(c.k, c.s), tile))
    if c.ct > 0:
        tpc = max(c.ct, ch_min)
    else:
        nc = max(1, min(cdiv(8192 if flow5 else 2048, groups), max(1, tiles // ch_min)))
        tpc = max(cdiv(tiles, nc), ch_min)
    return {"tile": tile, "chunk_tiles": tpc, "n_chunks": cdiv(c.Lh, tpc * tile), "n_groups": groups}


def check_dispatch(c: Case):
    sh = c.shape()
    if c.fused:
        assert ar_fused_supported(sh), c.id
        assert _lib.flow_geometry(sh.desc(), 2) == expected_geometry(c, 2), c.id
        return
    assert kernel_precision(sh) == PREC[c.runs], (c.id, kernel_precision(sh))
    for which in (0, 1):
        assert _lib.flow_geometry(sh.desc(), which) == expected_geometry(c, which), (c.id, which)


# ---------------------------------------------------------------------------------------------------------------
# the GPU side
# ---------------------------------------------------------------------------------------------------------------
NAN = float("nan")


@contextlib.contextmanager
def _nan_alloc():
    """Every float buffer the op allocates (torch.empty / torch.empty_like: the outputs) starts as NaN: the ABI says
    "written, not accumulated", so a finite result shows that every element was written."""
    empty, empty_like = torch.empty, torch.empty_like

    def fill(t):
        return t.fill_(NAN) if t.is_floating_point() else t

    with mock.patch.object(torch, "empty", lambda *a, **k: fill(empty(*a, **k))), \
            mock.patch.object(torch, "empty_like", lambda *a, **k: fill(empty_like(*a, **k))):
        yield


def _padded(x: torch.Tensor, extra: int) -> torch.Tensor:
    buf = torch.full((x.shape[0], x.shape[1] + extra), NAN, device=x.device)
    buf[:, :x.shape[1]] = x
    return buf[:, :x.shape[1]]


def _check_rows(name, t: torch.Tensor, cid):
    """t [B, n] rows at a pitch: every element finite, the padding between rows still NaN"""
    assert bool(torch.isfinite(t).all()), (cid, name, "an output element was not written")
    pitch = t.stride(0) if t.shape[0] > 1 else t.shape[1]
    if pitch > t.shape[1]:
        pad = t.as_strided((t.shape[0], pitch), (pitch, 1), t.storage_offset())[:, t.shape[1]:]
        assert bool(torch.isnan(pad).all()), (cid, name, "padding written")


class _Ctx:
    """The autograd context MAFlowFn.forward / backward use, so that the tensors the backward returns (du at u's
    pitch, with its padding) are inspected as the op made them."""

    def __init__(self, need_du):
        self.needs_input_grad = (False, False, need_du) + (True,) * 10

    def save_for_backward(self, *ts):
        self.saved_tensors = ts


def _dev(t, dtype=torch.float32):
    return None if t is None else t.to(dtype).to(DEV).contiguous()


def run_flow(c: Case, d: dict) -> dict:
    sh = c.shape()
    t = {n: _dev(v) for n, v in d.items() if n != "win" and not isinstance(v, float)}
    win = _dev(d["win"], torch.int32)
    u = _padded(t["u"], 5)
    tf = (t["theta_x"], t["w_theta"], t["b_theta"]) if c.fold else None
    ws = [t[n] for n in FR.WEIGHTS]
    with _nan_alloc():
        if c.fused:
            ws5 = [t[n] for n in ("w_eps", "w_hid", "b_hid", "w_head", "b_head")]
            x, ls, du, dC, dth, gw = ar_last_flow_fused(sh, win, u, t["C"], t["theta_term"], t["theta"], t["obs"],
                                                        t["obs_bin"], 1.0, d["scale"], *ws5, tf)
            out = {"x": x, "logsig": ls, "du": du, "dC": dC, "dtheta_term": dth}
            out.update({"d" + n: g for n, g in zip(("w_eps", "w_hid", "b_hid", "w_head", "b_head"), gw)})
        else:
            ctx = _Ctx(c.du)
            un, ls = MAFlowFn.forward(ctx, sh, win, u, t["C"], t["theta_term"], *ws, tf)
            gs = MAFlowFn.backward(ctx, _padded(t["du_next"], 3), t["dlogsig"])
            out = {"u_next": un, "logsig": ls, "dC": gs[3], "dtheta_term": gs[4]}
            if c.du:
                out["du"] = gs[2]
            else:
                assert gs[2] is None, (c.id, "du computed though not asked for")
            out.update({"d" + n: g for n, g in zip(FR.WEIGHTS, gs[5:12]) if g is not None})
    torch.cuda.synchronize()
    for n, v in out.items():
        if n in ("u_next", "du"):
            _check_rows(n, v, c.id)
        else:
            assert bool(torch.isfinite(v).all()), (c.id, n, "an output element was not written")
    assert bool(torch.isnan(u.as_strided((c.B, c.L + 5), (c.L + 5, 1), 0)[:, c.L:]).all())
    return {n: v.contiguous().cpu() for n, v in out.items()}


def _check(c: Case):
    check_dispatch(c)
    d, ref, bars = reference_and_bars(c)
    got = run_flow(c, d)
    again = run_flow(c, d)
    assert set(got) == set(ref), (c.id, sorted(got), sorted(ref))
    figs = FR.measures(got, ref)
    for n in ref:
        print(f"{c.id:48s} {n:12s} {figs[n]:.3e}  bar {bars[n]:.3e}")
    log = os.environ.get("VISSM_FLOW_ABI_FIGURES")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps({"id": c.id, "runs": c.runs, "figs": figs, "bars": bars}) + "\n")
    for n in ref:
        assert torch.equal(got[n], again[n]), (c.id, n, "two runs differ")
    bad = {n: (figs[n], bars[n]) for n in ref if not figs[n] <= bars[n]}
    assert not bad, (c.id, bad)


def _rows(*rows):
    cs = [c for c in CASES if c.row.split("e")[0] in rows]
    return pytest.mark.parametrize("c", cs, ids=[c.id for c in cs])


pytestmark = pytest.mark.gpu


@_rows("4", "5", "6", "7", "9", "10", "11", "12", "13", "15")
def test_flow_rows_run_before(c):
    """Rows whose kernels the model-level parity tests run (with the edges on rows 4, 9 and 11)."""
    _check(c)


@_rows("1", "2")
def test_flow_fp32_flow4(c):
    """flow_v4: no or one hidden layer, with BN, stride 2 and swap_out (rows 1 and 2 and row 2's edges)."""
    _check(c)


@_rows("3")
def test_flow_fp32_flow2(c):
    """flow_v2: two to four hidden layers, with and without BN (row 3)."""
    _check(c)


@_rows("8")
def test_flow_bf16_one_layer_bn_stride2(c):
    """Row 8: the one-sample bf16 kernels at one hidden layer with BN, stride 2 or swap_out."""
    _check(c)


@_rows("14")
def test_flow_bf16x3(c):
    """Row 14: Row<1, .., 3>."""
    _check(c)


@_rows("16")
def test_flow_bf16x2_one_sample(c):
    """Row 16: Row<1, .., 2>."""
    _check(c)


@_rows("17")
def test_flow_fallbacks(c):
    """Row 17: a reduced precision beyond flow5's shapes reports and computes exact fp32."""
    _check(c)


@pytest.mark.parametrize("c", FUSED_CASES, ids=[c.id for c in FUSED_CASES])
def test_fused_flow(c):
    """vissm_flow_ar_elbo_fused per element against flow_ref.fused_ref."""
    _check(c)
