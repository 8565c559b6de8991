"""CPU tests of the flow reference (tests/flow_ref.py) and of the power of the GPU tests built on it
(tests/test_gpu_flow_abi.py): the reference agrees with the oracle where the oracle covers it, its autograd is right,
its BN folding is an identity, its rounding switches are the established model's on the AR shape -- and, for every
case of the GPU table, the bars the GPU test will apply reject each of a list of single-defect kernels."""
import pytest
import torch

from oracle import nma_oracle as O
from oracle import precision_model as PM
from tests import flow_ref as FR
from tests import test_gpu_flow_abi as T

DT = torch.float64


def _draw(B, Lh, k, H, nh, bn, s2, n_win=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g, dtype=DT) * sc
    L = (2 if s2 else 1) * Lh + k
    d = dict(u=r(B, L), C=r(n_win, Lh, H, sc=0.3), theta_term=r(B, H, sc=0.2),
             win=(torch.arange(B) % n_win).int() if n_win > 1 else None,
             w_eps=r(k, H, sc=0.3), w_hid=r(nh, H, H, sc=0.15), b_hid=r(nh, H, sc=0.1),
             bn_g=1 + r(nh, H, sc=0.1) if bn else None, bn_b=r(nh, H, sc=0.1) if bn else None,
             w_head=r(H, 2, sc=0.2), b_head=r(2, sc=0.1))
    d["du_next"], d["dlogsig"] = r(B, L - k), r(B)
    return d


def _ws(d):
    return [d[n] for n in FR.WEIGHTS]


def _oracle_all(d, k, nh, bn, s2, swap, n_logsig, flow=None):
    """The oracle's flow on equivalent inputs: theta_term through an identity theta branch, C scattered to the
    positions the oracle's full-length first conv evaluates (its head takes every s-th)."""
    B, L = d["u"].shape
    H = d["w_eps"].shape[1]
    s = 2 if s2 else 1
    leaf = lambda t: t.detach().clone().requires_grad_(True) if t is not None else None
    u, C, tt = leaf(d["u"]), leaf(d["C"]), leaf(d["theta_term"])
    ws = [leaf(w) for w in _ws(d)]
    w_eps, w_hid, b_hid, bn_g, bn_b, w_head, b_head = ws
    eye, zero = torch.eye(H, dtype=DT), torch.zeros(H, dtype=DT)
    P = {"conv_w": w_eps[:, None, :], "th_w0": eye, "th_b0": zero, "th_w1": eye, "th_b1": zero, "th_w2": eye,
         "th_b2": zero, "head_w": w_head, "head_b": b_head}
    for l in range(nh):
        P[f"hid_w{l}"], P[f"hid_b{l}"] = w_hid[l], b_hid[l]
        if bn:
            P[f"bn_g{l}"], P[f"bn_b{l}"] = bn_g[l], bn_b[l]
    Cw = C[d["win"].long()] if d["win"] is not None else C[0][None].expand(B, -1, -1)
    if s2:
        CF = torch.stack([Cw, torch.zeros_like(Cw)], 2).reshape(B, -1, H)
    else:
        CF = Cw
    cfg = O.FlowCfg(k=k, H=H, n_hidden=nh, n_logsig=n_logsig, stride2=s2, bn=bn)
    un, sl = (flow or O.iaf_flow)(u, CF, tt, P, cfg)
    if swap:
        un = O.swap_pairs(un)
    ls = sl.sum(1)
    out = {"u_next": un.detach(), "logsig": ls.detach()}
    out.update(FR._grads([un, ls], [d["du_next"], d["dlogsig"]], u, C, tt, ws))
    return out


def _assert_close(a: dict, b: dict, tol=1e-12):
    assert set(a) == set(b)
    for n in a:
        err = float((a[n] - b[n]).abs().max()) / max(float(b[n].abs().max()), 1e-300)
        assert err <= tol, (n, err)


ORACLE_SHAPES = {"ar": dict(B=5, Lh=37, k=8, H=50, nh=1, bn=False, s2=False, swap=False, n_win=1),
                 "lv": dict(B=4, Lh=21, k=20, H=50, nh=3, bn=True, s2=True, swap=True, n_win=3),
                 "sv": dict(B=3, Lh=19, k=50, H=50, nh=3, bn=True, s2=False, swap=False, n_win=1)}


@pytest.mark.parametrize("fam", list(ORACLE_SHAPES))
def test_flow_ref_agrees_with_oracle(fam):
    sh = dict(ORACLE_SHAPES[fam])
    swap = sh.pop("swap")
    d = _draw(**sh, seed=3)
    k, nh, bn, s2 = sh["k"], sh["nh"], sh["bn"], sh["s2"]
    Lout = d["u"].shape[1] - k
    for n_logsig in (Lout - 3, Lout, 1):
        ref = FR.flow_ref_all(d["u"], d["C"], d["win"], d["theta_term"], _ws(d), d["du_next"], d["dlogsig"], k=k,
                              n_hidden=nh, bn=bn, stride2=s2, swap_out=swap, n_logsig=n_logsig)
        _assert_close(ref, _oracle_all(d, k, nh, bn, s2, swap, n_logsig))


def test_fused_ref_agrees_with_oracle_terms():
    B, M, k, H = 4, 30, 8, 50
    d = _draw(B, M + 1, k, H, 1, False, False, n_win=2, seed=5)
    g = torch.Generator().manual_seed(6)
    theta = torch.stack([torch.randn(B, generator=g, dtype=DT) * 0.3 + 1, torch.rand(B, generator=g, dtype=DT) * 0.8,
                         torch.randn(B, generator=g, dtype=DT).abs() * 0.2 + 0.5], 1)
    obs, obs_bin = torch.randn(2, M, generator=g, dtype=DT), (torch.rand(2, M, generator=g) < 0.3).double()
    scale = 5000.0 / M
    cfg = dict(k=k, n_hidden=1, bn=False, stride2=False, swap_out=False, n_logsig=M)
    got = FR.fused_ref(d["u"], d["C"], d["win"], d["theta_term"], theta, obs, obs_bin, 1.0, scale, _ws(d), **cfg)
    u, C, tt, ws = FR._leaves(d["u"], d["C"], d["theta_term"], _ws(d))
    x, ls = FR.flow_ref(u, C, d["win"], tt, *ws, **cfg)
    wl = d["win"].long()
    sde, ob = O.ar_elbo_terms(x, theta, obs[wl], obs_bin[wl], 1.0)
    want = {"x": x.detach(), "logsig": ls.detach()}
    want.update(FR._grads([-scale * (sde + ob + ls).sum()], None, u, C, tt, ws))
    _assert_close(got, want)


@pytest.mark.parametrize("s2", [False, True])
def test_flow_ref_gradcheck(s2):
    nh, bn, k = 2, True, 3
    d = _draw(2, 3, k, 3, nh, bn, s2, n_win=2, seed=8)
    names = ["u", "C", "theta_term"] + list(FR.WEIGHTS)
    ins = [d[n].clone().requires_grad_(True) for n in names]

    def f(u, C, tt, *ws):
        return FR.flow_ref(u, C, d["win"], tt, *ws, k=k, n_hidden=nh, bn=bn, stride2=s2, swap_out=s2, n_logsig=3)

    assert torch.autograd.gradcheck(f, ins, eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("nh,s2", [(1, False), (3, True), (4, False)])
def test_bn_folding_is_an_identity(nh, s2):
    d = _draw(4, 9, 5, 17, nh, True, s2, n_win=2, seed=9)
    cfg = dict(k=5, n_hidden=nh, bn=True, stride2=s2, swap_out=s2, n_logsig=6)
    run = lambda folded: FR.flow_ref_all(d["u"], d["C"], d["win"], d["theta_term"], _ws(d), d["du_next"],
                                         d["dlogsig"], folded=folded, **cfg)
    _assert_close(run(True), run(False))


@pytest.mark.parametrize("mode", ["bf16", "bf16x2f", "bf16x2"])
def test_rounding_switches_are_the_established_model(mode, monkeypatch):
    """At realisation 0 on an AR shape flow_ref rounds what precision_model.iaf_flow_emul rounds: equal to 1e-12,
    values and gradients.  flow_ref's one further rounding point (EXTRA["bias_g"]) moves the two bias gradients
    only."""
    sh = dict(ORACLE_SHAPES["ar"])
    sh.pop("swap")
    d = _draw(**sh, seed=4)
    k, Lout = sh["k"], d["u"].shape[1] - sh["k"]
    run = lambda: FR.flow_ref_all(d["u"], d["C"], d["win"], d["theta_term"], _ws(d), d["du_next"], d["dlogsig"], k=k,
                                  n_hidden=1, bn=False, stride2=False, swap_out=False, n_logsig=Lout - 3)
    with PM.emulate(mode):
        want = _oracle_all(d, k, 1, False, False, False, Lout - 3, flow=PM.iaf_flow_emul)
        with_extra = run()
        monkeypatch.setitem(FR.EXTRA, "bias_g", False)
        got = run()
    _assert_close(got, want)
    moved = {n for n in want if float((with_extra[n] - want[n]).abs().max()) > 1e-12 * float(want[n].abs().max())}
    assert moved == {"db_hid", "db_head"}
    monkeypatch.setitem(FR.EXTRA, "bias_g", True)
    exact = FR.flow_ref_all(d["u"], d["C"], d["win"], d["theta_term"], _ws(d), d["du_next"], d["dlogsig"], k=k,
                            n_hidden=1, bn=False, stride2=False, swap_out=False, n_logsig=Lout - 3)
    assert FR.measure("du", got["du"], exact["du"]) > 1e-4      # the switches were on


# ---------------------------------------------------------------------------------------------------------------
# the GPU table: dispatch, input conditions and power, case by case
# ---------------------------------------------------------------------------------------------------------------
ALL = T.CASES + T.FUSED_CASES
_ids = [c.id for c in ALL]


def test_table_covers_every_row():
    rows = {c.row for c in T.CASES}
    assert {str(i) for i in range(1, 18)} <= rows
    assert 120 <= len(T.CASES) <= 200, len(T.CASES)
    for r in T.NEW_ROWS:
        assert any(c.row == r for c in T.CASES)


@pytest.mark.parametrize("c", ALL, ids=_ids)
def test_case_dispatch(c):
    """The precision and the launch geometry the library picks for the case (host arithmetic: no GPU) are the
    table's: a case that silently took another path would fail here and in the GPU test."""
    T.check_dispatch(c)
    if c.row.isdigit() and c.B == 19 and c.Lh == 40 and c.ct == 1 and c.runs != "fp32":
        # the base shape walks what it is meant to: two groups of 16 (19 of one sample over several windows in the
        # backward) and three t-chunks while the halo fits one tile
        gb = T.expected_geometry(c, 1)
        halo = -(-c.k // c.s)
        assert gb["n_groups"] == (19 if c.n_win > 1 else 2)
        assert gb["n_chunks"] == (3 if halo <= 16 else 2 if halo <= 32 else 1)


@pytest.mark.parametrize("c", ALL, ids=_ids)
def test_case_input_conditions(c):
    d, ref, bars = T.reference_and_bars(c)
    for n, v in ref.items():
        assert bool(torch.isfinite(v).all()), n
        if v.numel() == 0:       # w_hid / b_hid without a hidden layer
            continue
        if n == "logsig" and c.n_logsig == 0:
            assert not bool(v.any())
            continue
        assert bool(v.abs().max() > 0), (n, "identically zero")
    with torch.no_grad():
        mu, r, pre = FR.flow_layers(d["u"], d["C"], d["win"], d["theta_term"], *T.weights(d), k=c.k, n_hidden=c.nh,
                                    bn=c.bn, stride2=c.s2)
    for l, z in enumerate(pre):
        share = float((z < 0).double().mean())
        assert 0.2 <= share <= 0.8, (l, share)
    assert bool((r > 0).any()) and bool((r < 0).any())


def _mutants(c, d, ref):
    """(name, outputs of a kernel with that single defect) for every defect that applies to the case"""
    gb = T.expected_geometry(c, 2 if c.fused else 1)
    CH = gb["chunk_tiles"] * gb["tile"]

    def edit(name, fn):
        out = {n: v.clone() for n, v in ref.items()}
        fn(out[name])
        return out

    if "du" in ref:     # 1: du zero at the one position just after a t-chunk join (one chunk: the middle)
        pos = c.s * CH if gb["n_chunks"] > 1 else c.L // 2
        du = ref["du"]
        b = int((du[:, pos].abs() / du.abs().max(1).values).argmax())
        yield "du_join", edit("du", lambda t: t[b].__setitem__(pos, 0.0))
    w = d["w_eps"].clone()                                  # 2: tap k - 1 of w_eps dropped
    w[c.k - 1] = 0
    yield "tap_dropped", T.reference(c, d, w_eps=w)
    if c.swap:                                              # 3: the last pair left unswapped
        yield "last_pair", edit("u_next", lambda t: t[:, -2:].copy_(t[:, -2:].flip(-1).clone()))
    # 4: n_logsig counted one too many.  Where that cannot show -- n_logsig = Lout, or stride 2 with an extra output
    # that is a copy (log sigma = 0: an odd n_logsig counts what n_logsig + 1 counts) -- one head position too few
    more = c.n_logsig + 1
    if more <= c.Lout and (not c.s2 or (c.Lout - more) % 2 == 1):
        miscount = more
    else:
        miscount = c.n_logsig - (2 if c.s2 and c.n_logsig % 2 == 0 else 1)
    yield "n_logsig", T.reference(c, d, n_logsig_count=miscount)
    if c.bn and c.nh > 0:                                   # 5: beta of one BN layer dropped
        bb = d["bn_b"].clone()
        bb[c.nh - 1] = 0
        yield "beta_dropped", T.reference(c, d, bn_b=bb)
    if c.B > 1:                                             # 6: one sample's dtheta_term row given to its partner
        yield "dtheta_partner", edit("dtheta_term", lambda t: t[1].copy_(t[0].clone()))
    dC = ref["dC"]                                          # 7: one dC row of the last partial tile dropped
    wmax = int((dC[:, -1].abs().amax(1) / dC.abs().amax((1, 2))).argmax())
    yield "dC_row", edit("dC", lambda t: t[wmax, -1].zero_())


@pytest.mark.parametrize("c", ALL, ids=_ids)
def test_case_power(c):
    """Each single-defect mutant of the reference outputs exceeds the case's bar on at least one tensor."""
    d, ref, bars = T.reference_and_bars(c)
    for name, out in _mutants(c, d, ref):
        figs = FR.measures(out, ref)
        assert any(figs[n] > bars[n] for n in ref), (name, {n: (figs[n], bars[n]) for n in ref})
