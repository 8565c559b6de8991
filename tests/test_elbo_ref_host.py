"""tests/elbo_ref.py on the CPU: the case builders meet the conditions that make the comparator's bar meaningful, the
comparator catches one wrong element (and a store past a row) and passes the fp32 reference itself, and the float64
reference is the oracle call that tests/test_gpu_elbo_models.py / tests/test_gpu_elbo.py already use."""
import pytest
import torch

from oracle import nma_oracle as O
from tests import elbo_ref as R
from tests.test_gpu_elbo_models import _oracle

BUILDERS = {"typical": R.typical_case, "tails": R.tails_case}


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(model, kind, M, B=5, n_win=3, seed=11):
        key = (model, kind, M, B, n_win, seed)
        if key not in cache:
            d = BUILDERS[kind](model, B, M, n_win, seed)
            cache[key] = (d, R.reference(model, d, torch.float64), R.reference(model, d, torch.float32))
        return cache[key]

    return get


@pytest.mark.parametrize("M", [5, 21])
@pytest.mark.parametrize("kind", ["typical", "tails"])
@pytest.mark.parametrize("model", R.MODELS)
def test_case_conditions(model, kind, M):
    """r32 / r64 finite, every scale > 0, per row scale <= 1e-3 max |r64| -- from the reference alone."""
    for B, n_win in ((1, 1), (5, 3)):
        c = R.case_conditions(model, BUILDERS[kind](model, B, M, n_win, seed=M + B))
        assert c["finite"] and c["positive"] and c["capped"], (B, n_win, c)


def test_tails_case_reaches_the_tails():
    """LV z over roughly [-12, 120] (both softplus regimes), masks other than 0 / 1 and the window-0 pin; SV states
    several units either side of -8 with theta at both ends of its spread."""
    d = R.tails_case("lv", 9, 519, 3, seed=1)
    assert float(d["z"].min()) < -11 and float(d["z"].max()) > 119
    assert ((d["mask"] != 0) & (d["mask"] != 1)).sum() >= 3
    assert (d["mask"][0, :, 0] == 0).all() and (d["shift"][0, :, 0] > 0).all()
    d = R.tails_case("sv", 9, 519, 3, seed=1)
    assert float(d["z"].min()) < -12.5 and float(d["z"].max()) > -3.5
    assert len(torch.unique(d["theta"][:, 2])) == 2


@pytest.mark.parametrize("model", R.MODELS)
def test_comparator_flags_one_planted_element(model, refs):
    """16 scale planted in ONE element of dz -- element 0, a chunk's last element, element M -- fails; r32 itself
    passes every output; the failure names the trajectory and the code path."""
    M = 21
    d, r64, r32 = refs(model, "typical", M)
    for k in R.OUTPUTS:
        assert R.compare(k, r32[k], r64[k], r32[k])["ok"], k
    zd = R.ZD[model]
    sc = R.scale_of("dz", r32["dz"], r64["dz"])
    for t, path in ((0, "tail"), (2 * R.KV - 1, "chunk 1"), (M, "tail")):
        for b in (0, 4):
            bad = r32["dz"].clone()
            i = zd * t + (zd - 1)
            bad[b, i] = r64["dz"][b, i] + 16.0 * sc[b, 0]
            res = R.compare("dz", bad, r64["dz"], r32["dz"])
            assert not res["ok"] and res["index"] == (b, i), (t, b, res)
            with pytest.raises(AssertionError, match=f"trajectory {b}, entry {i}, t={t}: {path}"):
                R.assert_close("dz", bad, r64["dz"], r32["dz"], model, M)
    # one wrong theta component / one wrong per-sample value
    bad = r32["dtheta"].clone()
    bad[2, 1] += 16.0 * R.scale_of("dtheta", r32["dtheta"], r64["dtheta"])[0, 1]
    assert not R.compare("dtheta", bad, r64["dtheta"], r32["dtheta"])["ok"]
    bad = r32["sde"].clone()
    bad[3] += 16.0 * R.scale_of("sde", r32["sde"], r64["sde"])[0]
    assert not R.compare("sde", bad, r64["sde"], r32["sde"])["ok"]
    # a NaN left in range fails
    bad = r32["dz"].clone()
    bad[1, 0] = float("nan")
    assert not R.compare("dz", bad, r64["dz"], r32["dz"])["ok"]


def test_small_error_in_one_element_hides_in_the_norm(refs):
    """The gap this comparator closes: the same planted element passes the whole-batch norm bar of 1e-4."""
    d, r64, r32 = refs("lv", "typical", 519, B=5)
    bad = r32["dz"].clone()
    bad[2, 2 * 259 + 1] += 16.0 * R.scale_of("dz", r32["dz"], r64["dz"])[2, 0]
    assert float((bad - r64["dz"]).norm() / r64["dz"].norm()) < 1e-4
    assert not R.compare("dz", bad, r64["dz"], r32["dz"])["ok"]


def test_guard_flags_a_store_past_a_row():
    """A value one element past the output (or before it) changes a sentinel; in-range writes do not."""
    n = 2 * 22
    for offset in (0, 1, 3):
        total, lo = R.guarded_layout(n, offset)
        buf = torch.empty(total, dtype=torch.int32)
        R.fill_guarded(buf, lo, n)
        assert torch.isnan(buf.view(torch.float32)[lo:lo + n]).all()
        assert R.guard_violations(buf, lo, n) == []
        buf.view(torch.float32)[lo:lo + n] = 1.5
        assert R.guard_violations(buf, lo, n) == []
        buf.view(torch.float32)[lo + n] = 1.5
        assert R.guard_violations(buf, lo, n) == [n]
        buf.view(torch.float32)[lo - 1] = float("nan")      # a plain NaN is not the sentinel either
        assert R.guard_violations(buf, lo, n) == [-1, n]


@pytest.mark.parametrize("model", R.MODELS)
def test_float64_reference_is_the_existing_oracle_call(model, refs):
    """reference(float64) on a shared case equals the oracle terms and autograd as the existing GPU tests call them."""
    d, r64, _ = refs(model, "typical", 21)
    z, th = d["z"].clone().requires_grad_(True), d["theta"].clone().requires_grad_(True)
    if model == "ar":
        w = d["win"].long()
        sde, obs = O.ar_elbo_terms(z, th, d["obs"][w], d["bin"][w], d["obs_std"])
        ex = torch.zeros_like(sde)
    else:
        sde, obs, ex = _oracle(model, d, z, th)
    loss = (sde * d["gs"]).sum()
    if d["go"] is not None:
        loss = loss + (obs * d["go"]).sum()
    if d["ge"] is not None:
        loss = loss + (ex * d["ge"]).sum()
    loss.backward()
    for k, v in (("sde", sde), ("obs", obs), ("extra", ex), ("dz", z.grad), ("dtheta", th.grad)):
        assert torch.equal(r64[k], v.detach()), k


def test_reference_optional_gradients_and_constant_z(refs):
    """None upstream gradients are zero; z_constant gives the same dtheta and no dz."""
    d, r64, _ = refs("lv", "typical", 21)
    zero = torch.zeros_like(d["gs"])
    a = R.reference("lv", d, g_obs=None, g_extra=None)
    b = R.reference("lv", d, g_obs=zero, g_extra=zero)
    assert torch.equal(a["dz"], b["dz"]) and torch.equal(a["dtheta"], b["dtheta"])
    c = R.reference("lv", d, z_constant=True)
    assert torch.equal(c["dtheta"], r64["dtheta"]) and not c["dz"].any()


def test_code_path_names():
    assert "tail" in R.code_path("sv", 519, 3)
    assert "chunk 1, iteration 0, lane 0" in R.code_path("sv", 519, 4)
    assert "chunk 64, iteration 0, lane 63" in R.code_path("lv", 519, 2 * (4 * 64 + 3))
    assert "deferred last element" in R.code_path("lv", 519, 2 * (4 * 64 + 3))
    assert "chunk 65, iteration 1, lane 0" in R.code_path("fhn", 519, 2 * 260)
    assert "tail" in R.code_path("sv", 518, 516)                 # (M + 1) / 4 = 129 full chunks: 516.. in the tail
    assert "chunk 128" in R.code_path("sv", 515, 515)            # the one-pass kernel's last chunk ...
    assert "tail" in R.code_path("sv", 515, 515, kernel="bwd")   # ... is tail in stream_bwd_kernel (M / 4 = 128)
