"""vissm_feat_geometry (host arithmetic, no GPU): which of the three tile variants vissm_feat_fwd / vissm_feat_bwd
launch for a descriptor, their blocks per window and dynamic LDS, against the rule restated here: kT is the largest of
32 / 16 with ceil(Lh / kT) n_win >= 512 blocks, else 8; VISSM_FEAT_KT / VISSM_FEAT_KT_BWD override it."""
import ctypes

import pytest

from viforssms_amd import _lib


def _desc(n_win, Lh, k=5, s=1, Cin=3, H=7, slack=2):
    Lf = s * (Lh - 1) + k + slack
    return _lib.FeatDesc(n_win, Lf, Cin, H, k, s, Lh, (Lf + 1) * Cin)


def _ceil(a, b):
    return -(-a // b)


def _pad32(r):
    return _ceil(r, 32) * 32


def _fwd_lds(kT, s, k, H, Cin):
    """rows of F a block computes, padded to 32: two activation buffers and one weight image, rows of H + 1 /
    max(Cin, H) + 1 floats"""
    RP, hp, wp = _pad32(s * (kT - 1) + k), H + 1, max(Cin, H) + 1
    return 4 * (RP * wp + RP * hp + wp * hp)


def _bwd_lds(kT, s, k, H, Cin):
    """staged dC rows, staged F rows, two gradient buffers, one layer input, one weight image"""
    hp, ip = H + 1, Cin + 1
    DP, FP, GP = _pad32(kT + _ceil(k - 1, s) + 1), _pad32(s * (kT - 1) + k), _pad32(s * kT)
    return 4 * (DP * hp + FP * hp + 2 * GP * hp + GP * max(ip, hp) + max(Cin, H) * hp)


@pytest.fixture(autouse=True)
def _no_override(monkeypatch):
    monkeypatch.delenv("VISSM_FEAT_KT", raising=False)
    monkeypatch.delenv("VISSM_FEAT_KT_BWD", raising=False)


@pytest.mark.parametrize("n_win,Lh,want", [
    (64, 256, 32),    # 8 x 64 = 512 blocks of 32 positions
    (64, 255, 32),    # the last block partial: still 8 per window
    (64, 224, 16),    # 7 x 64 = 448 < 512 at 32; 14 x 64 at 16
    (64, 128, 16),    # 4 x 64 at 32; 8 x 64 = 512 at 16
    (64, 127, 16),    # ceil(127 / 16) = 8: the partial block counts
    (64, 113, 16),
    (64, 112, 8),     # 7 x 64 = 448 < 512 at 16
    (1, 5017, 8),     # AR-cfg: 157 / 314 blocks
    (1, 512 * 16, 16), (1, 512 * 32, 32),
])
def test_feat_geometry_thresholds(n_win, Lh, want):
    d = _desc(n_win, Lh)
    for bwd in (False, True):
        g = _lib.feat_geometry(d, bwd)
        assert g["kt"] == want, (bwd, g)
        Lu = d.stride * (Lh - 1) + d.k
        assert g["blocks"] == (_ceil(Lu, d.stride * want) if bwd else _ceil(Lh, want))
        assert g["lds_bytes"] == (_bwd_lds if bwd else _fwd_lds)(want, d.stride, d.k, d.H, d.Cin)


def test_feat_geometry_ar_paper_resolves_to_8():
    """hyperparameters.txt's AR shape (50 windows of 199 rows, k = 50): 250 / 500 blocks, 12 short of the bar; a dozen
    more windows cross it"""
    d = _lib.FeatDesc(50, 199, 14, 50, 50, 1, 150, 199 * 14)
    assert _lib.feat_geometry(d, False)["kt"] == 8 and _lib.feat_geometry(d, True)["kt"] == 8
    d = _lib.FeatDesc(52, 199, 14, 50, 50, 1, 150, 199 * 14)
    assert _lib.feat_geometry(d, False)["kt"] == 16 and _lib.feat_geometry(d, True)["kt"] == 16


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("kt", [8, 16, 32])
def test_feat_geometry_override_each_direction(monkeypatch, kt, s):
    d = _desc(3, 41, k=6, s=s)
    base = (_lib.feat_geometry(d, False), _lib.feat_geometry(d, True))
    assert base[0]["kt"] == base[1]["kt"] == 8
    monkeypatch.setenv("VISSM_FEAT_KT", str(kt))
    f, b = _lib.feat_geometry(d, False), _lib.feat_geometry(d, True)
    assert f == {"kt": kt, "blocks": _ceil(41, kt), "lds_bytes": _fwd_lds(kt, s, 6, 7, 3)}
    assert b == base[1]                      # the forward's override leaves the backward alone
    monkeypatch.delenv("VISSM_FEAT_KT")
    monkeypatch.setenv("VISSM_FEAT_KT_BWD", str(kt))
    f, b = _lib.feat_geometry(d, False), _lib.feat_geometry(d, True)
    assert f == base[0]
    assert b == {"kt": kt, "blocks": _ceil(s * 40 + 6, s * kt), "lds_bytes": _bwd_lds(kt, s, 6, 7, 3)}
    # the backward's choice sizes its workspace: blocks x the slab row, + the reduced row
    n = 3 * 7 + 7 + 3 * (7 * 7 + 7) + 6 * 7 * 7 + 7
    al = lambda x: _ceil(x, 256) * 256
    ws = _lib.load().vissm_feat_workspace_size(ctypes.byref(d))
    assert ws >= 3 * b["blocks"] * n * 4 + n * 4 and ws <= al(3 * b["blocks"] * n * 4) + al(n * 4)
    monkeypatch.setenv("VISSM_FEAT_KT_BWD", "12")   # not a variant: ignored
    assert _lib.feat_geometry(d, True) == base[1]


def test_feat_geometry_lds_extreme_fits_the_requested_limit(monkeypatch):
    """kT = 32, s = 2, k = 64, H = 64, Cin = 63: the largest launch the shape limits allow stays within the 160 KB
    the kernels' dynamic-LDS attribute is raised to"""
    d = _lib.FeatDesc(1, 2 * 39 + 64, 63, 64, 64, 2, 40, 0)
    monkeypatch.setenv("VISSM_FEAT_KT", "32")
    monkeypatch.setenv("VISSM_FEAT_KT_BWD", "32")
    f, b = _lib.feat_geometry(d, False), _lib.feat_geometry(d, True)
    assert f["lds_bytes"] == 83460 and b["lds_bytes"] == 124800
    assert max(f["lds_bytes"], b["lds_bytes"]) <= 160 * 1024
    # no smaller variant or stride needs more
    for kt in (8, 16, 32):
        for s in (1, 2):
            assert _fwd_lds(kt, s, 64, 64, 63) <= 83460 and _bwd_lds(kt, s, 64, 64, 63) <= 124800


@pytest.mark.parametrize("bad", [(1, 100, 14, 65, 8, 1, 93, 0), (1, 100, 64, 50, 8, 1, 93, 0), (1, 100, 14, 50, 8, 3, 10, 0),
                                 (1, 100, 14, 50, 8, 1, 94, 0), (1, 100, 14, 50, 1, 2, 10, 0),
                                 (2, 100, 14, 50, 8, 1, 93, 99 * 14)])
def test_feat_geometry_refuses_bad_descriptor(bad):
    lib = _lib.load()
    out = (ctypes.c_int32 * 3)(-7, -7, -7)
    assert lib.vissm_feat_geometry(ctypes.byref(_lib.FeatDesc(*bad)), 0, out) == -1   # VISSM_EINVAL
    assert list(out) == [-7, -7, -7]
    with pytest.raises(_lib.VissmError):
        _lib.feat_geometry(_lib.FeatDesc(*bad), True)
    assert lib.vissm_feat_geometry(ctypes.byref(_lib.FeatDesc(1, 100, 14, 50, 8, 1, 93, 0)), 0, None) == -1
