"""The column statistics' host-checkable parts (viforssms_amd/csrc/colstat_math.hpp through libvissm_hostcheck.so, and
the host-only queries of libvissm.so): the order key and its inverse, the radix select's narrowing step, a numpy
emulation of the 4-pass select, and the descriptor checks.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from tests.colstat_util import data_classes, f32_from_bits as _f, np_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "viforssms_amd", "libvissm_hostcheck.so")


@pytest.fixture(scope="module")
def host():
    lib = ctypes.CDLL(HOSTCHECK)
    lib.vissm_host_colkey.restype = ctypes.c_uint32
    lib.vissm_host_colkey.argtypes = [ctypes.c_float]
    lib.vissm_host_colkey_inv.restype = ctypes.c_float
    lib.vissm_host_colkey_inv.argtypes = [ctypes.c_uint32]
    lib.vissm_host_col_narrow.restype = None
    lib.vissm_host_col_narrow.argtypes = [ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                          ctypes.POINTER(ctypes.c_uint32), ctypes.c_int]
    return lib


SPECIALS = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,
            0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000]
NANS = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0xFFFFFFFF, 0x7FFFFFFF]


def test_key_order_and_round_trip_on_special_values(host):
    vals = [_f(b) for b in SPECIALS]
    keys = [host.vissm_host_colkey(ctypes.c_float(v)) for v in vals]
    for v, k in zip(vals, keys):
        assert k == int(np_key(np.array([v]))[0])
        back = np.float32(host.vissm_host_colkey_inv(k))
        want = np.float32(0.0) if v == 0 else v
        assert back.view(np.uint32) == want.view(np.uint32), (v, hex(k))       # -0 -> +0, everything else bitwise
    for i, (a, ka) in enumerate(zip(vals, keys)):
        for b, kb in zip(vals[i + 1:], keys[i + 1:]):
            assert (ka < kb) == (a < b) and (kb < ka) == (b < a) and (ka == kb) == (a == b), (a, b)
    for b in NANS:
        k = host.vissm_host_colkey(ctypes.c_float(_f(b)))
        assert k == 0xFFFFFFFF and k > max(keys)                              # every NaN last
        assert np.isnan(host.vissm_host_colkey_inv(k))
    # sorting by key is numpy's sort
    rng = np.random.default_rng(0)
    x = rng.integers(0, 2 ** 32, 2000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    x = np.concatenate([x, np.array(vals, dtype=np.float32), np.array([_f(b) for b in NANS], dtype=np.float32)])
    k = np.array([host.vissm_host_colkey(ctypes.c_float(v)) for v in x], dtype=np.uint32)
    assert np.array_equal(k, np_key(x))
    assert np.array_equal(x[np.argsort(k, kind="stable")] + np.float32(0), np.sort(x) + np.float32(0), equal_nan=True)


def _narrow(host, hist, rank_left, prefix, p):
    h = np.ascontiguousarray(hist, dtype=np.int32)
    r, pre = ctypes.c_int32(int(rank_left)), ctypes.c_uint32(int(prefix))
    host.vissm_host_col_narrow(h.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(r), ctypes.byref(pre), p)
    return r.value, pre.value


def test_narrow_matches_cumsum_searchsorted(host):
    rng = np.random.default_rng(1)
    for trial in range(200):
        hist = rng.integers(0, 50, 256).astype(np.int32)
        hist[rng.random(256) < (0.0, 0.5, 0.97)[trial % 3]] = 0               # empty bins, nearly all empty
        if hist.sum() == 0:
            hist[rng.integers(256)] = 3
        cum = np.cumsum(hist)
        edges = np.concatenate([[0], cum[hist > 0][:-1], cum[hist > 0] - 1, [cum[-1] - 1]])   # first / last of a bin
        for rank in list(rng.integers(0, cum[-1], 5)) + list(edges[rng.integers(0, len(edges), 5)]):
            p = trial % 4
            prefix = int(rng.integers(0, 2 ** 32)) & ~((1 << (8 * (4 - p))) - 1) & 0xFFFFFFFF   # higher bytes set only
            d = int(np.searchsorted(cum, rank, side="right"))
            left, pre = _narrow(host, hist, rank, prefix, p)
            assert hist[d] > 0
            assert left == rank - (cum[d - 1] if d else 0) and 0 <= left < hist[d]
            assert pre == prefix | (d << (8 * (3 - p)))


def np_select(col, rank, host):
    """The 4-pass select on one column in numpy, narrowing through the library's own step."""
    keys = np_key(col)
    left, prefix = int(rank), 0
    for p in range(4):
        shift = 8 * (3 - p)
        m = np.ones(len(keys), bool) if p == 0 else (keys >> np.uint32(shift + 8)) == np.uint32(prefix >> (shift + 8))
        hist = np.bincount(((keys[m] >> np.uint32(shift)) & np.uint32(255)).astype(np.int64), minlength=256)
        left, prefix = _narrow(host, hist, left, prefix, p)
    return np.float32(host.vissm_host_colkey_inv(prefix))


def test_numpy_emulation_of_the_select_equals_sort(host):
    rng = np.random.default_rng(2)
    B = 257
    for name, col in data_classes(B, rng).items():
        ref = np.sort(col)
        for r in (0, 1, B // 2, B - 9, B - 2, B - 1):
            got = np_select(col, r, host)
            assert np.array_equal(np.array([got]) + np.float32(0), ref[r:r + 1] + np.float32(0), equal_nan=True), \
                (name, r, got, ref[r])
            if not np.isnan(got) and got != 0:
                assert got.view(np.uint32) == ref[r].view(np.uint32), (name, r)


def test_workspace_sizes_and_descriptor_refusals_without_gpu():
    from viforssms_amd import _lib
    lib = _lib.load()
    D = _lib.ColStatDesc
    ok = D(65536, 5001, 5001, 10)
    m, s = lib.vissm_col_moments_workspace_size(ctypes.byref(ok)), lib.vissm_col_select_workspace_size(ctypes.byref(ok))
    assert m > 0 and s > 0
    # bounded by slabs x columns, not by B x n_cols: at most 256 slabs of (2 doubles + 1 int32) per column
    assert m <= 256 * 5001 * 20 + 512 and s <= 4096
    big = D(2 ** 31 - 1, 5001, 5001, 10)
    assert 0 < lib.vissm_col_moments_workspace_size(ctypes.byref(big)) <= 256 * 5001 * 20 + 512
    assert lib.vissm_col_moments_workspace_size(ctypes.byref(D(1, 1, 1, 1))) > 0
    fake = ctypes.c_void_p(16)   # never dereferenced: the checks run first
    for bad, msg in [(D(0, 4, 4, 1), b"bad shape"), (D(4, 0, 4, 1), b"bad shape"), (D(4, 5, 4, 1), b"bad shape"),
                     (D(4, 4, 4, 0), b"n_ranks"), (D(4, 4, 4, 17), b"n_ranks")]:
        assert lib.vissm_col_moments_workspace_size(ctypes.byref(bad)) == 0
        assert msg in lib.vissm_last_error()
        assert lib.vissm_col_select_workspace_size(ctypes.byref(bad)) == 0
        assert lib.vissm_col_moments(ctypes.byref(bad), fake, fake, fake, fake, None) < 0
        assert lib.vissm_col_select_hist(ctypes.byref(bad), fake, fake, 0, fake, fake, None) < 0
        assert lib.vissm_col_select_narrow(ctypes.byref(bad), fake, fake, fake, 0, None) < 0
        assert lib.vissm_col_select_decode(ctypes.byref(bad), fake, fake, None) < 0
        assert msg in lib.vissm_last_error()
    good = D(4, 4, 4, 2)
    assert lib.vissm_col_select_hist(ctypes.byref(good), fake, fake, 4, fake, fake, None) < 0
    assert b"pass 4" in lib.vissm_last_error()
    assert lib.vissm_col_select_narrow(ctypes.byref(good), fake, fake, fake, -1, None) < 0
    assert lib.vissm_col_moments(ctypes.byref(good), None, fake, fake, fake, None) < 0
    assert b"null pointer" in lib.vissm_last_error()


def test_python_layer_refuses_bad_requests_without_gpu():
    import torch
    from viforssms_amd import _lib, ops, summary
    x = torch.zeros(8, 3)
    with pytest.raises(_lib.VissmError, match="GPU"):
        ops.col_moments(x)
    with pytest.raises(_lib.VissmError, match="GPU"):
        ops.col_order_stats(x, torch.tensor([0, 7], dtype=torch.int32))
    with pytest.raises(_lib.VissmError, match="ranks per column"):
        ops.col_order_stats(x, torch.zeros(17, dtype=torch.int32))
    with pytest.raises(ValueError):
        summary.column_summary(x, probs=[0.1] * 9)
    with pytest.raises(ValueError):
        summary.column_summary(x, probs=[1.5])
    assert ctypes.sizeof(_lib.ColStatDesc) == 16
    lib = ctypes.CDLL(HOSTCHECK)
    f = lib.vissm_host_abi_layout
    f.restype = None
    f.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]
    out = (ctypes.c_size_t * 2)()
    f(4, out)
    assert out[0] == ctypes.sizeof(_lib.ColStatDesc) and out[1] == _lib.ColStatDesc.n_ranks.offset
