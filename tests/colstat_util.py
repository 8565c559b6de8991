"""Shared by the column-statistics tests (tests/test_colstat_host.py, tests/test_gpu_colstat.py): the order key in
numpy and the data classes the radix select is tried on."""
import numpy as np


def f32_from_bits(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def np_key(x):
    """The order key of include/vissm.h in numpy (uint32 keys of a float32 array): -0 -> +0, any NaN -> 0xFFFFFFFF,
    else key = (b >> 31) ? ~b : (b | 0x80000000)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    b[b == np.uint32(0x80000000)] = 0
    k = np.where(b >> np.uint32(31) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[nan] = np.uint32(0xFFFFFFFF)
    return k


SPECIAL_ROWS = [0.0, -0.0, np.inf, -np.inf, 1e-42, -1e-42, f32_from_bits(0x7FC00000), f32_from_bits(0xFFC00000)]


def data_classes(B, rng, n_cols=None):
    """name -> float32 column [B] (n_cols None) or matrix [B, n_cols], each column drawn independently:
    normal     N(10, 3^2)
    ties       integers in [-3, 3]
    equal      one value throughout
    last_byte  1 + j 2^-23, j < 200: only the key's last byte separates the values, so pass 3 decides
    mixed      both signs around 0, with +-0, +-inf, +-1e-42 (denormal) and NaNs of both signs in the first rows"""
    shape = (B,) if n_cols is None else (B, n_cols)
    mixed = (rng.standard_normal(shape) * 1e-3).astype(np.float32)
    n = min(B, len(SPECIAL_ROWS))
    sp = np.array(SPECIAL_ROWS, dtype=np.float32)[:n]
    mixed[:n] = sp if n_cols is None else sp[:, None]
    j = rng.integers(0, 200, shape)
    return {"normal": (10 + 3 * rng.standard_normal(shape)).astype(np.float32),
            "ties": rng.integers(-3, 4, shape).astype(np.float32),
            "equal": np.full(shape, 2.5, np.float32),
            "last_byte": (1 + j * 2.0 ** -23).astype(np.float32),
            "mixed": mixed}
