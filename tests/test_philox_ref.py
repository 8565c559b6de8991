"""The base noise's integer generator on the host.  tests/philox_ref.py (numpy, from the paper's definition) must
reproduce the Random123 known-answer vectors; viforssms_amd/csrc/rng_math.hpp, the code the kernels run, compiled
for the CPU into libvissm_hostcheck.so (hc_philox, hc_u01), must equal it word for word; and the reference's own
normals must look like N(0, 1) under the three keys the engine draws from (the ELBO's, the q(theta) base draw's and a
64-bit one).  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from tests import philox_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "viforssms_amd", "libvissm_hostcheck.so")

# counter, key -> output (Random123's kat_vectors for philox4x32-10)
KAT = [
    ([0x00000000] * 4, [0x00000000] * 2, [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]
THETA_XOR = 0x5DEECE66D
DIST_KEYS = [1, 1 ^ THETA_XOR, 12345678901234567]


def _host():
    lib = ctypes.CDLL(HOSTCHECK)
    lib.hc_philox.restype = None
    lib.hc_philox.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.hc_u01.restype = ctypes.c_float
    lib.hc_u01.argtypes = [ctypes.c_uint32]
    return lib


def _hc_philox(lib, ctr, key):
    """ctr [N, 4], key [N, 2] -> [N, 4] uint32, one hc_philox call per row."""
    ctr = np.ascontiguousarray(ctr, dtype=np.uint32)
    key = np.ascontiguousarray(key, dtype=np.uint32)
    out = np.zeros_like(ctr)
    pc, pk, po = ctr.ctypes.data, key.ctypes.data, out.ctypes.data
    for i in range(ctr.shape[0]):
        lib.hc_philox(pc + 16 * i, pk + 8 * i, po + 16 * i)
    return out


def test_reference_reproduces_known_answers():
    for ctr, key, want in KAT:
        got = PR.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))
        assert got.dtype == np.uint64 and [int(v) for v in got] == want, [hex(int(v)) for v in got]
    # vectorised: the three at once
    got = PR.philox4x32_10(np.array([k[0] for k in KAT]), np.array([k[1] for k in KAT]))
    assert np.array_equal(got, np.array([k[2] for k in KAT], np.uint64))


def test_host_philox_known_answers():
    lib = _host()
    got = _hc_philox(lib, [k[0] for k in KAT], [k[1] for k in KAT])
    assert np.array_equal(got, np.array([k[2] for k in KAT], np.uint32)), [hex(int(v)) for v in got.ravel()]


def test_host_philox_equals_reference_on_random_blocks():
    lib = _host()
    rng = np.random.default_rng(20111112)
    N = 100_000
    ctr = rng.integers(0, 2 ** 32, (N, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, (N, 2), dtype=np.uint64)
    got = _hc_philox(lib, ctr, key)
    ref = PR.philox4x32_10(ctr, key)
    bad = np.flatnonzero((got.astype(np.uint64) != ref).any(1))
    assert bad.size == 0, (bad.size, ctr[bad[:1]], key[bad[:1]])


def test_host_philox_equals_reference_on_the_kernels_counters():
    """(g, 0, lo32(row), hi32(row)) under (lo32(seed), hi32(seed)): the first and last groups an int32 / uint32 group
    index can name, rows on both sides of 2^32 and at the top of the 64-bit range, seeds with high bits set."""
    lib = _host()
    gs = [0, 1, 2 ** 31 - 1, 2 ** 32 - 1]
    rows = [0, 1, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 7, 2 ** 63 + 1, 2 ** 64 - 1]
    seeds = [1, 2 ** 32, 0xFFFFFFFF00000001, 2 ** 64 - 1, 1 ^ THETA_XOR, 0x8000000080000000]
    ctr = np.array([[g, 0, r & 0xFFFFFFFF, r >> 32] for g in gs for r in rows for _ in seeds], np.uint64)
    key = np.array([[s & 0xFFFFFFFF, s >> 32] for _ in gs for _ in rows for s in seeds], np.uint64)
    got = _hc_philox(lib, ctr, key)
    assert np.array_equal(got.astype(np.uint64), PR.philox4x32_10(ctr, key))
    # rows 2^32 apart, and keys that differ only in their high word, give different blocks
    blocks = {tuple(b) for b in got.tolist()}
    assert len(blocks) == len(got)
    # and words() lays the counters out the same way
    for s in seeds[:4]:
        w = PR.words(s, 2 ** 32 - 3, 6, 9)
        c = np.array([[g, 0, (2 ** 32 - 3 + b) & 0xFFFFFFFF, (2 ** 32 - 3 + b) >> 32] for b in range(6)
                      for g in range(3)], np.uint64)
        k = np.tile(np.array([s & 0xFFFFFFFF, s >> 32], np.uint64), (18, 1))
        assert np.array_equal(_hc_philox(lib, c, k).astype(np.uint64).reshape(6, 3, 4), w)


def test_host_u01_is_the_exact_24_bit_uniform():
    lib = _host()
    rng = np.random.default_rng(7)
    ws = [0, 0xFF, 0x100, 0xFFFFFEFF, 0xFFFFFF00, 0xFFFFFFFF] + [int(w) for w in rng.integers(0, 2 ** 32, 20000)]
    for w in ws:
        want = ((w >> 8) + 1) / 2.0 ** 24
        got = lib.hc_u01(w)
        assert got == want and 0.0 < got <= 1.0, (hex(w), got, want)
        assert np.float32(want) == want                           # exact in fp32 as well
    assert lib.hc_u01(0) == 2.0 ** -24 and lib.hc_u01(0xFFFFFFFF) == 1.0
    assert np.array_equal(PR.uniforms(np.array(ws, np.uint64)), np.array([((w >> 8) + 1) / 2.0 ** 24 for w in ws]))


def test_reference_normals_layout():
    """normals() is the contract's layout: a shorter L is a prefix of a longer one, a later row0 a shifted block, the
    row offset wraps at 2^64, and each pair shares its radius."""
    a = PR.normals(1, 5, 7, 13)
    assert a.shape == (7, 13) and a.dtype == np.float64
    assert np.array_equal(PR.normals(1, 5, 7, 9), a[:, :9])
    assert np.array_equal(PR.normals(1, 8, 4, 13), a[3:])
    assert np.array_equal(PR.normals(1, 2 ** 64 - 2, 4, 8)[2:], PR.normals(1, 0, 2, 8))
    assert np.array_equal(PR.normals(1, 5, 7, 6, col0=7), a[:, 7:13])
    u = PR.uniforms(PR.words(1, 5, 7, 13))
    r1, r2 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    assert np.allclose(np.hypot(a[:, 0:12:4], a[:, 1:12:4]), r1[:, :3], rtol=1e-13, atol=0)
    assert np.allclose(np.hypot(a[:, 2:12:4], a[:, 3:12:4]), r2[:, :3], rtol=1e-13, atol=0)


def _dist_sample(key):
    return PR.normals_cached(key, 0, 2048, 2048)


@pytest.mark.parametrize("key", DIST_KEYS)
def test_reference_distribution(key):
    x = _dist_sample(key)
    caps, fig = PR.distribution_caps(x.size), PR.distribution_figures(x)
    print(f"key {key:#x}: " + ", ".join(f"{k} {fig[k]:.3e} (cap {caps[k]:.3e})" for k in fig))
    assert np.isfinite(x).all()
    for k, v in fig.items():
        assert v <= caps[k], (k, v, caps[k])


def test_reference_streams_of_two_keys_are_uncorrelated():
    a, b = _dist_sample(DIST_KEYS[0]), _dist_sample(DIST_KEYS[1])
    cross = abs(np.mean(a * b))
    print(f"cross-key product mean {cross:.3e} (cap {PR.distribution_caps(a.size)['cross']:.3e})")
    assert cross <= PR.distribution_caps(a.size)["cross"]
