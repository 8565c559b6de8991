"""An independent numpy reference of the base-noise stream (include/vissm.h, vissm_normal_base), written from the
definition in Salmon, Moraes, Dror & Shaw, "Parallel random numbers: as easy as 1, 2, 3" (SC'11), not from the
kernel:

    Philox-4x32, one round on counter (c0, c1, c2, c3) under key (k0, k1):
        (hi0, lo0) = mulhilo(0xD2511F53, c0),   (hi1, lo1) = mulhilo(0xCD9E8D57, c2)
        (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0,  lo1,  hi0 ^ c3 ^ k1,  lo0)
    ten rounds, the key bumped by the Weyl constants (0x9E3779B9, 0xBB67AE85) between rounds (nine bumps).

The library's contract on top of it: group g = j // 4 of row r is philox(ctr = (g, 0, lo32(r), hi32(r)),
key = (lo32(seed), hi32(seed))); a word w becomes u = ((w >> 8) + 1) * 2^-24 in (0, 1] (exact in fp32 and float64
alike, so this reference and the kernel start Box-Muller from identical uniforms); columns 4g .. 4g+3 are
(r1 cos 2 pi u_y, r1 sin 2 pi u_y, r2 cos 2 pi u_w, r2 sin 2 pi u_w) with r1 = sqrt(-2 ln u_x), r2 = sqrt(-2 ln u_z).

Everything is carried in uint64 arrays masked to 32 bits, so no intermediate wraps silently."""
import functools

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
MUL0, MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
WEYL0, WEYL1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
SH32 = np.uint64(32)
ROUNDS = 10


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (broadcast against each other in the leading dimensions), 32-bit values in any
    integer type -> the output block [..., 4] as uint64 holding 32-bit words."""
    ctr = np.asarray(ctr).astype(np.uint64) & M32
    key = np.asarray(key).astype(np.uint64) & M32
    c0, c1, c2, c3 = (ctr[..., i] for i in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    for rnd in range(ROUNDS):
        if rnd:
            k0, k1 = (k0 + WEYL0) & M32, (k1 + WEYL1) & M32
        p0, p1 = MUL0 * c0, MUL1 * c2                 # 32 x 32 bits: exact in 64
        c0, c1, c2, c3 = (p1 >> SH32) ^ c1 ^ k0, p1 & M32, (p0 >> SH32) ^ c3 ^ k1, p0 & M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1)


def words(seed, row0, B, L, g0=0):
    """The Philox words behind normal_base(seed, row0, B, L): uint64 [B, ceil(L / 4), 4], word order x, y, z, w
    (g0: the first group, for columns far from the origin)."""
    seed, row0 = int(seed) & (2 ** 64 - 1), int(row0) & (2 ** 64 - 1)
    G = (L + 3) // 4
    rows = np.array([(row0 + b) & (2 ** 64 - 1) for b in range(B)], dtype=np.uint64)      # wraps like uint64_t
    ctr = np.zeros((B, G, 4), np.uint64)
    ctr[..., 0] = np.arange(g0, g0 + G, dtype=np.uint64)[None, :]
    ctr[..., 2] = (rows & M32)[:, None]
    ctr[..., 3] = (rows >> SH32)[:, None]
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    return philox4x32_10(ctr, key)


def uniforms(w):
    """u = ((w >> 8) + 1) * 2^-24 in float64: a multiple of 2^-24 in (0, 1], so exactly representable in fp32 too."""
    return ((np.asarray(w, np.uint64) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24


def box_muller(u, dtype=np.float64):
    """u [..., 4] (x, y, z, w) -> the four normals [..., 4], every operation in `dtype`."""
    u = np.asarray(u).astype(dtype)
    two_pi, m2 = dtype(2.0 * np.pi), dtype(-2.0)
    r1, r2 = np.sqrt(m2 * np.log(u[..., 0])), np.sqrt(m2 * np.log(u[..., 2]))
    a1, a2 = two_pi * u[..., 1], two_pi * u[..., 3]
    return np.stack([r1 * np.cos(a1), r1 * np.sin(a1), r2 * np.cos(a2), r2 * np.sin(a2)], -1).astype(dtype)


def normals(seed, row0, B, L, dtype=np.float64, col0=0):
    """The [B, L] array vissm_normal_base(seed, row0, ., ., B, L, .) promises, in float64 (dtype = np.float32: the
    same Box-Muller restated in numpy float32 arithmetic, from the same exact uniforms).  col0 > 0: columns
    col0 .. col0 + L - 1 of a longer row."""
    g0, skip = col0 // 4, col0 % 4
    v = box_muller(uniforms(words(seed, row0, B, L + skip, g0)), dtype)
    return np.ascontiguousarray(v.reshape(B, -1)[:, skip:skip + L])


@functools.lru_cache(maxsize=8)
def normals_cached(seed, row0, B, L, dtype=np.float64):
    """normals() computed once per session and handed out read-only (the 2048 x 2048 samples of the distribution
    conditions, shared by the host and the device tests)."""
    a = normals(seed, row0, B, L, dtype)
    a.setflags(write=False)
    return a


# ----------------------------------------------------------------------------------------------------------------
# the distribution conditions of a [B, L] sample, n = B L; every figure is compared against its cap by the caller
# ----------------------------------------------------------------------------------------------------------------
def distribution_caps(n):
    """Caps at four standard errors of each estimator under N(0, 1) (var x = 1, var x^2 = 2, var x^3 = 15,
    var x^4 = 96, var of a product of independent normals = 1) and the Kolmogorov-Smirnov statistic's 1 % point."""
    s = np.sqrt(n)
    return {"ks": 1.63, "mean": 4.0 / s, "var": 4.0 * np.sqrt(2.0 / n), "m3": 4.0 * np.sqrt(15.0 / n),
            "m4": 4.0 * np.sqrt(96.0 / n), "lag_col": 4.0 / s, "lag_row": 4.0 / s, "cross": 4.0 / s}


def distribution_figures(x):
    """|figure| per condition of distribution_caps for a float64 [B, L] array (numpy)."""
    n = x.size
    flat = np.sort(x.reshape(-1))
    cdf = 0.5 * (1.0 + _erf(flat / np.sqrt(2.0)))
    i = np.arange(1, n + 1, dtype=np.float64)
    D = max(np.max(i / n - cdf), np.max(cdf - (i - 1.0) / n))
    m = x.mean()
    return {"ks": D * np.sqrt(n), "mean": abs(m), "var": abs(np.mean((x - m) ** 2) - 1.0), "m3": abs(np.mean(x ** 3)),
            "m4": abs(np.mean(x ** 4) - 3.0), "lag_col": abs(np.mean(x[:, :-1] * x[:, 1:])),
            "lag_row": abs(np.mean(x[:-1] * x[1:]))}


def _erf(z):
    """erf in float64 without scipy: torch's CPU erf (the test environment always has torch)."""
    import torch
    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(z, dtype=np.float64))).numpy()
