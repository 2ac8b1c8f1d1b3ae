"""References for the posterior draws (psoap_chunk_predict_draw, psoap_draw_normals), restated from the definitions and not
from psoap_amd/csrc/draw_rng.hpp:

* Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): ten rounds of
      (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0)),
  the key bumped by the Weyl constants (W0, W1) between rounds -- in plain Python integers, and the same over NumPy arrays;
* the generator's stream: key = the two 32-bit words of the seed, counter (i >> 1, d, 0, 0) for element i of draw d, and from
  the block's words k1 = (w0 >> 5) 2^26 + (w1 >> 6), u1 = (k1 + 1) 2^-53, k2 likewise from (w2, w3), u2 = k2 2^-53,
  r = sqrt(-2 ln u1), element 2p = r cos(2 pi u2), element 2p + 1 = r sin(2 pi u2) -- in long double, the angle reduced
  exactly to the nearest quarter turn first (u2 is a dyadic rational: the reduction is exact), so that the values near the
  zeros of the cosine and sine keep their relative accuracy;
* an upper Cholesky factor and the triangular products in long double.
"""
import numpy as np

LD = np.longdouble
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
# the known-answer vector of Philox4x32-10 for an all-zero counter and key (Random123's kat_vectors)
KAT_ZERO = (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)


def philox4x32_10(counter, key):
    """plain Python integers: counter (4 words), key (2 words) -> 4 words"""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def seed_key(seed):
    return seed & MASK, (seed >> 32) & MASK


def block(seed, pair, draw):
    return philox4x32_10((pair, draw, 0, 0), seed_key(seed))


def blocks(seed, pairs, draw):
    """the same over an array of pair indices (uint64 arithmetic on 32-bit values) -> (4, len(pairs)) uint64"""
    c0 = np.asarray(pairs, dtype=np.uint64)
    c1 = np.full_like(c0, draw)
    c2 = np.zeros_like(c0)
    c3 = np.zeros_like(c0)
    k0, k1 = (np.uint64(k) for k in seed_key(seed))
    m = np.uint64(MASK)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m, (p0 >> s32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return np.stack([c0, c1, c2, c3])


def bits53(hi, lo):
    return ((hi >> 5) << 26) | (lo >> 6)


def _quarter_turns(u2):
    """cos(2 pi u2), sin(2 pi u2) in long double with the exact reduction u2 = q / 4 + r, |r| <= 1/8"""
    u2 = np.asarray(u2, dtype=np.float64)
    q = np.floor(u2 * 4.0 + 0.5)
    r = (u2 - q / 4.0).astype(LD)                     # exact: both are multiples of 2^-53 below 2
    a = r * (LD(2) * _pi_ld())
    ca, sa = np.cos(a), np.sin(a)
    k = q.astype(np.int64) % 4
    cs = np.choose(k, [ca, -sa, -ca, sa])
    sn = np.choose(k, [sa, ca, -sa, -ca])
    return cs, sn


def _pi_ld():
    """pi to the precision of long double (4 atan(1) in that arithmetic)"""
    return LD(4) * np.arctan(LD(1))


def normals(seed, D, n):
    """(D, n) long double: what psoap_draw_normals(seed, D, n) approximates in fp64"""
    out = np.empty((D, n), dtype=LD)
    npairs = (n + 1) // 2
    for d in range(D):
        w = blocks(seed, np.arange(npairs), d)
        k1, k2 = bits53(w[0], w[1]), bits53(w[2], w[3])
        u1 = (k1 + np.uint64(1)).astype(np.float64) * 2.0 ** -53      # exact
        u2 = k2.astype(np.float64) * 2.0 ** -53                       # exact
        r = np.sqrt(LD(-2) * np.log(u1.astype(LD)))
        cs, sn = _quarter_turns(u2)
        z = np.empty(2 * npairs, dtype=LD)
        z[0::2], z[1::2] = r * cs, r * sn
        out[d] = z[:n]
    return out


def cholesky_upper(A):
    """U upper, U^T U = A, in long double; LinAlgError on a pivot that is not positive"""
    U = np.array(A, dtype=LD)
    n = U.shape[0]
    for k in range(n):
        if not U[k, k] > 0:
            raise np.linalg.LinAlgError(f"pivot {k} is not positive")
        U[k, k] = np.sqrt(U[k, k])
        U[k, k + 1:] /= U[k, k]
        U[k + 1:, k + 1:] -= np.outer(U[k, k + 1:], U[k, k + 1:])
    return np.triu(U)


def gram(L):
    """L L^T in long double"""
    L = np.asarray(L, dtype=LD)
    return L @ L.T


def draws(mu, U, z):
    """mu + U^T z_d row by row, in long double: (D, R)"""
    return np.asarray(mu, dtype=LD)[None, :] + np.asarray(z, dtype=LD) @ np.asarray(U, dtype=LD)
