"""Host reference of the seeded particle draws ("Device draws"): Philox4x32-10 (Salmon, Moraes, Dror & Shaw 2011)
vectorised in NumPy with uint64 arithmetic, and the map from a Philox block to a pair of doubles.

Addressing: the key is (seed & 0xffffffff, seed >> 32); the counter of pair p of the block of (group g, record r) of a stream is
(p, g, r, stream) with stream 0 eps, 1 unif, 2 xi0, 3 unif_bs; g and r are 0 where the noise mode shares that axis.  Pair p gives the
elements 2p and 2p + 1 of the block (eps [steps][N][D], unif [steps], xi0 [N][D], unif_bs [steps][B]); the second is dropped when the
block length is odd.  From the four words w0..w3: k1 = (w0 >> 5) 2^26 + (w1 >> 6), k2 = (w2 >> 5) 2^26 + (w3 >> 6), both < 2^53.
Uniform streams: k1 2^-53, k2 2^-53.  Normal streams: u1 = (k1 + 1) 2^-53, u2 = k2 2^-53, rho = sqrt(-2 ln u1), the elements
rho cos(2 pi u2) and rho sin(2 pi u2)."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
STREAMS = {"eps": 0, "unif": 1, "xi0": 2, "unif_bs": 3}
NORMAL = ("eps", "xi0")
NOISE = ("shared", "per_record", "independent")
TWO53 = 2.0 ** -53


def philox4x32(counter, key, rounds=10):
    """counter: four uint64 arrays of 32-bit words (broadcastable), key: two of them -> the four output words as uint64 arrays"""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & MASK for c in counter)
    k0, k1 = (np.asarray(k, np.uint64) & MASK for k in key)
    for i in range(rounds):
        p0, p1 = M0 * c0, M1 * c2                                  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        if i + 1 < rounds:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def pair_integers(seed, stream, g, r, p):
    """(k1, k2) of the pairs p (an integer array) of the block of (g, r): uint64 arrays below 2^53"""
    seed = int(seed)
    assert 0 <= seed < 2 ** 64
    p = np.asarray(p, np.uint64)
    z = np.zeros_like(p)
    w0, w1, w2, w3 = philox4x32((p, z + np.uint64(g), z + np.uint64(r), z + np.uint64(stream)),
                                (np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)))
    sh5, sh6, sh26 = np.uint64(5), np.uint64(6), np.uint64(26)
    return ((w0 >> sh5) << sh26) + (w1 >> sh6), ((w2 >> sh5) << sh26) + (w3 >> sh6)


def uniform_pair(k1, k2):
    return k1.astype(np.float64) * TWO53, k2.astype(np.float64) * TWO53


def normal_pair(k1, k2, dtype=np.float64):
    """The normal map of the pairs in `dtype` (np.float64: the reference; np.longdouble: what both are judged against)"""
    one, two = dtype(1), dtype(2)
    pi = dtype(4) * np.arctan(one)
    u1 = (k1.astype(dtype) + one) * dtype(TWO53)
    u2 = k2.astype(dtype) * dtype(TWO53)
    rho = np.sqrt(-two * np.log(u1))
    a = two * pi * u2
    return rho * np.cos(a), rho * np.sin(a)


def block(seed, name, g, r, length, dtype=np.float64):
    """The `length` elements of the block of (g, r) of stream `name`, flat"""
    k1, k2 = pair_integers(seed, STREAMS[name], g, r, np.arange((length + 1) // 2))
    a, b = normal_pair(k1, k2, dtype) if name in NORMAL else uniform_pair(k1, k2)
    out = np.empty(2 * a.size, a.dtype)
    out[0::2], out[1::2] = a, b
    return out[:length]


def lead_shape(noise, G, R):
    return {"shared": (), "per_record": (R,), "independent": (G, R)}[noise]


def draws(seed, noise, G, R, steps, N, D, with_xi0=False, B=0, dtype=np.float64):
    """The dict of prediction.particle_draws: eps lead + (steps, N, D), unif lead + (steps,), xi0 lead + (N, D), unif_bs
    lead + (steps, B)"""
    assert noise in NOISE
    lead = lead_shape(noise, G, R)
    shapes = {"eps": (steps, N, D), "unif": (steps,)}
    if with_xi0:
        shapes["xi0"] = (N, D)
    if B:
        shapes["unif_bs"] = (steps, B)
    out = {}
    for name, shp in shapes.items():
        n = int(np.prod(shp))
        arr = np.empty(lead + (n,), np.float64 if name not in NORMAL else dtype)
        for idx in np.ndindex(*lead):
            g, r = {0: (0, 0), 1: (0,) + idx, 2: idx}[len(idx)]
            arr[idx] = block(seed, name, g, r, n, dtype)
        out[name] = arr.reshape(lead + shp)
    return out
