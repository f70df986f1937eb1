"""numpy mirror of csrc/gpcc_rng.h, the random numbers of gpcc_sample_batch: Philox4x64-10 with key (seed, 0), the
Box-Muller normals of a draw and the row choice of a mixture draw.  Integer arithmetic in uint64 (the 64 x 64 -> 128-bit products from
32-bit halves), so the words are the header's bits; the normals use numpy's log, sqrt, cos and sin (within a few ulp of libm's)."""
import numpy as np

M0, M1 = np.uint64(0xD2E7470EE14C6C93), np.uint64(0xCA5A826395121157)
W0, W1 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBB67AE8584CAA73B)
MIXROW = (1 << 64) - 1          # the row word of the counters of mixture draws
_MASK32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _mulhilo(a, b):
    """(hi, lo) of the 128-bit product of uint64 arrays a and b."""
    a_lo, a_hi = a & _MASK32, a >> _S32
    b_lo, b_hi = b & _MASK32, b >> _S32
    ll = a_lo * b_lo
    lh = a_lo * b_hi
    hl = a_hi * b_lo
    hh = a_hi * b_hi
    mid = (ll >> _S32) + (lh & _MASK32) + (hl & _MASK32)
    hi = hh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32)
    return hi, a * b


def philox4x64(counter, key):
    """Philox4x64-10 of counters (..., 4) under keys (..., 2) (broadcast) -> uint64 words (..., 4)."""
    c = np.array(np.broadcast_to(np.asarray(counter, dtype=np.uint64), np.broadcast_shapes(np.shape(counter), np.shape(key)[:-1] + (4,))))
    k = np.array(np.broadcast_to(np.asarray(key, dtype=np.uint64), c.shape[:-1] + (2,)))
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    with np.errstate(over="ignore"):
        for r in range(10):
            if r > 0:
                k0 = k0 + W0
                k1 = k1 + W1
            hi0, lo0 = _mulhilo(M0, c0)
            hi1, lo1 = _mulhilo(M1, c2)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return np.stack([c0, c1, c2, c3], -1)


def uniform53(x):
    return (np.asarray(x, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def uniform53_open0(x):
    return ((np.asarray(x, dtype=np.uint64) >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53


STREAM_NORMALS, STREAM_PICK, STREAM_POINTS = 0, 1, 2     # word 3 of the counter: the dense normals, the row picks, the point blocks


def _blocks(seed, nb, draws, rows, stream):
    """The Box-Muller normals of the blocks 0 .. nb-1 of draws (s, m) in one stream -> array (len(draws), nb, 4)."""
    s = np.asarray(draws, dtype=np.uint64).ravel()
    m = np.broadcast_to(np.asarray(rows, dtype=np.uint64), s.shape)
    ctr = np.zeros((len(s), nb, 4), dtype=np.uint64)
    ctr[:, :, 0] = np.arange(nb, dtype=np.uint64)[None, :]
    ctr[:, :, 1] = s[:, None]
    ctr[:, :, 2] = m[:, None]
    ctr[:, :, 3] = stream
    x = philox4x64(ctr, np.array([seed, 0], dtype=np.uint64))
    z = np.empty((len(s), nb, 4))
    for p in range(2):
        u1, u2 = uniform53_open0(x[..., 2 * p]), uniform53(x[..., 2 * p + 1])
        r, th = np.sqrt(-2.0 * np.log(u1)), (2.0 * np.pi) * u2
        z[..., 2 * p] = r * np.cos(th)
        z[..., 2 * p + 1] = r * np.sin(th)
    return z


def normals(seed, T, draws, rows):
    """The standard normals of draws (s, m) -> array (len(draws), T): element j of draw s of row m from counter (j // 4, s, m, 0)
    (m = MIXROW for a mixture draw).  draws and rows are equal-length sequences (rows may be one scalar)."""
    nb = (int(T) + 3) // 4
    z = _blocks(seed, nb, draws, rows, STREAM_NORMALS)
    return z.reshape(len(z), 4 * nb)[:, :int(T)]


def point_normals(seed, points, draws, rows):
    """The normals of the linear-time draws (gpcc_sample_markov_batch) -> array (len(draws), points, 4): block e of
    draw s of row m from counter (e, s, m, 2) -- the header's normal4_stream(.., 2).  e indexes a point (training points in
    gpcc_create's order, then the test points in the caller's order, then one block for the offsets), never a merged position."""
    return _blocks(seed, int(points), draws, rows, STREAM_POINTS)


def pick_uniforms(seed, S):
    """u_s of mixture draws s = 0 .. S-1: word 0 of counter (s, 0, 2^64 - 1, 1)."""
    ctr = np.zeros((int(S), 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(int(S), dtype=np.uint64)
    ctr[:, 2] = np.uint64(MIXROW)
    ctr[:, 3] = 1
    return uniform53(philox4x64(ctr, np.array([seed, 0], dtype=np.uint64))[:, 0])


def cumulative_weights(weights):
    """c_m = c_{m-1} + w_m in row order (the header's sum)."""
    c = np.empty(len(weights))
    acc = 0.0
    for m, w in enumerate(np.asarray(weights, dtype=np.float64)):
        acc = acc + float(w)
        c[m] = acc
    return c


def pick_rows(seed, S, weights):
    """The row of each of S mixture draws: the first m with u_s c_{M-1} < c_m and w_m > 0."""
    w = np.asarray(weights, dtype=np.float64).ravel()
    c = cumulative_weights(w)
    x = pick_uniforms(seed, S) * c[-1]
    rows = np.searchsorted(c, x, side="right")
    for i in np.flatnonzero(~(w[rows] > 0.0)):            # (does not happen: c_m > c_{m-1} implies w_m > 0)
        while rows[i] < len(w) - 1 and not w[rows[i]] > 0.0:
            rows[i] += 1
    return rows.astype(np.int32)
