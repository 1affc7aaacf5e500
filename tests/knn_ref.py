"""tests/knn_ref.py -- the k-NN contract of include/nr3d_hip.h (nr3d_knn_points, nr3d_knn_points_backward) restated in numpy, written from
the contract, and the two input generators of the k-NN tests.

Forward: per-dimension float32 differences; norm 2 accumulates d_0 * d_0 and then fmaf(d_c, d_c, dist) -- the fmaf as one float64
multiply-add rounded to float32 (the product of two float32 is exact in float64; the float64 sum is rounded once more, a double rounding
that the lattice never meets and the float tests allow for in their bound) -- norm 1 accumulates |d_c| in float32.  Selection:
``np.lexsort((j, dist))``, the first min(K, lengths2[n]) pairs, zeros after them and in the rows past lengths1[n].
Backward: float64; an idx outside [0, P2) is skipped, as the contract says (no term in either gradient).

lattice(): coordinates k / 256 with integer |k| <= kmax and D (2 kmax)^2 <= 2^24: every difference, square and partial sum is exact in
float32, so the fmaf chain, separate multiply-add and float64 give the same bits, and the lattice is full of ties.
normal(): standard normal float32; distances are judged against float64 within dist_bound()."""
import numpy as np

EPS = 2.0 ** -24


def lattice_kmax(D):
    """the largest power of two kmax with D (2 kmax)^2 <= 2^24"""
    k = 1
    while D * (4 * k) ** 2 <= 2 ** 24:
        k *= 2
    return k


def lattice(rng, shape, kmax=None):
    D = shape[-1]
    kmax = lattice_kmax(D) if kmax is None else kmax
    assert D * (2 * kmax) ** 2 <= 2 ** 24
    return (rng.integers(-kmax, kmax + 1, size=shape).astype(np.float32) / np.float32(256)).astype(np.float32)


def normal(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def wild_lengths(rng, N, P, at=0):
    """int64 [N]: -5, P, P + 1, -1, 2^40, INT64_MIN, INT64_MAX and 0 in the clouds at .. at + 7, random values of [1, P] in the others;
    the contract clamps each into [0, P].  lengths1 with at = 0 and lengths2 with at = 8 put every wild value of one beside a live
    value of the other."""
    assert N >= 8 + at
    l = rng.integers(1, P + 1, N).astype(np.int64)
    l[at:at + 8] = [-5, P, P + 1, -1, 2 ** 40, I64_MIN, I64_MAX, 0]
    return l


def spoil_idx(rng, idx, P2, share=0.1):
    """a copy of idx with about `share` of its entries replaced by -1, P2, P2 + 7 and 2^40, none of them an index of knn_points, and the
    bool mask of the replaced entries"""
    bad = rng.random(idx.shape) < share
    out = idx.copy()
    out[bad] = rng.choice(np.array([-1, P2, P2 + 7, 2 ** 40], np.int64), int(bad.sum()))
    return out, bad


def directed_p2(D, order, P2=1025):
    """float32 [P2, D] that varies in coordinate 0 only, k / 256 with 0 <= k < P2, the other coordinates 0.  Against a query whose
    coordinate 0 is <= 0 the distance grows with k, so: "descending": k = P2 - 1 - j, every candidate is the nearest so far (enters at
    slot 0 and shifts the whole list); "ascending": k = j, nothing enters once the list is full; "alternating": far, near, far, ...
    (k = P2 - 1 - j / 2 for even j, (j - 1) / 2 for odd j); "equal": every point the same (k = 3)"""
    j = np.arange(P2)
    k = {"descending": P2 - 1 - j, "ascending": j, "alternating": np.where(j % 2 == 0, P2 - 1 - j // 2, (j - 1) // 2),
         "equal": np.full(P2, 3)}[order]
    p2 = np.zeros((P2, D), np.float32)
    p2[:, 0] = k.astype(np.float32) / np.float32(256)
    return p2


def dist_bound(D, dist):
    """|float32 chain - float64| <= (D + 4) 2^-24 dist: one rounding of each difference, squared, plus one rounding per accumulation
    step of non-negative terms"""
    return (D + 4) * EPS * dist


def _lengths(lengths, N, P):
    return np.full(N, P, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, P)


def pair_dists(a, b, norm):
    """a float32 [P1, D], b float32 [P2, D] -> float32 [P1, P2] by the contract's arithmetic"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d = a[:, None, 0] - b[None, :, 0]
    dist = (d * d if norm == 2 else np.abs(d)).astype(np.float32)
    for c in range(1, a.shape[1]):
        d = (a[:, None, c] - b[None, :, c]).astype(np.float32)
        if norm == 2:
            dist = (d.astype(np.float64) * d.astype(np.float64) + dist.astype(np.float64)).astype(np.float32)
        else:
            dist = (dist + np.abs(d)).astype(np.float32)
    return dist


def pair_dists64(a, b, norm):
    d = np.asarray(a, np.float64)[:, None, :] - np.asarray(b, np.float64)[None, :, :]
    return (d * d).sum(-1) if norm == 2 else np.abs(d).sum(-1)


def knn_points(p1, p2, lengths1=None, lengths2=None, norm=2, K=1):
    """-> (idx int64 [N, P1, K], dists float32 [N, P1, K])"""
    p1, p2 = np.asarray(p1, np.float32), np.asarray(p2, np.float32)
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    l1, l2 = _lengths(lengths1, N, P1), _lengths(lengths2, N, P2)
    idx = np.zeros((N, P1, K), np.int64)
    dists = np.zeros((N, P1, K), np.float32)
    for n in range(N):
        n1, n2 = int(l1[n]), int(l2[n])
        k = min(K, n2)
        if n1 == 0 or k == 0:
            continue
        dm = pair_dists(p1[n, :n1], p2[n, :n2], norm)
        order = np.lexsort((np.broadcast_to(np.arange(n2), dm.shape), dm), axis=-1)[:, :k]     # by dist, equal dist by j
        idx[n, :n1, :k] = order
        dists[n, :n1, :k] = np.take_along_axis(dm, order, 1)
    return idx, dists


def knn_gather(x, idx, lengths=None):
    """x [N, M, U], idx [N, L, K] -> [N, L, K, U], zero where k >= lengths[n]"""
    x = np.asarray(x)
    N, M, U = x.shape
    K = idx.shape[2]
    out = np.zeros(idx.shape + (U,), x.dtype)
    l = _lengths(lengths, N, M)
    for n in range(N):
        k = min(K, int(l[n]))
        if M:
            out[n, :, :k] = x[n][idx[n, :, :k]]
    return out


def knn_backward(p1, p2, lengths1, lengths2, idx, norm, grad_dists):
    """float64 -> (grad_p1 [N, P1, D], grad_p2 [N, P2, D], abs_p1, abs_p2: the sums of |t| behind each element, m_p2 int64 [N, P2]: the
    number of contributions to each p2 point)"""
    p1, p2, g = np.asarray(p1, np.float64), np.asarray(p2, np.float64), np.asarray(grad_dists, np.float64)
    N, P1, D = p1.shape
    P2, K = p2.shape[1], idx.shape[2]
    l1, l2 = _lengths(lengths1, N, P1), _lengths(lengths2, N, P2)
    g1, g2 = np.zeros((N, P1, D)), np.zeros((N, P2, D))
    a1, a2 = np.zeros((N, P1, D)), np.zeros((N, P2, D))
    m2 = np.zeros((N, P2), np.int64)
    for n in range(N):
        n1, k = int(l1[n]), min(K, int(l2[n]))
        for kk in range(k):
            j = np.asarray(idx[n, :n1, kk], np.int64)
            ok = (j >= 0) & (j < P2)                               # an idx outside [0, P2) is skipped: no term in either gradient
            rows, j = np.nonzero(ok)[0], j[ok]
            diff = p1[n, rows] - p2[n, j]
            t = 2.0 * g[n, rows, kk, None] * diff if norm == 2 else g[n, rows, kk, None] * np.where(diff > 0, 1.0, -1.0)
            np.add.at(g1[n], rows, t)
            np.add.at(a1[n], rows, np.abs(t))
            np.add.at(g2[n], j, -t)
            np.add.at(a2[n], j, np.abs(t))
            np.add.at(m2[n], j, 1)
    return g1, g2, a1, a2, m2
