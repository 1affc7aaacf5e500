"""numpy float64 restatement of the Lipschitz weight normalisation (csrc/mlp_lipschitz.hip; the reference's LipshitzMLP.normalization,
nr3d_lib/models/blocks/mlp.py:214-220) and of its gradient, and the builder of the lattice inputs on which every intermediate is exact
in float32 in ANY summation order -- so kernel, torch chain and restatement must agree bit for bit there.

    sp = softplus(c) (beta 1, threshold 20),  a_r = sum_j |W[r, j]|,  den_r = max(a_r, sp),  W~[r, j] = W[r, j] sp / den_r
    S_r = sum_j G[r, j] W[r, j],  pass_r = a_r >= sp
    dL/dW[r, j] = G[r, j] sp / den_r - (pass_r ? sign(W[r, j]) S_r sp / den_r^2 : 0),   dL/dc = sigmoid(c) sum_r S_r / den_r

The lattice: weights are multiples of 1/8 whose row abs-sums are drawn per row from ABS_SUMS = {5.5, 16, 32, 64, 128, 0} (clamped rows, the
tie a == sp, scaled rows, the zero row), c = 32 (softplus(32) == 32 by the threshold, sigmoid(32) == 1 in float32), G = +- 2^-2 .. 2^2.
Scales are 1, 1/2, 1/4; every product and partial sum is a multiple of 2^-14 below 2^11: exact in float32 (and W, W~ in half)."""
import numpy as np

ABS_SUMS = (5.5, 16.0, 32.0, 64.0, 128.0, 0.0)
LATTICE_C = 32.0
LATTICE_SHAPES = ((1, 1), (3, 3), (64, 35), (64, 64), (3, 65), (130, 128), (5, 257))      # (rows, cols)
LATTICE_COLS = (1, 3, 35, 64, 65, 128, 257)


def softplus(c):
    c = np.asarray(c, np.float64)
    with np.errstate(over="ignore"):
        return np.where(c > 20.0, c, np.log1p(np.exp(np.minimum(c, 50.0))))


def sigmoid(c):
    c = np.asarray(c, np.float64)
    with np.errstate(over="ignore"):
        return np.where(c > 20.0, 1.0, 1.0 / (1.0 + np.exp(-c)))


def normalize(W, c):
    """W [rows, cols], scalar c -> W~ in float64"""
    W = np.asarray(W, np.float64)
    sp = softplus(c)
    den = np.maximum(np.abs(W).sum(axis=1), sp)
    return W * (sp / den)[:, None]


def normalize_backward(W, c, G):
    """-> (dL/dW [rows, cols], dL/dc scalar) in float64"""
    W, G = np.asarray(W, np.float64), np.asarray(G, np.float64)
    sp = softplus(c)
    a = np.abs(W).sum(axis=1)
    den = np.maximum(a, sp)
    S = (G * W).sum(axis=1)
    through_a = np.where((a >= sp)[:, None], np.sign(W) * (S * sp / den ** 2)[:, None], 0.0)
    return G * (sp / den)[:, None] - through_a, float(sigmoid(c) * (S / den).sum())


def lattice_layer(rng, rows, cols):
    """(W, G) float32 [rows, cols]: row r has abs-sum ABS_SUMS[k_r] -- the first rows walk through ABS_SUMS in order (every shape with six
    rows has every kind), the others draw from it -- split at random over the columns in units of 1/8, random signs"""
    W = np.zeros((rows, cols), np.float64)
    for r in range(rows):
        target = ABS_SUMS[r % len(ABS_SUMS)] if r < len(ABS_SUMS) else ABS_SUMS[int(rng.integers(len(ABS_SUMS)))]
        units = rng.multinomial(int(round(target * 8)), np.full(cols, 1.0 / cols))
        W[r] = units / 8.0 * rng.choice([-1.0, 1.0], size=cols)
    G = rng.choice([-1.0, 1.0], size=(rows, cols)) * 2.0 ** rng.integers(-2, 3, size=(rows, cols))
    assert np.array_equal(W, W.astype(np.float16).astype(np.float64))
    return W.astype(np.float32), G.astype(np.float32)


def lattice_network(seed=0, shapes=LATTICE_SHAPES):
    """([W_l], [G_l], c [n_layers]) float32"""
    rng = np.random.default_rng(seed)
    layers = [lattice_layer(rng, r, c) for r, c in shapes]
    return [w for w, _ in layers], [g for _, g in layers], np.full(len(shapes), LATTICE_C, np.float32)
