"""A numpy restatement of csrc/importance.hip (include/nr3d_hip.h states the order of every operation): the update with Python-int fixed
point, the Kogge-Stone-with-carry scan in float32, the three lower-bound searches.  Every float32 operation is rounded once, as the
kernels round (no contraction).  tests/test_importance_cpu.py pins it on literals written out by hand; the GPU tests compare bytes."""
import math

import numpy as np

F = np.float32
CHUNK = 2 ** 15


# ---- update ----------------------------------------------------------------------------------------------------------------------
def corners(i, xy, val, N, H, W):
    """per sample: None (dropped) or ([flat cell] * 4, [float32 contribution] * 4), in the order (h, w), (h+1, w), (h, w+1), (h+1, w+1)"""
    xy = np.asarray(xy, F).reshape(-1, 2)
    val = np.asarray(val, F).reshape(-1)
    n = val.shape[0]
    frames = np.full(n, i, np.int64) if np.ndim(i) == 0 else np.asarray(i, np.int64).reshape(-1)
    out = []
    one = F(1)
    for s in range(n):
        f, x, y, v = int(frames[s]), xy[s, 0], xy[s, 1], val[s]
        if f < 0 or f >= N or not (np.isfinite(x) and np.isfinite(y) and np.isfinite(v)) or v < 0:
            out.append(None)
            continue
        with np.errstate(over="ignore"):
            wf, hf = F(x * F(W)), F(y * F(H))
        if not (np.isfinite(wf) and np.isfinite(hf)):
            out.append(None)
            continue
        wt, ht = np.trunc(wf), np.trunc(hf)
        w_w, w_h = F(wf - wt), F(hf - ht)
        w, h = int(min(max(wt, 0), W - 2)), int(min(max(ht, 0), H - 2))
        base = (f * H + h) * W + w
        c = [F(F(F(one - w_h) * F(one - w_w)) * v), F(F(w_h * F(one - w_w)) * v), F(F(F(one - w_h) * w_w) * v), F(F(w_h * w_w) * v)]
        out.append(([base, base + W, base + 1, base + W + 1], c))
    return out


def fix(c):
    """a float32 contribution as a signed integer of 2^-32 units: |c| clamped to 2^16, round half to even"""
    c = float(min(max(F(c), F(-65536.0)), F(65536.0)))
    return round(c * 4294967296.0)          # exact product (a float32 times a power of two), Python rounds half to even as llrint does


def unfix(q):
    """float(double(q) * 2^-32): int -> double rounds to nearest even, as the conversion of an int64 does"""
    return F(float(q) * (1.0 / 4294967296.0))


def update(error_map, i, xy, val, return_counts=False):
    """the fused update: per chunk of 2^15 samples, integer sums per cell, then map[cell] = map[cell] + unfix(sum) for every cell whose
    sum is not 0.  Returns a new map (and, with return_counts, the number of contributions and their exact float64 sum per cell)."""
    m = np.array(error_map, F, copy=True)
    N, H, W = m.shape
    flat = m.reshape(-1)
    cs = corners(i, xy, val, N, H, W)
    counts = np.zeros(flat.shape[0], np.int64)
    exact = np.zeros(flat.shape[0], np.float64)
    for b in range(0, len(cs), CHUNK):
        acc = {}
        for c in cs[b:b + CHUNK]:
            if c is None:
                continue
            for cell, v in zip(*c):
                q = fix(v)
                if q:
                    acc[cell] = acc.get(cell, 0) + q
                counts[cell] += 1
                exact[cell] += float(v)
        for cell, q in acc.items():
            if q:
                flat[cell] = F(flat[cell] + unfix(q))
    if return_counts:
        return m, counts.reshape(m.shape), exact.reshape(m.shape)
    return m


def cells_touched_twice(i, xy, val, N, H, W):
    """True when two (sample, corner) pairs of the call share a cell -- where the reference's update is undefined"""
    seen = set()
    for c in corners(i, xy, val, N, H, W):
        if c is None:
            continue
        for cell in c[0]:
            if cell in seen:
                return True
            seen.add(cell)
    return False


def lattice_update(N, H, W, seed, per_sample_frames):
    """collision-free lattice inputs -> (i, xy, val): one sample per 2 x 2 block of cells, xy in multiples of 1 / (4 res), val in
    multiples of 2^-10 below 4.  Only positions whose float32 product with the resolution is the lattice value itself are kept (for a
    resolution that is no power of two, x = k / (4 res) is rounded and x * res may miss k / 4 by an ulp), so that every weight is a
    multiple of 1/4 and every contribution a multiple of 2^-14: exact in float32 and in the 2^-32 fixed point."""
    rng = np.random.default_rng(seed)

    def coord(cell, res):
        for q in rng.permutation(4):
            k = cell * 4 + int(q)
            x = F(k / (4.0 * res))
            if float(F(x * F(res))) * 4 == k:
                return x
        return None
    f, xy = [], []
    for fr in range(N if per_sample_frames else 1):
        for h in range(0, H - 1, 2):
            for w in range(0, W - 1, 2):
                x, y = coord(w, W), coord(h, H)
                if x is not None and y is not None:
                    f.append(fr)
                    xy.append((x, y))
    order = rng.permutation(len(f))
    f, xy = np.array(f, np.int64)[order], np.array(xy, F).reshape(-1, 2)[order]
    val = (rng.integers(0, 4096, len(f)) / 1024.0).astype(F)
    return (f if per_sample_frames else 0), xy, val


# ---- construct_cdf ---------------------------------------------------------------------------------------------------------------
def scan(v):
    """float32 [..., L] -> the inclusive scan along the last axis in the kernels' order: 64-element chunks, Kogge-Stone inside a chunk
    (steps 1 .. 32, all elements at once), then the carry (the previous chunk's last result, 0 before the first) added to every element"""
    v = np.asarray(v, F)
    L = v.shape[-1]
    out = np.empty_like(v)
    carry = np.zeros(v.shape[:-1], F)
    for b in range(0, L, 64):
        c = np.zeros(v.shape[:-1] + (64,), F)
        c[..., :min(64, L - b)] = v[..., b:b + 64]
        off = 1
        while off < 64:
            nxt = c.copy()
            nxt[..., off:] = c[..., off:] + c[..., :-off]
            c = nxt
            off *= 2
        c = (c + carry[..., None]).astype(F)
        carry = c[..., min(64, L - b) - 1].copy()      # the chunk's last ELEMENT (the row's end in the last chunk)
        out[..., b:b + 64] = c[..., :min(64, L - b)]
    return out, carry


def norm(c, total, min_pdf):
    a, b = F(1 - min_pdf), F(min_pdf)            # the Python doubles, rounded once
    L = c.shape[-1]
    ramp = (np.arange(1, L + 1).astype(F) / F(L)).astype(F)
    return (((a * c).astype(F) / total[..., None]).astype(F) + (b * ramp).astype(F)).astype(F)


def construct_cdf(error_map, min_pdf, max_pdf=None):
    """-> (cdf_x_cond_y, cdf_y, cdf_img, the map as construct_cdf leaves it without `clean`)"""
    e = np.array(error_map, F, copy=True)
    if max_pdf is not None:
        e = np.where(e > F(max_pdf), F(max_pdf), e).astype(F)
    c, pdf_y = scan((e + F(1e-10)).astype(F))
    cdf_x = norm(c, pdf_y, min_pdf)
    c, pdf_img = scan(pdf_y)
    cdf_y = norm(c, pdf_img, min_pdf)
    c, total = scan(pdf_img[None])
    cdf_img = norm(c, total, min_pdf)[0]
    return cdf_x, cdf_y, cdf_img, e


def construct_cdf_f64(error_map, min_pdf, max_pdf=None):
    """the same quantities evaluated in float64 from the float32 inputs"""
    e = np.asarray(error_map, F).astype(np.float64)
    if max_pdf is not None:
        e = np.minimum(e, float(F(max_pdf)))
    a, b = float(F(1 - min_pdf)), float(F(min_pdf))

    def nrm(c):
        L = c.shape[-1]
        return a * c / c[..., -1:] + b * (np.arange(1, L + 1) / L)
    cx = np.cumsum(e + float(F(1e-10)), axis=2)
    cy = np.cumsum(cx[:, :, -1], axis=1)
    ci = np.cumsum(cy[:, -1])
    return nrm(cx), nrm(cy), nrm(ci)


# ---- sampling --------------------------------------------------------------------------------------------------------------------
def lower(row, u):
    """min(the first k with row[k] >= u, len - 1)"""
    lo, hi = 0, len(row)
    while lo < hi:
        mid = (lo + hi) >> 1
        if row[mid] < u:
            lo = mid + 1
        else:
            hi = mid
    return min(lo, len(row) - 1)


def invert(row, u):
    k = lower(row, u)
    prev = row[k - 1] if k > 0 else F(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return k, F(F(F(F(u - prev) / F(row[k] - prev)) + F(k)) / F(len(row)))


def sample(cdf_img, cdf_y, cdf_x_cond_y, frame_ind, u_img, u_x, u_y):
    """-> (i int64 [n], xy float32 [n, 2]); frame_ind None (searched in cdf_img), an int or an array"""
    n = len(u_x)
    N = cdf_y.shape[0]
    i = np.empty(n, np.int64)
    xy = np.empty((n, 2), F)
    for s in range(n):
        if frame_ind is None:
            f = lower(cdf_img, F(u_img[s]))
        else:
            f = int(frame_ind if np.ndim(frame_ind) == 0 else frame_ind[s])
            f = min(max(f + N if f < 0 else f, 0), N - 1)
        h, y = invert(cdf_y[f], F(u_y[s]))
        _, x = invert(cdf_x_cond_y[f, h], F(u_x[s]))
        i[s], xy[s, 0], xy[s, 1] = f, x, y
    return i, xy
