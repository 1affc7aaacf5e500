"""The float64 judge of the contracted occupancy march (tanh / sphere contraction, csrc/occ_grid.hip contract<> / probe<>).

Outside AABB grids the marcher's t recurrence does not depend on what is probed (hit and miss both do t0 <- t1, t1 <- t0 + dt(t0),
tm <- (t0 + t1) / 2), so a ray has ONE probe sequence, and a march through an all-ones grid with a sample cap above the longest ray
(a *trace*) lists it: one sample (t_start, t_end, ridx, gidx) per probe.  Only the cell of a probe depends on tanhf / sqrtf.  Given
the rays, the ROI, the resolution, the contraction type and a trace's public outputs, `judge` says for every probe where it lies,
which cell that is in float64, and whether float32 may legitimately put it into the neighbouring cell.  Nothing in here calls the
oracle or the library.

The probe position.  The marcher forms tm = (t0 + t1) * 0.5f (two float32 operations, repeated here in float32) and p = fmaf(tm, d,
o), rounded ONCE.  Python 3.10 has no math.fma; the single rounding comes from sphere_trace_ref.fma32 instead: the product of two
float32 is exact in float64 (48 bits), its sum with o is rounded to odd in float64 (TwoSum gives the sign of the rounding error), and
a round-to-odd value of 53 >= 2 * 24 + 2 bits rounds to the float32 the exact sum rounds to (tests/test_sphere_trace_cpu.py holds
fma32 against exact rational arithmetic).

The contracted coordinate, in float64 from that float32 p (oracle/occ_grid_oracle.c:36-54, helpers_contraction.h:10-73):
    u = (p - roi_min) / (roi_max - roi_min)
    tanh    c = tanh(u - 0.5) * 0.5 + 0.5
    sphere  v = 2 u - 1, n = |v|, v <- (2 - 1 / n) * v / n where n > 1, c = v * 0.25 + 0.5
    q = c * res, cell = clip(floor(q), 0, res - 1)        (the marcher truncates; c >= 0, so that is the floor)

The tie distance.  A probe is *undecided* on an axis when |q - round(q)| < DELTA_ULPS * 2^-24 * res index units and round(q) is an
interior face (0 < round(q) < res: at faces 0 and res the clamp puts both sides into the same cell).  DELTA_ULPS = 16 is derived,
not tuned.  h = 2^-24 is half an ulp of 1 and bounds the relative error of one correctly rounded float32 operation; the build is
-fno-fast-math -ffp-contract=off, so nothing is fused or reassociated.  c is at most 1 in magnitude, so an error of e * h in c is
e * h * res index units.
  shared   e = max - min, a = p - min, u = a / e: three roundings, |du| <= 3 h |u|.
  tanh     x = u - 0.5 rounds once more and |u| <= |x| + 0.5: |dx| <= (4 |x| + 1.5) h.  tanh damps it by sech^2(x):
           (4 |x| + 1.5) sech^2(x) <= 4 * 0.45 + 1.5 = 3.3 (x sech^2(x) <= 0.45, sech^2 <= 1).  tanhf itself: HIP documents 2 ulp,
           an ulp of a value below 1 is at most 2 h: 4 h.  (3.3 + 4) h, halved by the exact * 0.5: 3.65 h; + 0.5 rounds a value
           below 1: 0.5 h; the multiply by res: 1 h.  Fewer than 6 h.
  sphere   v = 2 u - 1 rounds once (the doubling is exact) and |u| <= (|v| + 1) / 2: |dv_i| <= (4 |v_i| + 3) h.  Inside the unit
           ball c = v / 4 + 1 / 2: 1.75 h + 0.5 h + 1 h.  Outside (n > 1): n^2 is two fmaf and a product of non-negative terms (3 h)
           of inputs with the errors above, d(n^2) <= 2 sum |v_i| |dv_i| <= (8 n^2 + 10.4 n) h, and the square root halves the
           relative error and rounds once: dn / n <= (5.5 + 5.2 / n + 1) h.  r_i = v_i / n, |r_i| <= 1: |dr_i| <= (4 + 3 / n) h +
           (6.5 + 5.2 / n) h + h = (11.5 + 8.2 / n) h.  s = 2 - 1 / n: ds <= (6.5 + 5.2 / n + 1) h / n + 2 h.  w_i = s r_i with
           s = 2 - 1 / n: |dw_i| <= s |dr_i| + ds + 2 h, which is 36.4 h at n = 1 (s = 1), 32.5 h at n = 2 and falls to 27 h as n
           grows (s -> 2 only where the 1 / n terms vanish).  c = w / 4 + 1 / 2: below 10 h; + 0.5 h + 1 h.  Fewer than 12 h.
Both stay under 16 half-ulps of 1.  A disagreement farther than that from a face is a finding about the kernel (or about this bound),
not a reason to widen DELTA_ULPS."""
import numpy as np

from sphere_trace_ref import fma32

F = np.float32
TANH, SPHERE = 1, 2
DELTA_ULPS = 16


def delta(res):
    """the tie distance per axis, in index units"""
    return DELTA_ULPS * 2.0 ** -24 * np.asarray(res, np.float64)


def probe_positions(rays_o, rays_d, t_starts, t_ends, ridx):
    """float32 [S, 3]: fmaf(tm, d, o) with tm = (t0 + t1) * 0.5f, each float32 operation rounded once"""
    t0, t1 = np.asarray(t_starts, F).reshape(-1), np.asarray(t_ends, F).reshape(-1)
    tm = (t0 + t1) * F(0.5)
    assert tm.dtype == F
    r = np.asarray(ridx).reshape(-1)
    return fma32(tm[:, None], np.asarray(rays_d, F)[r], np.asarray(rays_o, F)[r])


def contract64(p, roi, ctype):
    """-> (float64 [S, 3]: the contracted coordinate of float32 positions p, [S] bool: the sphere's n > 1 branch was taken -- None
    for tanh); roi [6] or one row [S, 6] per position"""
    p = np.asarray(p, F).astype(np.float64)
    roi = np.asarray(roi, F).astype(np.float64)
    mn, mx = roi[..., :3], roi[..., 3:]
    u = (p - mn) / (mx - mn)
    if ctype == TANH:
        return np.tanh(u - 0.5) * 0.5 + 0.5, None
    assert ctype == SPHERE, ctype
    v = u * 2.0 - 1.0
    n = np.sqrt((v * v).sum(-1, keepdims=True))
    ns = np.where(n > 1.0, n, 1.0)
    v = np.where(n > 1.0, (2.0 - 1.0 / ns) * (v / ns), v)
    return v * 0.25 + 0.5, n[:, 0] > 1.0


def judge(rays_o, rays_d, roi, res, ctype, t_starts, t_ends, ridx):
    """-> dict over the S probes of a trace:
         p [S, 3] float32     the probe position
         c, q [S, 3] float64  the contracted coordinate and c * res
         cell [S, 3] int64    clip(floor(q), 0, res - 1)
         flat [S] int64       the cell's flat index (z contiguous), without a batch offset
         undecided [S, 3]     q is within delta(res) of the interior face `face`
         face [S, 3] int64    round(q): the cell across it is face - 1 where cell == face and face where cell == face - 1
         outside [S] bool     (sphere) the n > 1 branch was taken
       roi: [6], or [S, 6] with the ROI of every probe (batched grids)"""
    res = np.asarray(res, np.int64)
    p = probe_positions(rays_o, rays_d, t_starts, t_ends, ridx)
    c, outside = contract64(p, roi, ctype)
    q = c * res.astype(np.float64)
    cell = np.clip(np.floor(q), 0, res - 1).astype(np.int64)
    face = np.rint(q).astype(np.int64)
    undecided = (np.abs(q - face) < delta(res)) & (face > 0) & (face < res)
    flat = (cell[:, 0] * res[1] + cell[:, 1]) * res[2] + cell[:, 2]
    return dict(p=p, c=c, q=q, cell=cell, flat=flat, undecided=undecided, face=face, outside=outside)


def unflatten(flat, res):
    """flat index [S] -> [S, 3]"""
    flat = np.asarray(flat, np.int64)
    return np.stack([flat // (res[1] * res[2]), flat // res[2] % res[1], flat % res[2]], 1)


def check_cells(j, gidx, res):
    """the rule of every comparison with a float32 marcher: on a decided axis the cell is the float64 cell; on an undecided axis it is
    the float64 cell or its neighbour across exactly the face within delta.  gidx [S]: flat cells without a batch offset.
    -> (bad [S] bool: the probe breaks the rule, excused [S] bool: it is allowed only thanks to a tie)"""
    got = unflatten(gidx, np.asarray(res, np.int64))
    same = got == j["cell"]
    other = np.where(j["cell"] == j["face"], j["face"] - 1, j["face"])      # the cell on the far side of the near face
    ok = same | (j["undecided"] & (got == other))
    return ~ok.all(1), ok.all(1) & ~same.all(1)


def ray_has(flag, ridx, n_rays):
    """[n_rays] bool: some probe of the ray carries the per-probe flag"""
    out = np.zeros(n_rays, bool)
    out[np.asarray(ridx).reshape(-1)[np.asarray(flag, bool)]] = True
    return out


def filter_trace(trace, grid, cap, n_rays):
    """what a march through `grid` with the sample cap `cap` must emit, given the trace (packed_info, t_starts, t_ends, ridx, [bidx,]
    gidx) of the same rays: per ray the first `cap` probes whose cell is occupied.  gidx indexes grid.ravel() (batched: with the
    entry's offset).  -> the same list of arrays"""
    pi, ridx, gidx = trace[0], trace[3], trace[-1]
    occ = np.asarray(grid, bool).ravel()[gidx]
    csum = np.cumsum(occ)
    before_ray = np.concatenate([[0], csum])[pi[:, 0]]            # occupied probes before the ray's first
    rank = csum - np.repeat(before_ray, pi[:, 1])                 # 1-based rank of an occupied probe inside its ray
    keep = occ & (rank <= cap)
    cnt = np.bincount(ridx[keep], minlength=n_rays).astype(np.int32)
    cum = np.cumsum(cnt, dtype=np.int32)
    return [np.stack([cum - cnt, cnt], 1).astype(np.int32)] + [a[keep] for a in trace[1:]]
