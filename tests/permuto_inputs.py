"""Input families, float64 references and comparison functions of the permutohedral encoder's table tests: shared by
tests/test_permuto_table_gpu.py (the kernels against the restatement) and tests/test_permuto_inputs_cpu.py (the restatement alone
proves that the inputs reach what they claim, and that the comparison functions catch a wrong tie-break or a dropped `sum`
correction).

Families of points, N = 300 each (one full 256-thread block plus a partial one, no multiple of 64), two levels of resolutions
[4, 37]:
  face   no shifts; point i has i mod 4 non-zero coordinates (at most D) at random positions, values in (-3, 3); in every second
         point with two or more of them, two are equal; i mod 4 == 0 is the origin.  A point with one non-zero coordinate j has
         elevated coordinates 0..j equal, j+1 alone and j+2..D zero: the `elev - rem0` values tie in two groups, and the strict `<`
         of the rank comparison (permuto_cuda.h:245) decides the simplex, hence dL/dx and dL/d(dL_dy).
  half   no shifts; one non-zero coordinate x_j, a float32 neighbour of m (D+1)/2 / scale_j (m odd) with fl(x_j scale_j) ==
         m (D+1)/2 exactly, so that `up - elev == elev - down` in the rounding to the nearest remainder-0 point
         (permuto_cuda.h:230).  No claim is made for this family: flipping that tie changes no row of y, dL/dx or dL/dparam (the
         `sum` correction brings either choice to the same simplex); the rows are plain coverage of the comparison.
  wide   no shifts; uniform in (-8, 8): negative elevated coordinates (floorf below zero) and a non-zero `sum` correction.
  table  the points of the every-table-entry test: 150 rows uniform in [0, 1), 150 rows `wide`, per-level Gaussian shifts.
"""
import contextlib
import functools

import torch

import permuto_ref as R
from test_permuto_gpu import HALF_TOL, _rowcheck
from util import assert_close

N = 300
RES = [4.0, 37.0]
TABLE = 509                               # prime, smaller than N (D + 1): rows collide
WIDTHS = {2: [2, 4], 4: [4, 4]}           # pseudo-level width -> n_feats (width 2: the second level walks two chunks)
FAMILIES = ["face", "half", "wide", "table"]
FACE_DIMS = [2, 3, 4, 7, 16, 17, 24, 64]  # both sides of the unroll boundary (vertex loops unrolled up to D = 16)
DTYPES = [torch.float32, torch.float16]
# every (D, width, dtype) the library compiles; each case of the every-table-entry test launches its four kernels
TABLE_CASES = [(D, w, dt) for D in R.SUPPORTED for w in sorted(WIDTHS) for dt in DTYPES]
QUANTITIES = ["y", "dL_dx", "dL_dparam", "dL_ddLdy", "dL_dparam2"]


def scales_of(meta):
    return torch.tensor(meta["level_scales_multidim"], dtype=torch.float32)


def face(D, g, n=N):
    x = torch.zeros(n, D)
    for i in range(n):
        k = min(i % 4, D)
        if k == 0:
            continue
        idx = torch.randperm(D, generator=g)[:k]
        v = torch.rand(k, generator=g) * 6 - 3
        if k >= 2 and (i // 4) % 2 == 1:
            v[1] = v[0]
        x[i, idx] = v
    return x


def half(D, scales, n=N):
    """point i: level l, coordinate j = divmod(i mod (L D), D), odd multiple m cycling through +-1, +-3, +-5, +-7; the float32
    neighbour of m (D+1)/2 / scale[l, j] whose product with the scale is exactly m (D+1)/2, the nearest float where none is"""
    L = scales.shape[0]
    x = torch.zeros(n, D)
    inf = torch.tensor(float("inf"))
    for i in range(n):
        lvl, j = divmod(i % (L * D), D)
        q = (i // (L * D)) % 8
        m = (2 * (q // 2) + 1) * (1 if q % 2 == 0 else -1)
        target = torch.tensor(m * (D + 1) / 2.0, dtype=torch.float32)
        s = scales[lvl, j]
        x0 = target / s
        cand = [x0, torch.nextafter(x0, inf), torch.nextafter(x0, -inf)]
        x[i, j] = next((c for c in cand if bool(c * s == target)), x0)
    return x


def wide(D, g, n=N):
    return torch.rand(n, D, generator=g) * 16 - 8


@functools.lru_cache(maxsize=None)
def case(D, width, family, size=TABLE):
    """the inputs of one case: table values and dL/dy rounded to half, so that one float64 reference serves both table dtypes"""
    g = torch.Generator().manual_seed(7919 * D + 31 * width + FAMILIES.index(family))
    r = R.create_meta(D, size, RES, WIDTHS[width])
    assert r["n_feat_per_pseudo_lvl"] == width
    sh = None
    if family == "face":
        x = face(D, g)
    elif family == "half":
        x = half(D, scales_of(r))
    elif family == "wide":
        x = wide(D, g)
    else:
        x = torch.cat([torch.rand(N // 2, D, generator=g), wide(D, g, N - N // 2)])
        sh = 10.0 * torch.randn(len(RES), D, generator=g)
    p = torch.randn(r["n_params"], generator=g).half().float()
    gy = torch.randn(N, r["n_encoded_dims"], generator=g).half().float()
    ggx = torch.randn(N, D, generator=g)
    return dict(D=D, width=width, family=family, size=size, meta=r, x=x, shifts=sh, p=p, gy=gy, ggx=ggx,
                levels=dict(level_offsets=r["level_offsets"], n_params=r["n_params"]))


def compute_reference(meta, x, p, gy, ggx, shifts, **kw):
    """float64 y, dL/dx, dL/dparam and the double backward's dL/d(dL_dy), dL/dparam from the restatement (kw: R.encode's batching
    and max_level arguments)"""
    x64 = x.double().requires_grad_(True)
    p64 = p.double().requires_grad_(True)
    gy64 = gy.double().requires_grad_(True)
    y = R.encode(meta, x, p64, shifts=shifts, x64=x64, **kw)
    nab, dp = torch.autograd.grad(y, [x64, p64], gy64, create_graph=True)
    ggy, dp2 = torch.autograd.grad((nab * ggx.double()).sum(), [gy64, p64])
    return {"y": y.detach(), "dL_dx": nab.detach(), "dL_dparam": dp.detach(), "dL_ddLdy": ggy, "dL_dparam2": dp2}


@functools.lru_cache(maxsize=None)
def reference(D, width, family, size=TABLE):
    c = case(D, width, family, size)
    return compute_reference(c["meta"], c["x"], c["p"], c["gy"], c["ggx"], c["shifts"])


@contextlib.contextmanager
def simplex_replaced(fn):
    """the restatement with another `simplex` (a mutant standing in for a wrong kernel)"""
    orig = R.simplex
    R.simplex = fn
    try:
        yield
    finally:
        R.simplex = orig


def tol_of(dtype):
    return HALF_TOL if dtype == torch.float16 else 1e-5


def compare(name, got, want, dtype, levels=None, tag=""):
    """one quantity against the restatement, to the bounds of tests/test_permuto_gpu.py: 1e-5 (float32) or HALF_TOL (half) of the
    column scale, of the level scale for the parameter gradients; dL/dx 1e-5 / 2e-5.  Per-point quantities row by row first: every
    row off the restatement is counted, none is excused."""
    tol = tol_of(dtype)
    if name == "dL_dx":
        tol = 2e-5 if dtype == torch.float16 else 1e-5
    got = got.detach().float() if got.dtype == torch.float16 else got.detach()
    if name.startswith("dL_dparam"):
        assert_close(got, want.numpy(), rel=tol, name=f"{name} {tag}", levels=levels)
    else:
        _rowcheck(f"{name} {tag}", got, want, tol)
        assert_close(got, want.numpy(), rel=tol, name=f"{name} {tag}")


def compare_all(got, want, dtype, levels, tag="", names=QUANTITIES):
    for name in names:
        compare(name, got[name], want[name], dtype, levels, tag)
