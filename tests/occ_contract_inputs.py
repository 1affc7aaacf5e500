"""The scenes of the contracted-march tests (tests/test_occ_contract_cpu.py pins them and the judge, tests/test_occ_contract_gpu.py
marches them on the device): defined once, shared.

  pow2      ROI [-0.5, 0.5]^3, 32^3: extents and resolution powers of two -- the multiply-only instantiation (to_unit<true>)
  non_pow2  ROI [-0.8, -0.6, -0.9, 0.7, 0.9, 0.5], (20, 24, 28): the dividing instantiation
  gamma     as non_pow2 with step 0.005, max_step 0.05, dt_gamma 0.01: a ray that starts at t = 0 steps by the lower clamp of
            calc_dt until t = 0.5 and by the upper one from t = 5 on
  outside   as pow2 with step 0.05 and the origin shifted by OUTSIDE_SHIFT: the coordinates run far outside the ROI -- tanh saturates
            into the first and the last cell, at the far end of some rays to 1.0f itself (index == res, the clamp), and the sphere's
            n > 1 branch is taken, left and taken again along a ray

Rays: pinhole_rays(20, seed=3) with far = near + 6 (the rays that miss [-1, 1]^3 start at t = 0); ray 3 axis-aligned, ray 5 with
far == near, ray 6 with near > far, the last three rays cut off (397: no multiple of 4, 16 or 256)."""
import numpy as np

from test_occ_grid_gpu import grids, pinhole_rays          # the camera and the grids of the marcher's AABB tests (plain numpy)

F = np.float32
ROI_POW2 = np.array([-0.5, -0.5, -0.5, 0.5, 0.5, 0.5], F)
ROI_NON_POW2 = np.array([-0.8, -0.6, -0.9, 0.7, 0.9, 0.5], F)
OUTSIDE_SHIFT = np.array([2.5, -1.0, 2.5], F)

SCENES = {
    # name: (roi, res, step, max_step, dt_gamma, origin shift)
    "pow2": (ROI_POW2, (32, 32, 32), 0.02, 1e10, 0.0, None),
    "non_pow2": (ROI_NON_POW2, (20, 24, 28), 0.02, 1e10, 0.0, None),
    "gamma": (ROI_NON_POW2, (20, 24, 28), 0.005, 0.05, 0.01, None),
    "outside": (ROI_POW2, (32, 32, 32), 0.05, 1e10, 0.0, OUTSIDE_SHIFT),
}
CTYPES = (1, 2)
TRACE_STEPS = 400                 # above the longest probe sequence of every scene (tests/test_occ_contract_cpu.py asserts it)
CAPS = (1, 7, 40, 64, 65, TRACE_STEPS)        # 7, 40 and 65 fall inside a look-ahead group of 16, 32 and 64 lanes
GRID_SEED = 4


def rays(shift=None):
    o, d, near, far = pinhole_rays(20, seed=3)
    far = (near + F(6.0)).astype(F)
    d[3] = np.array([0, 0, 1], F)
    far[5] = near[5]
    near[6], far[6] = 2.0, 1.0
    o, d, near, far = o[:-3].copy(), d[:-3].copy(), near[:-3].copy(), far[:-3].copy()
    if shift is not None:
        o += shift
    return o, d, near, far


def scene(name):
    """-> dict(o, d, near, far, roi, res, step, max_step, gamma)"""
    roi, res, step, max_step, gamma, shift = SCENES[name]
    o, d, near, far = rays(shift)
    return dict(o=o, d=d, near=near, far=far, roi=roi, res=res, step=step, max_step=max_step, gamma=gamma)


def march_args(sc, grid, ctype, max_steps):
    """the positional arguments of oracle.ray_marching / bindings._occ_grid.ray_marching after the rays, as numpy"""
    return (sc["roi"], grid, ctype, sc["step"], sc["max_step"], sc["gamma"], max_steps, True)


def scene_grids(res):
    """the two grids of the filter identity: random (occupancy 0.5) and a thin shell"""
    g = grids(res, GRID_SEED)
    return {"random": g["random"], "shell": g["shell"]}


# ---- the batched route: three grids over three ROIs (one power of two, two not) at a power-of-two resolution, so that the waves of
# entry 0 take the multiply-only instantiation and the others the dividing one -----------------------------------------------------
BATCH_RES = (32, 16, 32)
BATCH_ROI = np.stack([ROI_POW2, ROI_NON_POW2, (ROI_NON_POW2 * F(0.9)).astype(F)]).astype(F)


def batch_grids(kind):
    rng = np.random.default_rng(GRID_SEED + 1)
    if kind == "full":
        return np.ones((3,) + BATCH_RES, bool)
    return rng.random((3,) + BATCH_RES) > 0.5


def batch_cases():
    """-> {name: (rays dict, kwargs of the batched march)}: per-ray entries with -1 among them, and three equal runs of rays"""
    sc = scene("non_pow2")
    n = sc["o"].shape[0]
    bi = np.random.default_rng(9).integers(-1, 3, n).astype(np.int32)
    m = n // 3 * 3
    cut = {k: (v[:m].copy() if k in ("o", "d", "near", "far") else v) for k, v in sc.items()}
    return {"batch_inds": (sc, dict(batch_inds=bi)), "batch_data_size": (cut, dict(batch_data_size=m // 3))}
