"""numpy restatement of the time-sliced march (nr3d_dynamic_ray_marching_*): the float32 frame lookup of
``torch_consecutive_nearest1d`` (nr3d_lib/utils.py:675-699), the static | dynamic union, then the batched-march reference of
tests/test_occ_grid_gpu.py (``oracle.ray_marching`` on the [n_slices, Rx, Ry, Rz] union with the slice as batch index) and the
per-sample gathers.  Also the inputs of tests/golden/keyframe_nearest.npz (``golden_cases``): the generator script and the tests
share them."""
import numpy as np

TABLE_KEYS = np.array([0, .25, .25, .5, 1], np.float32)
TABLE_T = np.array([-1, 0, .125, .25, .3, .375, .75, 1, 2, np.nan, np.inf, -np.inf], np.float32)
TABLE_WANT = [0, 0, 1, 1, 2, 3, 4, 4, 4, 4, 4, 1]
TABLE2_KEYS = np.array([0, 1], np.float32)
TABLE2_T = np.array([-1, .3, .5, 2, np.nan], np.float32)
TABLE2_WANT = [0, 0, 1, 1, 1]


def golden_cases():
    """[(name, keys f32 [T], t f32 [n])]: the two tables, then seeded random keys with T in {1, 2, 5, 37}, with duplicated keys,
    and t below, above, on and midway between keys (plus random values and the non-finite ones)"""
    cases = [("table5", TABLE_KEYS, TABLE_T), ("table2", TABLE2_KEYS, TABLE2_T)]
    rng = np.random.default_rng(20)
    for T in (1, 2, 5, 37):
        for dup in (False, True):
            keys = np.sort(rng.uniform(-1, 1, T)).astype(np.float32)
            if dup and T >= 2:
                keys[T // 2] = keys[T // 2 - 1]
                if T >= 5:
                    keys[-1] = keys[-2]
            mid = ((keys[:-1].astype(np.float64) + keys[1:]) / 2).astype(np.float32)       # float32 midpoints: ties or one ulp off
            t = np.concatenate([keys, mid, np.nextafter(mid, np.float32(2)), np.nextafter(mid, np.float32(-2)),
                                [keys[0] - 1, keys[0] - np.float32(1e-6), keys[-1] + 1, keys[-1] + np.float32(1e-6)],
                                rng.uniform(-1.5, 1.5, 40), [np.nan, np.inf, -np.inf]]).astype(np.float32)
            cases.append((f"T{T}{'dup' if dup else ''}", keys, t))
    return cases


def nearest_keyframe(keys, t):
    """frame index int64 per t: float32 operations in the reference's order"""
    keys, t = np.asarray(keys, np.float32), np.asarray(t, np.float32)
    T = keys.shape[0]
    out = np.zeros(t.shape, np.int64)
    if T == 1:
        return out
    for n, v in enumerate(t.ravel()):
        i = T                                                  # first index with key[i] >= t; NaN compares false: T
        for k in range(T):
            if keys[k] >= v:
                i = k
                break
        i = min(max(i, 1), T - 1)
        with np.errstate(invalid="ignore"):
            prev, nxt = np.abs(np.float32(keys[i - 1] - v)), np.abs(np.float32(keys[i] - v))
        out.ravel()[n] = i - 1 if prev < nxt else i
    return out


def rays_slice(keys, rays_ts, batch_inds=None, n_batches=0):
    """int32 per ray: batch * T + frame, -1 for a batch index outside [0, n_batches)"""
    frame = nearest_keyframe(keys, rays_ts)
    if batch_inds is None:
        return frame.astype(np.int32)
    b = np.asarray(batch_inds, np.int64)
    return np.where((b < 0) | (b >= n_batches), -1, b * len(keys) + frame).astype(np.int32)


def march(oracle, o, d, near, far, rays_ts, keys, grid_dynamic, grid_static, step, max_step, gamma, max_steps, batch_inds=None,
          n_batches=0):
    """-> dict of numpy arrays named as bindings._occ_grid.dynamic_ray_marching's"""
    T = len(keys)
    sl = rays_slice(keys, rays_ts, batch_inds, n_batches)
    union = np.asarray(grid_dynamic, bool)
    if grid_static is not None:
        union = union | np.asarray(grid_static, bool)[None]
    roi = np.tile(np.array([-1, -1, -1, 1, 1, 1], np.float32), (union.shape[0], 1))
    packed_info, t_starts, t_ends, ridx, bidx, gidx = oracle.ray_marching(o, d, near, far, roi, union, 0, step, max_step, gamma,
                                                                          max_steps, True, batch_inds=sl)
    hit = np.nonzero(packed_info[:, 1])[0].astype(np.int64)
    flat = bidx.astype(np.int64)
    out = dict(packed_info=packed_info, rays_slice=sl, ridx_hit=hit, pack_infos=packed_info[hit].astype(np.int64),
               t_starts=t_starts[:, 0], t_ends=t_ends[:, 0], ridx=ridx.astype(np.int64), gidx=gidx,
               ts=np.asarray(keys, np.float32)[flat % T], bidx=None if batch_inds is None else flat // T)
    return out
