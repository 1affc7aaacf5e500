"""Permutohedral encoder, host side: the meta builder against the restated create_meta (tests/permuto_ref.py), its errors,
get_permuto_cfg, and the package importing without a GPU."""
import numpy as np
import pytest

import permuto_ref as R


@pytest.fixture(scope="module")
def backend():
    from nr3d_lib_amd import _hip
    import os
    if not os.path.exists(_hip.LIB_PATH):
        _hip.build()
    import nr3d_lib_amd.bindings._permuto as B
    return B


@pytest.mark.parametrize("D,hs,res,nf", [
    (3, 2 ** 12, [4., 8., 16., 32., 64., 128., 256., 512.], [4, 4, 2, 2, 2, 2, 2, 2]),
    (7, 2 ** 16, [16.0, 32.0, 64.0, 128.0, 256.0, 512.0, 1024.0, 2048.0], [2] * 8),
    (2, 3001, [3.5, 7.25], [4, 8]),
    (64, 1024, [1.0, 2.0, 3.0], [2, 6, 4]),
    (24, 17, list(np.geomspace(10, 1000, 24)), [2] * 24),
])
def test_meta_matches_restated_create_meta(backend, D, hs, res, nf):
    m = backend.PermutoEncMeta(D, hs, res, nf)
    r = R.create_meta(D, hs, res, nf)
    for k in ("n_dims_to_encode", "n_levels", "n_feat_per_pseudo_lvl", "n_pseudo_levels", "n_encoded_dims", "n_params",
              "level_offsets", "level_n_params", "level_sizes", "level_n_feats", "level_scales0", "map_levels", "map_cnt"):
        assert getattr(m, k) == r[k], k
    assert m.level_scales_multidim.shape == (len(res), D)
    assert np.array_equal(m.level_scales_multidim.numpy(), np.array(r["level_scales_multidim"], np.float32))


def test_pseudo_width(backend):
    assert backend.PermutoEncMeta(3, 64, [2, 4], [4, 8]).n_feat_per_pseudo_lvl == 4
    assert backend.PermutoEncMeta(3, 64, [2, 4], [4, 2]).n_feat_per_pseudo_lvl == 2
    assert backend.PermutoEncMeta(3, 64, [2, 4], [2, 2]).n_feat_per_pseudo_lvl == 2


@pytest.mark.parametrize("args,msg", [
    ((21, 64, [2.], [2]), "not supported n_dims_to_encode=21"),
    ((1, 64, [2.], [2]), "not supported n_dims_to_encode=1"),
    ((3, 64, [2., 4.], [2, 3]), "greatest common divisor"),
    ((3, 64, [2., 4.], [1, 1]), "greatest common divisor"),
    ((3, 64, [1.] * 25, [2] * 25), "exceeds maximum level=24"),
    ((3, 2 ** 30, [1., 2.], [2, 2]), "param size too large"),
    ((3, 64, [1., 2.], [2]), "same length"),
])
def test_meta_errors(backend, args, msg):
    with pytest.raises(RuntimeError, match=msg):
        backend.PermutoEncMeta(*args)
    with pytest.raises(RuntimeError):
        R.create_meta(*args)


def test_supported_dims_match_the_library(backend):
    import ctypes as C
    from nr3d_lib_amd import _hip
    buf = (C.c_int32 * 64)()
    n = _hip.lib().nr3d_permuto_supported_n_input_dims(buf)
    assert list(buf[:n]) == backend.supported_n_input_dims == R.SUPPORTED


def test_get_permuto_cfg():
    from nr3d_lib_amd.models.grid_encodings.permuto import get_permuto_cfg
    c = get_permuto_cfg('multi_res')
    assert np.allclose(c['res_list'], np.geomspace(10.0, 1000.0, 16)) and c['n_feats_list'] == [2] * 16
    assert c['hashmap_size'] == 2 ** 19
    c = get_permuto_cfg('multi_res', coarsest_res=16., finest_res=2048., n_levels=8, n_feats=4, log2_hashmap_size=16,
                        apply_random_shifts_per_level=False)
    assert np.allclose(c['res_list'], np.geomspace(16., 2048., 8)) and c['n_feats_list'] == [4] * 8
    assert c['hashmap_size'] == 2 ** 16 and c['apply_random_shifts_per_level'] is False
    with pytest.raises(RuntimeError):
        get_permuto_cfg('bogus')


def test_package_imports_without_gpu(backend):
    from nr3d_lib_amd.models.grid_encodings.permuto import (PermutoEncImpl, PermutoEncoding, generate_meta,  # noqa: F401
                                                             level_param_index_shape)
    m = generate_meta(3, [4., 8.], [2, 4], 256)
    assert level_param_index_shape(m, 1) == ((slice(512, 512 + 1024),), (256, 4))
    enc = PermutoEncoding(3, permuto_cfg=dict(res_list=[4., 8.], n_feats_list=[2, 4], hashmap_size=256), dtype=torch_float())
    assert enc.flattened_params.shape == (m.n_params,) and enc.out_features == 6
    assert enc.get_level_param(1).shape == (256, 4)
    assert float(enc.flattened_params.detach().abs().max()) <= 1e-4
    assert set(enc.stat_param()) >= {"total.mean", "lv.0.mean", "lv.1.absmax"}
    assert enc.get_extra_state()["hashmap_size"] == 256


def torch_float():
    import torch
    return torch.float
