"""GPU: csrc/forest_ray_test.hip (nr3d_forest_ray_test_count / _emit) through ``bindings._forest.forest_ray_test`` and
``ForestBlockSpace.ray_test`` against the dense torch route of the same method (``FUSED_FOREST_RAY_TEST = False``), by ``torch.equal``
on every field after the dense output's equal entries are put in (entry, block) order -- the one thing the dense route leaves to its
sort.  Forests and rays come from tests/forest_ray_test_ref.py (level 0, the plus, level 4 at 15 % and full, a strip one block thick;
random, lattice, inside, behind and missing rays); no case is excused."""
import numpy as np
import pytest
import torch

import forest_ray_test_ref as R

pytestmark = pytest.mark.gpu

FORESTS = R.forests()
FIELDS = ("rays_inds", "seg_pack_infos", "seg_block_inds", "seg_entries", "seg_exits", "near", "far", "rays_o", "rays_d", "tag")
BOUNDS = ("none_none", "number_number", "tensor_tensor", "none_number")


def _space(dev, fo):
    from nr3d_lib_amd.models.spatial import ForestBlockSpace
    space = ForestBlockSpace(device=dev)
    space.populate(mode="from_corners", corners=fo.block_ks.astype(np.int64), level=fo.level, world_origin=fo.world_origin.tolist(),
                   world_block_size=fo.world_block_size.tolist())
    assert np.array_equal(space.block_ks.cpu().numpy(), fo.block_ks)
    return space


def _bounds(fo, kind, n, rng, dev):
    span = float((fo.world_block_size * (1 << fo.level)).max())
    if kind == "none_none":
        return None, None
    if kind == "number_number":
        return 0.05, 0.45 * span
    if kind == "none_number":
        return None, 0.45 * span
    near = torch.from_numpy(rng.uniform(0.0, 0.3, n).astype(np.float32)).to(dev)
    far = torch.from_numpy(rng.uniform(0.2 * span, 1.5 * span, n).astype(np.float32)).to(dev)
    return near, far


def _route(space, fused, o, d, near, far, **kw):
    """ForestBlockSpace.ray_test through one route; the fused one must reach the binding exactly once"""
    from nr3d_lib_amd.models.spatial import forest as F
    calls, keep, binding = [], F.FUSED_FOREST_RAY_TEST, F.forest_ray_test

    def counted(*a, **k):
        calls.append(1)
        return binding(*a, **k)
    try:
        F.FUSED_FOREST_RAY_TEST, F.forest_ray_test = fused, counted
        ret = space.ray_test(o, d, near=near, far=far, **kw)
    finally:
        F.FUSED_FOREST_RAY_TEST, F.forest_ray_test = keep, binding
    assert len(calls) == (1 if fused else 0)
    return ret


def _ties_in_block_order(rt, far_absent=False):
    """the dense route's dict with equal entries of a pack ordered by block index (numpy on the host) -> (dict, tied pairs).
    ``far_absent``: ``far`` is the last segment's exit, so it follows the order too"""
    if rt["num_rays"] == 0:
        return rt, 0
    dev = rt["seg_entries"].device
    e, b, x = (rt[k].cpu().numpy() for k in ("seg_entries", "seg_block_inds", "seg_exits"))
    pack = np.repeat(np.arange(rt["num_rays"]), rt["seg_pack_infos"][:, 1].cpu().numpy())
    assert pack.shape == e.shape
    order = np.lexsort((b, e, pack))
    assert np.array_equal(e[order], e)                              # entries were sorted already: only ties move
    ties = int(((np.diff(e) == 0) & (np.diff(pack) == 0)).sum())
    out = dict(rt)
    out["seg_block_inds"], out["seg_exits"] = torch.from_numpy(b[order]).to(dev), torch.from_numpy(x[order]).to(dev)
    if far_absent:
        out["far"] = out["seg_exits"][rt["seg_pack_infos"].sum(-1) - 1]
    return out, ties


def _assert_same(fused, dense, what):
    assert fused["num_rays"] == dense["num_rays"], what
    if dense["num_rays"] == 0:
        assert fused["rays_inds"] is None and dense["rays_inds"] is None
        for k in ("rays_o", "rays_d"):
            assert tuple(fused[k].shape) == tuple(dense[k].shape) == (0, 3) and fused[k].dtype == dense[k].dtype, (what, k)
        assert set(fused) == set(dense)
        return
    assert set(fused) == set(dense), (what, set(fused) ^ set(dense))
    for k in FIELDS:
        a, b = fused[k], dense[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.is_contiguous(), (what, k, a.dtype, b.dtype, a.shape, b.shape)
        assert torch.equal(a, b), (what, k, int((a != b).sum()), a.numel())


def _compare(space, fo, o, d, near, far, what):
    tag = torch.arange(o.shape[0], device=o.device, dtype=torch.float32) * 0.5
    dense, ties = _ties_in_block_order(_route(space, False, o, d, near, far, tag=tag, label="kept"), far is None)
    fused = _route(space, True, o, d, near, far, tag=tag, label="kept")
    _assert_same(fused, dense, what)
    assert fused.get("label", "kept") == "kept"
    return dense, ties


@pytest.mark.parametrize("bounds", BOUNDS)
@pytest.mark.parametrize("name", list(FORESTS))
def test_space_ray_test_equals_the_dense_route(dev, name, bounds):
    fo, space = FORESTS[name], _space(dev, FORESTS[name])
    rng = np.random.default_rng(11)
    segments = ties = 0
    for kind, n in (("random", 1000), ("lattice", 1000), ("inside", 65), ("behind", 64), ("miss", 63)):
        o, d = (torch.from_numpy(a).to(dev) for a in R.rays(fo, rng, n, kind))
        near, far = _bounds(fo, bounds, n, rng, dev)
        dense, t = _compare(space, fo, o, d, near, far, (name, bounds, kind))
        if kind in ("behind", "miss"):
            assert dense["num_rays"] == 0
        else:
            assert dense["num_rays"] > 0
            segments += dense["seg_entries"].numel(); ties += t
        if kind == "inside" and bounds in ("none_none", "none_number"):
            assert dense["num_rays"] == n and bool((dense["near"] == 0).all())       # the origin's own block starts at 0
    assert segments > 0
    if name == "l4_sparse" and bounds == "none_none":
        assert ties > 0                                              # anisotropic blocks: rounding ties two entries (see the CPU test)


@pytest.mark.parametrize("bounds", BOUNDS)
def test_level_15_forest_walked_from_global_memory(dev, bounds):
    """blocks scattered over a level-15 cube (the deepest an int16 block_ks allows): more non-leaf nodes than the kernel keeps in LDS
    (kLdsNodes = 8192 of csrc/forest_ray_test.hip), so this is the variant that reads bytes and exsum from global memory"""
    rng = np.random.default_rng(15)
    blocks = [tuple(k) for k in rng.integers(0, 1 << 15, (900, 3)).tolist()] + [(32767, 32767, 32767), (0, 0, 0)]
    fo = R.Forest(blocks, 15, (-1000.0, 20.0, 3.5), (0.5, 0.25, 0.5))
    assert fo.level_poffset > 8192
    space = _space(dev, fo)
    for kind, n in (("lattice", 1000), ("inside", 65), ("miss", 63)):
        o, d = (torch.from_numpy(a).to(dev) for a in R.rays(fo, rng, n, kind))
        near, far = _bounds(fo, bounds, n, rng, dev)
        dense, _ = _compare(space, fo, o, d, near, far, ("l15", bounds, kind))
        assert (dense["num_rays"] > 0) == (kind != "miss")


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65])
def test_ray_counts_around_a_wave(dev, n):
    """a wave holds 8 rays of 8 lanes, a workgroup 16 rays"""
    fo = FORESTS["l4_sparse"]
    space = _space(dev, fo)
    rng = np.random.default_rng(n)
    o, d = (torch.from_numpy(a).to(dev) for a in R.rays(fo, rng, n, "inside"))
    for bounds in BOUNDS:
        near, far = _bounds(fo, bounds, n, rng, dev)
        dense, _ = _compare(space, fo, o, d, near, far, (n, bounds))
        if near is None:                                            # from 0 on, the origin's own block is always a hit
            assert dense["num_rays"] == n


def test_far_cuts_the_last_segments_away(dev):
    fo = FORESTS["l4_full"]
    space = _space(dev, fo)
    o = torch.tensor([[-9.0, 0.5, 0.5], [-9.0, -3.5, 2.5]], device=dev)
    d = torch.tensor([[1.0, 0, 0], [1.0, 0, 0]], device=dev)
    full, _ = _compare(space, fo, o, d, None, None, "full")
    cut, _ = _compare(space, fo, o, d, None, torch.tensor([5.5, 17.0], device=dev), "cut")
    assert full["seg_pack_infos"][:, 1].tolist() == [16, 16] and cut["seg_pack_infos"][:, 1].tolist() == [5, 16]
    assert cut["seg_exits"][4].item() == 5.5 and cut["far"].tolist() == [5.5, 17.0] and full["far"].tolist() == [17.0, 17.0]
    assert cut["near"].tolist() == [1.0, 1.0]


def test_zero_direction_components_inside_on_the_plane_and_outside(dev):
    """parallel to a slab: strictly inside (hits), exactly on one of its planes (0 / 0: the dense route rejects the pair), outside"""
    fo = FORESTS["l4_full"]                                          # [-8, 8]^3, unit blocks
    space = _space(dev, fo)
    ys = [-7.5, -7.0, -8.0, 8.0, 8.5, -8.5, 0.0, 0.5]
    rays = [([-9.0, y, 0.5], [1.0, 0, 0]) for y in ys]               # one zero ... (z strictly inside its slab)
    rays += [([-9.0, y, 0.5], [0.6, 0, 0.8]) for y in ys]            # ... one zero, oblique in the others
    rays += [([0.5, y, -9.0], [0, 0, 1.0]) for y in ys] + [([0.0, y, 9.0], [0, 0, -1.0]) for y in ys]        # two zeros
    rays += [([0.5, 0.5, 0.5], [0, -1.0, 0]), ([0.5, 0.5, 0.5], [0, 0, 1.0])]                                 # from inside a block
    o = torch.tensor([r[0] for r in rays], device=dev)
    d = torch.tensor([r[1] for r in rays], device=dev)
    for near, far in ((None, None), (0.05, 12.0)):
        dense, _ = _compare(space, fo, o, d, near, far, ("zeros", near))
        hit = set(dense["rays_inds"].tolist())
        assert {0, 7, 8, 15, 16, 23, 32, 33} <= hit                  # strictly inside
        assert not ({1, 2, 3, 4, 5, 6} & hit) and not ({24 + i for i in range(8)} & hit)      # on a plane, outside; x = 0 is a plane


def test_binding_equals_the_dense_route_and_checks_its_arguments(dev):
    from nr3d_lib_amd import _hip as H
    from nr3d_lib_amd.bindings._forest import forest_ray_test
    fo = FORESTS["plus"]
    space = _space(dev, fo)
    rng = np.random.default_rng(5)
    o, d = (torch.from_numpy(a).to(dev) for a in R.rays(fo, rng, 1000, "lattice"))
    for bounds in BOUNDS:
        near, far = _bounds(fo, bounds, 1000, rng, dev)
        dense, _ = _ties_in_block_order(_route(space, False, o, d, near, far), far is None)
        got = forest_ray_test(space.meta, o, d, near, far)
        assert set(got) == {"rays_inds", "seg_pack_infos", "seg_block_inds", "seg_entries", "seg_exits", "near", "far"}
        for k, v in got.items():
            assert v.dtype == dense[k].dtype and torch.equal(v, dense[k]), (bounds, k)
        assert H.tiles(got["seg_pack_infos"], got["seg_entries"].numel())
        # ... and equals the numpy restatement of the descent
        cut = lambda v: v[:200].contiguous() if isinstance(v, torch.Tensor) else v                  # noqa: E731
        host = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else v                      # noqa: E731
        want = R.ray_test(R.descent, fo, host(cut(o)), host(cut(d)), host(cut(near)), host(cut(far)))
        head = forest_ray_test(space.meta, cut(o), cut(d), cut(near), cut(far))
        for k, v in want.items():
            assert np.array_equal(head[k].cpu().numpy(), v), (bounds, k)
    assert forest_ray_test(space.meta, o[:0], d[:0]) is None
    for bad in (lambda: forest_ray_test(space.meta, o.double(), d.double()), lambda: forest_ray_test(space.meta, o, d[:10]),
                lambda: forest_ray_test(space.meta, o, d, near=torch.zeros(3, device=dev)), lambda: forest_ray_test(space.meta, o.cpu(), d.cpu()),
                lambda: forest_ray_test(space.meta, o.t().contiguous().t(), d)):
        with pytest.raises(RuntimeError):
            bad()


def test_other_inputs_keep_the_dense_route(dev):
    fo = FORESTS["plus"]
    space = _space(dev, fo)
    o, d = (torch.from_numpy(a).to(dev) for a in R.rays(fo, np.random.default_rng(2), 64, "random"))
    from nr3d_lib_amd.models.spatial import forest as F
    keep = F.FUSED_FOREST_RAY_TEST
    try:
        F.FUSED_FOREST_RAY_TEST = True
        assert F._takes_fused_ray_test(space, o, d, None, 4.0) and F._takes_fused_ray_test(space, o, d, d[:, 0], d[:, 1])
        assert not F._takes_fused_ray_test(space, o.double(), d.double(), 0.05, 4.0)          # other dtypes: the torch chain
        assert not F._takes_fused_ray_test(space, o.half(), d.half(), None, None)
        assert not F._takes_fused_ray_test(space, o.cpu(), d.cpu(), None, None)
        assert not F._takes_fused_ray_test(space, o, d, d[:, :1], None)                       # a bound that is not [R]
        assert not F._takes_fused_ray_test(space, o, d, None, d[:, 0].double())
        F.FUSED_FOREST_RAY_TEST = False
        assert not F._takes_fused_ray_test(space, o, d, None, None)
    finally:
        F.FUSED_FOREST_RAY_TEST = keep
    c = _route(space, True, o[:, [0, 1, 2]].t().contiguous().t(), d, None, None, return_rays=False)      # a strided view is made contiguous
    assert "rays_o" not in c and c["num_rays"] > 0


def test_two_calls_give_the_same_bytes(dev):
    fo = FORESTS["l4_full"]
    space = _space(dev, fo)
    o, d = (torch.from_numpy(a).to(dev) for a in R.rays(fo, np.random.default_rng(9), 1000, "lattice"))
    a, b = _route(space, True, o, d, None, 9.0), _route(space, True, o, d, None, 9.0)
    for k in FIELDS[:-1]:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k


def test_fused_segments_give_the_marcher_the_same_samples(dev):
    from nr3d_lib_amd.bindings import _occ_grid
    fo = FORESTS["l4_sparse"]
    space = _space(dev, fo)
    rng = np.random.default_rng(4)
    grid = torch.from_numpy(rng.random((fo.n_trees, 4, 4, 4)) > 0.5).to(dev)
    o, d = (torch.from_numpy(a).to(dev) for a in R.rays(fo, rng, 1000, "random"))
    out = []
    for fused in (True, False):
        rt = _route(space, fused, o, d, 0.05, 9.0)
        if not fused:
            rt, _ = _ties_in_block_order(rt)
        out.append(_occ_grid.forest_ray_marching(space.meta, rt["rays_o"], rt["rays_d"], rt["near"], rt["far"], rt["seg_block_inds"].int(),
                                                 rt["seg_entries"], rt["seg_exits"], rt["seg_pack_infos"].int(), grid, 0.04, 1e10, 0.0, 64, True))
    assert out[0][1].shape[0] > 0
    for a, b, name in zip(out[0], out[1], ("packed_info", "t_starts", "t_ends", "ridx", "blidx", "gidx")):
        assert torch.equal(a, b), name
