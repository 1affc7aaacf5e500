"""CPU: the forest ray test's contract (include/nr3d_hip.h: nr3d_forest_ray_test_*) in its numpy restatement
tests/forest_ray_test_ref.py: the octree descent returns the dense slab test's segments EXACTLY -- blocks, entries, exits and order by
``array_equal`` -- on seeded forests of levels 0 to 4 at about 15 %, 50 % and full occupancy, anisotropic blocks, origins off zero,
random and lattice rays, with and without near / far; both agree with what the reference's own ``ray_box_intersection`` recorded
(tests/golden/ref_forest_ray_test.npz); the header, the generated table and the routing switch are in place."""
import os
import re

import numpy as np
import pytest
import torch

import forest_ray_test_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_forest_ray_test.npz")


def _same(got, want, what):
    for a, b, name in zip(got[:3], want[:3], ("blocks", "entries", "exits")):
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, name, a, b)


@pytest.mark.parametrize("level", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("occupancy", [0.15, 0.5, 1.0])
def test_descent_equals_dense_exactly(level, occupancy):
    rng = np.random.default_rng(1000 * level + int(100 * occupancy))
    wb = (np.array([1.0, 0.5, 1.0], np.float32) * np.float32(rng.choice([1.0, 0.7, 12.5]))).astype(np.float32)
    wo = rng.uniform(-3, 3, 3).astype(np.float32) if level % 2 else np.array([-2, -2, -2], np.float32)
    fo = R.Forest(R.random_blocks(rng, level, occupancy), level, wo, wb)
    n = 1 << level
    segments = ties = most = 0
    for kind, count in (("random", 60), ("lattice", 90), ("inside", 30), ("behind", 5), ("miss", 5)):
        o, d = R.rays(fo, rng, count, kind)
        for i in range(count):
            near, far = (np.float32(0), np.float32(np.inf)) if i % 3 == 0 else \
                (np.float32(0.05), np.float32(rng.uniform(0.5, 3 * n) * wb.max()))
            want = R.dense(fo, o[i], d[i], near, far)
            got = R.descent(fo, o[i], d[i], near, far)
            _same(got, want, (kind, i, o[i], d[i], near, far))
            segments += len(want[0]); ties += int((np.diff(want[1]) == 0).sum()); most = max(most, got[3])
            if kind in ("behind", "miss"):
                assert len(want[0]) == 0
    assert segments > 0
    total_nodes = fo.level_poffset + fo.n_trees
    assert most <= total_nodes                                     # the walk tests a node at most once
    if level == 4 and occupancy == 1.0:
        assert most < total_nodes // 4                             # whole subtrees are pruned


def test_zero_over_zero_pairs_are_rejected_and_nodes_keep_their_leaves():
    """a ray parallel to a slab: strictly inside it, on one of its planes (0 / 0: rejected by the dense route) and outside"""
    fo = R.Forest([(x, y, 0) for x in range(4) for y in range(4)], 2, (0, 0, 0), (1, 1, 1))
    d = np.array([1, 0, 0], np.float32)
    z, inf = np.float32(0), np.float32(np.inf)
    for y, blocks in ((0.5, [0, 2, 8, 10]), (1.0, []), (1.5, [1, 3, 9, 11]), (-0.5, []), (0.0, []), (4.0, [])):
        o = np.array([-1.0, y, 0.5], np.float32)
        want = R.dense(fo, o, d, z, inf)
        _same(R.descent(fo, o, d, z, inf), want, y)
        assert want[0].tolist() == blocks, (y, want[0])
    o = np.array([0.5, 0.5, 0.5], np.float32)                       # two zero components, from inside a block
    want = R.dense(fo, o, np.array([0, 0, -1], np.float32), z, inf)
    _same(R.descent(fo, o, np.array([0, 0, -1], np.float32), z, inf), want, "two zeros")
    assert want[0].tolist() == [0] and want[1][0] == 0 and want[2][0] == 0.5
    for bad in (np.nan, np.inf):                                   # non-finite rays hit nothing on either route
        o = np.array([bad, 0.5, 0.5], np.float32)
        assert len(R.dense(fo, o, d, z, inf)[0]) == 0 == len(R.descent(fo, o, d, z, inf)[0])
        dd = np.array([1, bad, 0], np.float32)
        _same(R.descent(fo, np.array([-1, 0.5, 0.5], np.float32), dd, z, inf), R.dense(fo, np.array([-1, 0.5, 0.5], np.float32), dd, z, inf), bad)


def test_far_cuts_the_last_segments_away_and_equal_entries_come_in_block_order():
    fo = R.forests()["l4_full"]
    o, d = np.array([-9.0, 0.5, 0.5], np.float32), np.array([1, 0, 0], np.float32)
    full = R.descent(fo, o, d, np.float32(0), np.float32(np.inf))
    cut = R.descent(fo, o, d, np.float32(0), np.float32(5.5))
    assert len(full[0]) == 16 and len(cut[0]) == 5 and cut[2][-1] == 5.5 and np.array_equal(cut[0], full[0][:5])
    _same(cut, R.dense(fo, o, d, np.float32(0), np.float32(5.5)), "cut")
    # rays through lattice edges and corners of anisotropic blocks: rounding makes two blocks share an entry depth
    fo = R.forests()["l4_sparse"]
    o, d = R.rays(fo, np.random.default_rng(0), 300, "lattice")
    tied_rays = 0
    for i in range(300):
        want = R.dense(fo, o[i], d[i], np.float32(0), np.float32(np.inf))
        got = R.descent(fo, o[i], d[i], np.float32(0), np.float32(np.inf))
        _same(got, want, ("tie", i))
        tied = np.nonzero(np.diff(got[1]) == 0)[0]
        tied_rays += len(tied) > 0
        assert (np.diff(got[0])[tied] > 0).all()
    assert tied_rays >= 1


def test_reference_forests_match_the_product_octree_builder():
    from nr3d_lib_amd.models.spatial.forest import octree_from_corners
    for name, fo in R.forests().items():
        octree, exsum, points, pyramid = octree_from_corners(torch.from_numpy(fo.block_ks.astype(np.int64)), fo.level)
        assert np.array_equal(octree.numpy(), fo.octree) and np.array_equal(exsum.numpy(), fo.exsum), name
        assert int(pyramid[1, fo.level]) == fo.level_poffset and np.array_equal(points[fo.level_poffset:].numpy(), fo.block_ks), name


def test_against_the_reference_slab_test_recorded_in_the_golden_file():
    z = np.load(GOLDEN)
    assert len(z["cases"]) == 6
    hits = 0
    for c in z["cases"]:
        g = lambda k: z[f"{c}_{k}"]                                                              # noqa: E731
        fo = R.Forest(g("block_ks").tolist(), int(g("level")), g("world_origin"), g("world_block_size"))
        assert np.array_equal(fo.block_ks, g("block_ks"))
        o, d, t_near, t_far, mask = g("rays_o"), g("rays_d"), g("t_near"), g("t_far"), g("mask")
        near, far = np.broadcast_to(g("near"), (o.shape[0],)), np.broadcast_to(g("far"), (o.shape[0],))
        for i in range(o.shape[0]):
            hit = np.nonzero(mask[i])[0]
            hit = hit[np.argsort(t_near[i, hit], kind="stable")]
            want = (hit.astype(np.int64), t_near[i, hit], t_far[i, hit])
            _same(R.dense(fo, o[i], d[i], near[i], far[i]), want, (c, i, "dense"))
            _same(R.descent(fo, o[i], d[i], near[i], far[i]), want, (c, i, "descent"))
            hits += len(hit)
    assert hits > 100


def test_packed_result_of_the_restatement():
    fo = R.forests()["plus"]
    o, d = R.rays(fo, np.random.default_rng(3), 40, "lattice")
    a, b = R.ray_test(R.dense, fo, o, d, 0.05, 3.0), R.ray_test(R.descent, fo, o, d, 0.05, 3.0)
    assert a["seg_pack_infos"][:, 1].sum() == a["seg_block_inds"].shape[0] > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_abi_and_switch():
    from nr3d_lib_amd import _abi
    from nr3d_lib_amd.models.spatial import forest as F
    header = open(os.path.join(ROOT, "include", "nr3d_hip.h")).read()
    assert int(re.search(r"#define\s+NR3D_ABI_VERSION\s+(\d+)", header).group(1)) == 30 == _abi.ABI_VERSION      # additions keep the number
    head = ["ptr", "uint32_t", "ptr", "ptr", "ptr", "float", "ptr", "float"]
    assert _abi.SIGNATURES["nr3d_forest_ray_test_count"] == ("int", head + ["ptr", "ptr"])
    assert _abi.SIGNATURES["nr3d_forest_ray_test_emit"] == ("int", head + ["ptr", "ptr", "uint64_t", "ptr", "ptr", "ptr", "ptr"])
    assert "forest_ray_test.hip" in open(os.path.join(ROOT, "nr3d_lib_amd", "csrc", "Makefile")).read()
    import json
    measured = json.load(open(os.path.join(ROOT, "profiles", "forest_ray_test.json")))
    assert F.FUSED_FOREST_RAY_TEST is measured["default_on"] is all(r["fused_wins"] for r in measured["rows"].values())
    assert measured["rounds_plus7"] >= 7 and min(r["shortest_round_ms"] for r in measured["rows"].values()) >= measured["window_ms"]
    space = F.ForestBlockSpace()
    space.populate(mode="from_corners", corners=torch.tensor(R.PLUS[1]), level=2)
    o = torch.zeros(4, 3)
    assert not F._takes_fused_ray_test(space, o, o, None, None)                 # CPU tensors keep the torch route
    assert not F._takes_fused_ray_test(space, o.double(), o.double(), 0.1, 2.0)


def test_binding_refuses_cpu_tensors():
    from nr3d_lib_amd.bindings._forest import ForestMeta, forest_ray_test
    with pytest.raises(RuntimeError):
        forest_ray_test(ForestMeta(), torch.zeros(2, 3), torch.ones(2, 3))
