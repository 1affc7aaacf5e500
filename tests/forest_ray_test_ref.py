"""tests/forest_ray_test_ref.py -- the forest ray test's contract (include/nr3d_hip.h: nr3d_forest_ray_test_count / _emit) restated in
numpy, written from the contract's text: ``dense`` is the slab test on every block (what ForestBlockSpace.ray_test computes in torch),
``descent`` the per-ray walk of the byte octree that csrc/forest_ray_test.hip runs -- same node test, same child order, same leaf
arithmetic -- so that the claim "the descent loses no hit and changes no float" is checked on the CPU, where every intermediate can be
looked at.  Also the forests and the rays the CPU and GPU tests share."""
import numpy as np

f32 = np.float32


def morton(k, level):
    c = 0
    for b in range(level):
        c |= ((k[0] >> b & 1) << (3 * b + 2)) | ((k[1] >> b & 1) << (3 * b + 1)) | ((k[2] >> b & 1) << (3 * b))
    return c


class Forest:
    """the SPC layout of include/nr3d_hip.h built from block coordinates: nodes level by level, children in child-index order
    (x<<2 | y<<1 | z), one byte per non-leaf node, exsum the exclusive prefix sum of the popcounts"""

    def __init__(self, blocks, level, world_origin=(0, 0, 0), world_block_size=(1, 1, 1)):
        self.level = level
        ks = sorted({tuple(int(v) for v in k) for k in blocks}, key=lambda k: morton(k, level))
        assert ks and all(0 <= v < (1 << level) for k in ks for v in k)
        per_level = [None] * (level + 1)
        per_level[level] = ks
        for l in range(level - 1, -1, -1):
            per_level[l] = sorted({tuple(v >> 1 for v in k) for k in per_level[l + 1]}, key=lambda k: morton(k, l))
        octree = []
        for l in range(level):
            have = set(per_level[l + 1])
            for k in per_level[l]:
                byte = 0
                for c in range(8):
                    if (2 * k[0] + (c >> 2 & 1), 2 * k[1] + (c >> 1 & 1), 2 * k[2] + (c & 1)) in have:
                        byte |= 1 << c
                octree.append(byte)
        self.octree = np.array(octree, np.uint8)
        pop = np.array([bin(b).count("1") for b in octree], np.int64)
        self.exsum = np.concatenate([[0], np.cumsum(pop)]).astype(np.int32)
        self.level_poffset = sum(len(p) for p in per_level[:level])
        self.block_ks = np.array(ks, np.int16).reshape(-1, 3)
        self.n_trees = len(ks)
        self.world_origin = np.array(world_origin, f32)
        self.world_block_size = np.array(world_block_size, f32)


def dense(fo, o, d, near, far):
    """one ray against every block -> (block indices, entries, exits) by (entry, block) ascending.  near / far float32 scalars
    (no bound: 0 / +inf)"""
    wb, wo = fo.world_block_size, fo.world_origin
    bmin = fo.block_ks.astype(f32) * wb + wo
    with np.errstate(all="ignore"):
        t0, t1 = (bmin - o) / d, ((bmin + wb) - o) / d
        tn = np.maximum(np.minimum(t0, t1).max(1), near)          # np.maximum / minimum / max / min propagate NaN like torch's
        tf = np.minimum(np.maximum(t0, t1).min(1), far)
    hit = np.nonzero((tf > tn) & (tf > 0))[0]
    hit = hit[np.argsort(tn[hit], kind="stable")]
    return hit.astype(np.int64), tn[hit].astype(f32), tf[hit].astype(f32)


def _nan_min(a, b):
    return a if a != a else (b if b != b else (a if a < b else b))


def _nan_max(a, b):
    return a if a != a else (b if b != b else (a if a > b else b))


def _leaf(fo, k, o, d, near, far):
    wb, wo = fo.world_block_size, fo.world_origin
    tn = tf = None
    with np.errstate(all="ignore"):
        for a in range(3):
            bmin = f32(k[a]) * wb[a] + wo[a]
            bmax = bmin + wb[a]
            t0, t1 = (bmin - o[a]) / d[a], (bmax - o[a]) / d[a]
            lo, hi = _nan_min(t0, t1), _nan_max(t0, t1)
            tn = lo if a == 0 else _nan_max(tn, lo)
            tf = hi if a == 0 else _nan_min(tf, hi)
    e, x = _nan_max(tn, near), _nan_min(tf, far)
    return bool(x > e and x > 0), e, x


def _node(fo, k, shift, o, d, near, far):
    wb, wo = fo.world_block_size, fo.world_origin
    e, x = near, far
    with np.errstate(all="ignore"):
        for a in range(3):
            k0, k1 = k[a] << shift, ((k[a] + 1) << shift) - 1
            lo = f32(k0) * wb[a] + wo[a]
            hi = (f32(k1) * wb[a] + wo[a]) + wb[a]
            if d[a] == 0:
                if not (lo <= o[a] <= hi):
                    return False
            else:
                t0, t1 = (lo - o[a]) / d[a], (hi - o[a]) / d[a]
                e, x = _nan_max(e, _nan_min(t0, t1)), _nan_min(x, _nan_max(t0, t1))
    return bool(x >= e and x >= 0)


def descent(fo, o, d, near, far):
    """one ray down the byte octree, children front to back -> (block indices, entries, exits) by (entry, block), nodes tested"""
    L, out, tested = fo.level, [], 1
    if L == 0:
        ok, e, x = _leaf(fo, (0, 0, 0), o, d, near, far)
        if ok:
            out.append((e, 0, x))
    elif _node(fo, (0, 0, 0), L, o, d, near, far):
        sm = (4 if d[0] < 0 else 0) | (2 if d[1] < 0 else 0) | (1 if d[2] < 0 else 0)
        stack = [(0, 0, (0, 0, 0))]                 # (depth, node, coordinates); children pushed back to front
        while stack:
            depth, node, k = stack.pop()
            bits = int(fo.octree[node])
            push = []
            for i in range(8):
                c = i ^ sm
                if not bits >> c & 1:
                    continue
                child = int(fo.exsum[node]) + bin(bits & ((2 << c) - 1)).count("1")
                ck = (2 * k[0] + (c >> 2 & 1), 2 * k[1] + (c >> 1 & 1), 2 * k[2] + (c & 1))
                tested += 1
                if depth + 1 == L:
                    ok, e, x = _leaf(fo, ck, o, d, near, far)
                    if ok:
                        out.append((e, child - fo.level_poffset, x))
                elif _node(fo, ck, L - depth - 1, o, d, near, far):
                    push.append((depth + 1, child, ck))
            # a depth-first walk that visits a node's subtree before its next sibling emits in another order than this level-wise
            # one; the order is fixed by the sort below either way
            stack.extend(reversed(push))
    out.sort(key=lambda r: (r[0], r[1]))
    return (np.array([r[1] for r in out], np.int64), np.array([r[0] for r in out], f32), np.array([r[2] for r in out], f32), tested)


def ray_test(fn, fo, o, d, near=None, far=None):
    """every ray through ``fn`` (dense or descent) -> dict of the packed result as ForestBlockSpace.ray_test returns it (numpy)"""
    R = o.shape[0]
    nr = np.broadcast_to(f32(0) if near is None else np.asarray(near, f32), (R,))
    fr = np.broadcast_to(f32(np.inf) if far is None else np.asarray(far, f32), (R,))
    sb, se, sx, inds, infos = [], [], [], [], []
    for i in range(R):
        b, e, x = fn(fo, o[i], d[i], nr[i], fr[i])[:3]
        if len(b):
            inds.append(i)
            infos.append((len(sb), len(b)))
            sb += b.tolist(); se += e.tolist(); sx += x.tolist()
    return dict(rays_inds=np.array(inds, np.int64), seg_pack_infos=np.array(infos, np.int64).reshape(-1, 2),
                seg_block_inds=np.array(sb, np.int64), seg_entries=np.array(se, f32), seg_exits=np.array(sx, f32))


# ---- forests and rays shared by the CPU and the GPU tests ----------------------------------------------------------------------------
PLUS = (2, [(1, 1, 1), (2, 1, 1), (1, 2, 1), (0, 1, 1), (1, 1, 2), (2, 2, 1)])          # tests/test_forest_cpu.py FORESTS["plus"]


def random_blocks(rng, level, occupancy):
    n = 1 << level
    occ = rng.random((n, n, n)) < occupancy
    if not occ.any():
        occ[0, 0, 0] = True
    return [tuple(k) for k in np.argwhere(occ).tolist()]


def forests():
    """name -> Forest: level 0, the plus, level 4 at 15 % and full, a strip one block thick; anisotropic blocks, origins off zero"""
    rng = np.random.default_rng(7)
    return {
        "single": Forest([(0, 0, 0)], 0, (-0.5, 0.25, 1.0), (1.0, 2.0, 0.5)),
        "plus": Forest(PLUS[1], PLUS[0], (-2.0, -2.0, -2.0), (1.0, 1.0, 1.0)),
        "l4_sparse": Forest(random_blocks(rng, 4, 0.15), 4, (-3.1, 0.7, -8.3), (0.7, 0.35, 0.7)),
        "l4_full": Forest(random_blocks(rng, 4, 1.0), 4, (-8.0, -8.0, -8.0), (1.0, 1.0, 1.0)),
        "strip": Forest([(x, 3, 1) for x in range(32) if x not in (5, 6, 20)], 5, (-10.0, 0.0, 0.0), (12.5, 12.5, 6.25)),
    }


def rays(fo, rng, R, kind):
    """float32 (o, d) [R, 3].  random: origins in and around the forest's cube, normal directions (normalised).  lattice: origins on
    the half-block lattice (faces, edges, corners and block centres), directions with components in {-1, 0, 1} (normalised): through
    faces, edges and corners, with one and two zero components, inside a slab, on its plane and outside.  inside: origins strictly
    inside occupied blocks.  behind: the forest wholly behind the origin.  miss: every ray passes beside the cube."""
    n, wb, wo = 1 << fo.level, fo.world_block_size, fo.world_origin
    d = rng.normal(size=(R, 3)).astype(f32)
    if kind == "random":
        o = (rng.uniform(-0.5, n + 0.5, (R, 3)).astype(f32) * wb + wo).astype(f32)
    elif kind == "lattice":
        half = rng.integers(-1, 2 * n + 2, (R, 3))
        near_block = 2 * fo.block_ks[rng.integers(0, fo.n_trees, R)].astype(np.int64) + rng.integers(-3, 6, (R, 3))
        half[::2] = near_block[::2]                                # every other origin within a block and a half of an occupied block
        o = ((half.astype(f32) * f32(0.5)) * wb + wo).astype(f32)
        d = rng.integers(-1, 2, (R, 3)).astype(f32)
        d[(d == 0).all(1)] = (1, 0, 0)
    elif kind == "inside":
        k = fo.block_ks[rng.integers(0, fo.n_trees, R)].astype(f32)
        o = ((k + rng.uniform(0.05, 0.95, (R, 3)).astype(f32)) * wb + wo).astype(f32)
    elif kind == "behind":
        o = ((f32(n) + rng.uniform(0.5, 2.0, (R, 3)).astype(f32)) * wb + wo).astype(f32)
        d = np.abs(d) + f32(0.01)
    elif kind == "miss":
        o = (np.array([-1.0, n + 0.5, n + 0.5], f32) * wb + wo + np.zeros((R, 1), f32)).astype(f32)
        d = np.abs(d) * np.array([1, 0.2, 0.2], f32) + f32(0.01)
    else:
        raise ValueError(kind)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)
