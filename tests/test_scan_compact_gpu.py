"""GPU: the device-wide exclusive scan (csrc/scan.h) and the pack compaction (csrc/compact.h) against tests/scan_ref.py -- every size class,
every class boundary, every compiled instantiation.  Integers only: every comparison is ``torch.equal``, there is no tolerance in this file.

Both headers pick their kernel by the number of counts n: n == 0 a memset; n <= kSmallMax one workgroup of kSmallThreads threads, compiled
for PER = 1, 2, 4, 8, 16, 32 counts per thread; above it three launches over tiles of kTile counts, whose middle launch walks the tile sums
kThreads at a time (a second round from kThreads * kTile + 1 counts on).

Which case runs which kernel (n; "a" .. "g" are the test groups below, SIZES the shared list):

  kernel                               scan<i64,i64>            compact<i64,1>           scan<i32,i32>                     compact<i32,1>
  k_pack_infos_small / k_c_small
    PER 1   (n <= 1024)                a: 1 .. 1024             b: 1 .. 1024             d: 1024                           e: 1024 (info32)
    PER 2   (.. 2048)                  a: 1025, 2048; g: 1025   b: 1025, 2048            d: 1025                           e: 1025 (info32)
    PER 4   (.. 4096)                  a: 2049, 4096; g: 2112   b: 2049, 4096            f: 2049 (sample_on_segments)      e: 4096 (info32); f: 2049 (none)
    PER 8   (.. 8192)                  a: 4097, 8192            b: 4097, 8192            d: 4097                           e: 8192 (info32)
    PER 16  (.. 16384)                 a: 8193, 16384           b: 8193, 16384           d: 8193                           e: 16384 (info32)
    PER 32  (.. 32768)                 a: 16385, 32767, 32768   b: 16385, 32767, 32768   d: 16385, 32768                   e: 32768 (info32)
  k_tile_sums / k_c_tile_sums,
  k_write_pack_infos / k_c_write       a: 32769 .. 526337       b: 32769 .. 526337       d: 32769, 34817, 524289; f: 32769  e: 32769, 34817 (info32); f: 32769 (none)
  k_scan_tile_sums / k_c_scan_tiles
    one round  (<= 256 tiles)          a: 32769 .. 524288       b: 32769 .. 524288       d: 32769, 34817; f: 32769         e: 32769, 34817; f: 32769
    two rounds (> 256 tiles)           a: 524289, 526337        b: 524289, 526337        d: 524289                         (k_c_scan_tiles is not a template: b)
  k_compact_samples                    c (on the begin_all of compact<i64,1>)

("info32" / "none": compact<i32,1> with and without the marcher's int32 packed_info table, one instantiation, a run-time pointer.)
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import marching_cubes_ref as MC
import scan_ref as R

pytestmark = pytest.mark.gpu

# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------
# csrc/scan.h: kSmallThreads = 1024 (threads of the one-workgroup kernels), kSmallMax = 32768 (largest n they take),
#              kThreads = 256 (threads of the tile kernels, and tile sums per round of the middle launch), kTile = kThreads * kItems = 2048
K_SMALL_THREADS, K_SMALL_MAX, K_THREADS, K_TILE = 1024, 32768, 256, 2048
PERS = (1, 2, 4, 8, 16, 32)

SIZES = ([0, 1, 63, 64, 65, K_SMALL_THREADS - 1, K_SMALL_THREADS, K_SMALL_THREADS + 1]              # empty, one wave +- 1, PER 1 | 2
         + [v for p in PERS[1:-1] for v in (p * K_SMALL_THREADS, p * K_SMALL_THREADS + 1)]          # PER p | 2 p
         + [K_SMALL_MAX - 1, K_SMALL_MAX, K_SMALL_MAX + 1]                                          # one workgroup | three launches
         + [17 * K_TILE, 17 * K_TILE + 1]                                                           # whole tiles, one count more
         + [K_THREADS * K_TILE, K_THREADS * K_TILE + 1]                                             # one round of tile sums | two
         + [(K_THREADS + 1) * K_TILE + 1])                                                          # 258 tiles, the last holds one count
assert SIZES == [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 32767, 32768, 32769, 34816, 34817,
                 524288, 524289, 526337], "the constants above no longer give the size list this file was written for"
assert PERS[-1] * K_SMALL_THREADS == K_SMALL_MAX

MARK = -7            # what every output holds before its kernel runs: an untouched row reads -7 whatever the allocator returns


def small_per(n):
    """PER of the one-workgroup kernel that takes n counts (scan.h / compact.h: per = ceil(n / kSmallThreads), next compiled value)"""
    assert 0 < n <= K_SMALL_MAX
    per = -(-n // K_SMALL_THREADS)
    return next(p for p in PERS if per <= p)


def n_tiles(n):
    return -(-n // K_TILE)


def single_positions(n):
    """where pattern (d) puts its one count: first, last, and the first index of the last tile (three launches) or of the last thread's
    chunk (one workgroup; only where that index exists)"""
    pos = {"single_first": 0, "single_last": n - 1}
    third = (n_tiles(n) - 1) * K_TILE if n > K_SMALL_MAX else (K_SMALL_THREADS - 1) * small_per(n)
    if third < n:
        pos["single_chunk"] = third
    seen, out = set(), {}
    for k, v in pos.items():
        if v not in seen:
            seen.add(v)
            out[k] = v
    return out


PATTERNS = ("zero", "one", "random", "single_first", "single_last", "single_chunk", "large")


def patterns_of(n):
    if n == 0:
        return ["zero"]
    return ["zero", "one", "random"] + list(single_positions(n)) + (["large"] if n >= 4096 else [])


def make_counts(n, pattern):
    rng = np.random.default_rng([n, PATTERNS.index(pattern)])
    if pattern == "zero":
        return np.zeros(n, np.int64)
    if pattern == "one":
        return np.ones(n, np.int64)
    if pattern == "random":                                  # [0, 7), about 30 % zeros
        c = rng.integers(1, 7, n, dtype=np.int64)
        c[rng.random(n) < 0.3] = 0
        return c
    if pattern == "large":                                   # uniform with mean 2^34 / n: the total is 2^34 (1 +- 1 / sqrt(3 n))
        return rng.integers(0, 2 * (2 ** 34 // n) + 1, n, dtype=np.int64)
    c = np.zeros(n, np.int64)
    c[single_positions(n)[pattern]] = 3
    return c


CASES = [(n, p) for n in SIZES for p in patterns_of(n)]
IDS = [f"{n}-{p}" for n, p in CASES]


def test_constants_are_the_headers():
    """the size list above is derived from these four numbers: a change of scan.h / compact.h must show up here, not pass unnoticed"""
    from nr3d_lib_amd import _hip as H
    scan_h = open(os.path.join(H.CSRC, "scan.h")).read()
    compact_h = open(os.path.join(H.CSRC, "compact.h")).read()

    def const(text, name):
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", text)
        assert m, name
        return m.group(1).strip()

    assert int(const(scan_h, "kThreads")) == K_THREADS
    assert int(const(scan_h, "kItems")) * K_THREADS == K_TILE and const(scan_h, "kTile") == "kThreads * kItems"
    assert int(const(scan_h, "kSmallMax")) == K_SMALL_MAX
    assert int(const(scan_h, "kSmallThreads")) == K_SMALL_THREADS == int(const(compact_h, "kSmallThreads"))
    assert int(const(compact_h, "kShift")) == 36
    for text in (scan_h, compact_h):                         # the PER ladder of both dispatchers
        assert [int(v) for v in re.findall(r"_SMALL\((\d+)\);", text)] == list(PERS)


# ---- the C entry points, called the way the bindings call them ---------------------------------------------------------------------------
def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _scan_tmp(n, dev):
    from nr3d_lib_amd import _hip as H
    nbytes = H.lib().nr3d_scan_tmp_bytes(max(n, 1))
    return torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=dev)


def scan_i64(dev, counts):
    """nr3d_pack_infos_from_n as bindings._pack_ops._pack_infos_from_n calls it -> (pack_infos [n, 2], total)"""
    from nr3d_lib_amd import _hip as H
    n = counts.shape[0]
    c = _dev(counts, dev)
    pi = torch.full((n, 2), MARK, dtype=torch.int64, device=dev)
    total = H.host_i64(1, dev)
    tmp = _scan_tmp(n, dev)
    H.check(H.lib().nr3d_pack_infos_from_n(n, H.ptr(c), H.ptr(pi), H.ptr(total), H.ptr(tmp), H.stream_of(tmp)))
    tot = H.wait_i64(total, dev)[0]
    torch.cuda.synchronize(dev)
    return pi, tot


def guard_rows(n):
    """rows behind the n a rank-indexed output needs.  A rank is written as an index: one that overshoots must land in memory of this
    test's own and be SEEN there.  The bound is what a wrong prefix can add at most -- every hit counted twice plus one wave of a tile
    (64 threads x kItems)."""
    return n + 64 * (K_TILE // K_THREADS) + 512


def compact_i64(dev, counts, tag):
    """nr3d_prune_compact_packs as bindings._pack_ops.packed_compression_compact calls it -> (begin_all [n], idx, pack_infos, totals);
    idx and pack_infos keep their guard rows"""
    from nr3d_lib_amd import _hip as H
    n = counts.shape[0]
    c = _dev(counts, dev)
    t = None if tag is None else _dev(tag, dev)
    rows = n + guard_rows(n)
    begin_all = torch.full((n,), MARK, dtype=torch.int64, device=dev)
    idx = torch.full((rows,), MARK, dtype=torch.int64, device=dev)
    pi = torch.full((rows, 2), MARK, dtype=torch.int64, device=dev)
    totals = H.host_i64(2, dev)
    tmp = _scan_tmp(n, dev)
    H.check(H.lib().nr3d_prune_compact_packs(n, H.ptr(c), H.ptr(t), H.ptr(begin_all), H.ptr(idx), H.ptr(pi), H.ptr(totals), H.ptr(tmp),
                                             H.stream_of(tmp)))
    tot = tuple(H.wait_i64(totals, dev))
    torch.cuda.synchronize(dev)
    return begin_all, idx, pi, tot


def _eq(got, want):
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = got.cpu()
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (got.dtype, got.shape, want.dtype, want.shape)
    if not torch.equal(got, want):
        bad = (got != want).reshape(got.shape[0], -1).any(1).nonzero().view(-1)
        raise AssertionError(f"{bad.numel()} of {got.shape[0]} rows differ, the first at {int(bad[0])}: got {got[bad[0]].tolist()}, "
                             f"want {want[bad[0]].tolist()}")


# ---- a. scan<int64, int64> -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,pattern", CASES, ids=IDS)
def test_scan_i64(dev, n, pattern):
    counts = make_counts(n, pattern)
    want_pi, want_total = R.pack_infos_from_counts(counts)
    if pattern == "large":
        assert 2 ** 33 <= want_total <= 2 ** 35, want_total
    got_pi, got_total = scan_i64(dev, counts)
    _eq(got_pi, want_pi)
    assert got_total == want_total


@pytest.mark.parametrize("n", [K_SMALL_THREADS + 1, K_SMALL_MAX + 1, K_THREADS * K_TILE + 1])
def test_scan_i64_producers(dev, n):
    """the scan behind its callers: get_pack_infos_from_n, the binding's own scan and interleave_arange"""
    from nr3d_lib_amd.bindings import _pack_ops as P
    from nr3d_lib_amd.graphics.pack_ops import get_pack_infos_from_n
    counts = make_counts(n, "random")
    want_pi, want_total = R.pack_infos_from_counts(counts)
    c = _dev(counts, dev)
    _eq(get_pack_infos_from_n(c), want_pi)
    pi, num = P._pack_infos_from_n(c)
    assert num == want_total
    _eq(pi, want_pi)
    out, nidx = P.interleave_arange(c, True)
    want_nidx = np.repeat(np.arange(n, dtype=np.int64), counts)
    _eq(nidx, want_nidx)
    _eq(out, np.arange(want_total, dtype=np.int64) - want_pi[want_nidx, 0])     # the concatenated per-pack aranges


# ---- b. compact<int64, 1> ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tagged", [False, True], ids=["index", "tag"])
@pytest.mark.parametrize("n,pattern", CASES, ids=IDS)
def test_compact_i64(dev, n, pattern, tagged):
    counts = make_counts(n, pattern)
    tag = (np.arange(n, dtype=np.int64) * 7919 + 13) % 1000003 - 500 if tagged else None
    want_begin, want_idx, want_pi, want_tot = R.compact_packs(counts, tag)
    if pattern == "large":
        assert 2 ** 33 <= want_tot[0] <= 2 ** 35, want_tot
    begin_all, idx, pi, tot = compact_i64(dev, counts, tag)
    assert tot == want_tot
    n_hit = want_tot[1]
    _eq(begin_all, want_begin)
    _eq(idx[:n_hit], want_idx)
    _eq(pi[:n_hit], want_pi)
    # a rank that overshoots writes behind the hits: every row from n_hit on, guard rows included, still holds the marker
    assert bool((idx[n_hit:] == MARK).all()) and bool((pi[n_hit:] == MARK).all())
    if pattern == "zero":
        assert tot == (0, 0) and bool((idx == MARK).all()) and bool((pi == MARK).all())


# ---- c. k_compact_samples on the begin_all of (b) --------------------------------------------------------------------------------------------
SAMPLE_LENS = [0, 1, 63, 64, 65, 128, 129, 200, 0, 64, 1, 0, 200, 127]        # 14 packs: four workgroups of four waves, the last half empty
SAMPLE_GAPS = [2, 0, 0, 1, 0, 0, 3, 0, 0, 0, 5, 0, 0, 1]                      # rows in FRONT of each pack that belong to no pack
SAMPLE_OUTPUTS = ("pidx", "f1", "f2", "f3", "l1")


@pytest.mark.parametrize("absent", [None] + list(SAMPLE_OUTPUTS))
@pytest.mark.parametrize("selector", ["all", "none", "random"])
def test_compact_samples(dev, selector, absent):
    from nr3d_lib_amd import _hip as H
    rng = np.random.default_rng(7)
    lens, gaps = np.array(SAMPLE_LENS, np.int64), np.array(SAMPLE_GAPS, np.int64)
    begin = np.cumsum(lens + gaps) - lens
    pack_infos = np.stack([begin, lens], 1)
    P, S = len(lens), int(begin[-1] + lens[-1]) + 4
    in_pack = np.zeros(S, bool)
    for b, l in pack_infos:
        in_pack[b:b + l] = True
    sel = {"all": np.ones(S, bool), "none": np.zeros(S, bool), "random": rng.random(S) < 0.5}[selector]
    if selector == "none":
        sel[~in_pack] = True                                 # rows outside every pack are nobody's: their selector must not be read
    keep = np.nonzero(sel & in_pack)[0].astype(np.int64)     # ascending pack, ascending sample
    kept_per_pack = np.array([int(sel[b:b + l].sum()) for b, l in pack_infos], np.int64)
    want_begin, _, _, (S2, _) = R.compact_packs(kept_per_pack)
    assert S2 == keep.shape[0]
    begin_all, _, _, tot = compact_i64(dev, kept_per_pack, None)
    assert tot[0] == S2
    _eq(begin_all, want_begin)

    src = dict(f1=rng.standard_normal(S).astype(np.float32), f2=rng.standard_normal(S).astype(np.float32),
               f3=rng.standard_normal((S, 3)).astype(np.float32), l1=rng.integers(-2 ** 40, 2 ** 40, S, dtype=np.int64))
    want = dict(pidx=keep, **{k: v[keep] for k, v in src.items()})
    tail = 8                                                 # rows behind the S2 kept samples: they keep the marker
    ins = {k: (None if k == absent else _dev(v, dev)) for k, v in src.items()}
    outs = {}
    for k in SAMPLE_OUTPUTS:
        if k == absent:
            outs[k] = None
        elif k in ("pidx", "l1"):
            outs[k] = torch.full((S2 + tail,), MARK, dtype=torch.int64, device=dev)
        else:
            outs[k] = torch.full((S2 + tail,) + ((3,) if k == "f3" else ()), float(MARK), dtype=torch.float32, device=dev)
    pi_t, sel_t = _dev(pack_infos, dev), _dev(sel, dev)
    H.check(H.lib().nr3d_prune_compact_samples(P, H.ptr(pi_t), H.ptr(begin_all), H.ptr(sel_t), H.ptr(ins["f1"]), H.ptr(ins["f2"]),
                                               H.ptr(ins["f3"]), H.ptr(ins["l1"]), H.ptr(outs["pidx"]), H.ptr(outs["f1"]),
                                               H.ptr(outs["f2"]), H.ptr(outs["f3"]), H.ptr(outs["l1"]), H.stream_of(pi_t)))
    torch.cuda.synchronize(dev)
    for k in SAMPLE_OUTPUTS:
        if k == absent:
            continue
        got = outs[k]
        if got.dtype == torch.float32:                       # moved, not computed: the bits
            _eq(got[:S2].view(torch.int32), want[k].view(np.int32))
        else:
            _eq(got[:S2], want[k])
        assert bool((got[S2:] == MARK).all()), k


# ---- d / e. scan<int32, int32> and compact<int32, 1> with info32 behind the occupancy marcher -------------------------------------------------
MARCH_STEP, MARCH_MAX_STEPS = 0.125, 4


def march_rays(n):
    """Rays inside an all-true grid over [-1, 1]^3 with dt_gamma = 0: every step is MARCH_STEP long and every probe hits, so ray i takes
    one sample per mid-point MARCH_STEP * (k + 1/2) below its own t_max, at most MARCH_MAX_STEPS.  t_max = MARCH_STEP * k with k = 0 for
    about 40 % of the rays and 1 .. 4 for the others (all exact in float32: no mid-point is near a t_max).  Origins within 0.25 of the
    centre and the longest march 0.5: no sample leaves the region of interest.  The tests read the counts from the marcher's output."""
    rng = np.random.default_rng(n)
    o = rng.uniform(-0.25, 0.25, (n, 3)).astype(np.float32)
    d = rng.standard_normal((n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    k = rng.integers(1, MARCH_MAX_STEPS + 1, n)
    k[rng.random(n) < 0.4] = 0
    return dict(rays_o=o, rays_d=d, t_min=np.zeros(n, np.float32), t_max=(k * MARCH_STEP).astype(np.float32),
                roi=np.array([-1, -1, -1, 1, 1, 1], np.float32), grid=np.ones((4, 4, 4), bool))


def assert_mixed(counts):
    """the inputs are worth the run: a quarter of the packs empty, a quarter not, three different lengths among those"""
    n = counts.shape[0]
    assert int((counts == 0).sum()) * 4 >= n and int((counts > 0).sum()) * 4 >= n, ((counts == 0).sum(), n)
    assert np.unique(counts[counts > 0]).shape[0] >= 3, np.unique(counts)


def _march_args(dev, n):
    r = march_rays(n)
    t = {k: _dev(v, dev) for k, v in r.items()}
    return t["rays_o"], t["rays_d"], t["t_min"], t["t_max"], t["roi"], t["grid"]


def _check_march(counts, begin, S, ridx):
    """the invariants of a marcher's pack table: begin is the exclusive cumsum of the counts, S their sum, the samples ray by ray"""
    n = counts.shape[0]
    assert_mixed(counts)
    want_pi, want_total = R.pack_infos_from_counts(counts)
    assert S == want_total
    assert np.array_equal(begin.astype(np.int64), want_pi[:, 0])
    assert ridx.shape[0] == S
    assert np.array_equal(ridx.astype(np.int64), np.repeat(np.arange(n, dtype=np.int64), counts))


MARCH_SIZES = [1024, 1025, 4097, 8193, 16385, 32768, 32769, 34817, 524289]


@pytest.mark.parametrize("n", MARCH_SIZES)
def test_march_scan_i32(dev, n):
    from nr3d_lib_amd.bindings import _occ_grid as G
    packed_info, t_starts, t_ends, ridx, gidx = G.ray_marching(*_march_args(dev, n), G.AABB, MARCH_STEP, MARCH_STEP, 0.0, MARCH_MAX_STEPS, True)
    assert packed_info.dtype == torch.int32 and tuple(packed_info.shape) == (n, 2) and ridx.dtype == torch.int32
    pi = packed_info.cpu().numpy()
    _check_march(pi[:, 1].astype(np.int64), pi[:, 0], int(t_starts.shape[0]), ridx.cpu().numpy())
    assert t_ends.shape == t_starts.shape and gidx.shape[0] == t_starts.shape[0]


FINISHED_SIZES = [1024, 1025, 4096, 8192, 16384, 32768, 32769, 34817]


@pytest.mark.parametrize("n", FINISHED_SIZES)
def test_march_finished_compact_i32(dev, n):
    """compact<int32, 1> with the int32 table: nr3d_ray_marching_count with with_hit_rays = 1 directly (the binding keeps packed_info to
    itself), then the binding end to end"""
    from nr3d_lib_amd import _hip as H
    from nr3d_lib_amd.bindings import _occ_grid as G
    rays_o, rays_d, t_min, t_max, roi, grid = args = _march_args(dev, n)
    rows = n + guard_rows(n)
    packed_info = torch.full((n, 2), MARK, dtype=torch.int32, device=dev)
    ridx_hit = torch.full((rows,), MARK, dtype=torch.int64, device=dev)
    pack_infos = torch.full((rows, 2), MARK, dtype=torch.int64, device=dev)
    totals = H.host_i64(2, dev)
    tmp = _scan_tmp(n, dev)
    res = (C.c_int32 * 3)(*grid.shape)
    H.check(H.lib().nr3d_ray_marching_count(
        n, H.ptr(rays_o), H.ptr(rays_d), H.ptr(t_min), H.ptr(t_max), H.ptr(roi), res, H.ptr(grid), int(G.AABB), MARCH_STEP, MARCH_STEP, 0.0,
        MARCH_MAX_STEPS, False, None, 0, H.ptr(packed_info), H.ptr(totals), H.ptr(tmp), None, 0, 1, H.ptr(ridx_hit), H.ptr(pack_infos),
        H.stream_of(tmp)))
    S, n_hit = H.wait_i64(totals, dev)
    torch.cuda.synchronize(dev)
    pi = packed_info.cpu().numpy()
    counts = pi[:, 1].astype(np.int64)
    assert_mixed(counts)
    want_begin, want_idx, want_pi, want_tot = R.compact_packs(counts)
    assert (S, n_hit) == want_tot
    assert np.array_equal(pi[:, 0].astype(np.int64), want_begin)
    _eq(ridx_hit[:n_hit], want_idx)                          # == nonzero(counts)
    _eq(pack_infos[:n_hit], want_pi)                         # == the int64 rows of packed_info where the count is above 0
    assert np.array_equal(want_pi, pi[counts > 0].astype(np.int64))
    assert bool((ridx_hit[n_hit:] == MARK).all()) and bool((pack_infos[n_hit:] == MARK).all())
    # the binding, with its sample cache: the same tables, and the samples ray by ray
    out = G.ray_marching_finished(*args, G.AABB, MARCH_STEP, MARCH_STEP, 0.0, MARCH_MAX_STEPS, True)
    assert out["n_hit"] == n_hit
    _eq(out["ridx_hit"], want_idx)
    _eq(out["pack_infos"], want_pi)
    _check_march(counts, want_begin, int(out["t_starts"].shape[0]), out["ridx"].cpu().numpy())


# ---- f. compact<int32, 1> without info32 and the tracer's own scan<int32, int32> ---------------------------------------------------------------
def trace_rays(n):
    """An 8^3 grid over [-1, 1]^3 whose slabs iz = 2, 4, 6 are occupied.  About 40 % of the rays start outside the grid and point away from
    it: no segment.  The others start inside slab 2 (z in [-0.45, -0.3]) and run towards +z (d_z > 0.95): slab 2 ends at t < 0.22, slab 4
    begins at t in (0.3, 0.48), slab 6 at t in (0.8, 1.0); rays_far is one of 0.25, 0.6, 1.2 -- one, two or three segments, no far near an
    entry.  -> (grid, rays_o, rays_d, near, far, hit)"""
    rng = np.random.default_rng(1000 + n)
    grid = np.zeros((8, 8, 8), bool)
    grid[:, :, [2, 4, 6]] = True
    hit = rng.random(n) >= 0.4
    o = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), rng.uniform(-0.45, -0.3, n)], 1)
    d = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), np.ones(n)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o[~hit] = [0.0, 0.0, -3.0]
    d[~hit, 2] *= -1
    far = rng.choice(np.array([0.25, 0.6, 1.2]), n)
    return grid, o.astype(np.float32), d.astype(np.float32), np.zeros(n, np.float32), far.astype(np.float32), hit


@pytest.mark.parametrize("n", [2 * K_SMALL_THREADS + 1, K_SMALL_MAX + 1])
def test_sphere_trace_compact_and_scan_i32(dev, n):
    from nr3d_lib_amd.bindings import _sphere_trace as ST
    grid, o, d, near, far, hit = trace_rays(n)
    g = ST.DenseGrid(8, 8, 8, _dev(grid, dev))
    rays_o, rays_d = _dev(o, dev), _dev(d, dev)
    valid, pack, segs, _, _ = ST.ray_march(g, rays_o, rays_d, _dev(near, dev), _dev(far, dev))
    assert valid.dtype == torch.int64 and pack.dtype == torch.int32 and tuple(pack.shape) == (valid.shape[0], 2)
    valid_np, pack_np = valid.cpu().numpy(), pack.cpu().numpy().astype(np.int64)
    # the hit rays are the rays aimed at the grid, in ascending order; their table is the exclusive cumsum of its own counts
    assert np.array_equal(valid_np, np.nonzero(hit)[0])
    counts = np.zeros(n, np.int64)
    counts[valid_np] = pack_np[:, 1]
    assert_mixed(counts)
    want_begin, want_idx, want_pi, (total, n_hit) = R.compact_packs(counts)
    assert n_hit == valid_np.shape[0] and total == segs.shape[0]
    assert np.array_equal(valid_np, want_idx) and np.array_equal(pack_np, want_pi)

    # the tracer's scan<int32, int32>: sample_on_segments over ALL n rays -- the rays without a segment enter with an empty pack, are
    # OUT from the start and take no sample
    full = np.stack([want_begin, counts], 1).astype(np.int32)
    tracer = ST.SphereTracer(0.01, 1.0)
    tracer.init_rays(rays_o, rays_d, torch.arange(n, dtype=torch.int64, device=dev), _dev(full, dev), segs)
    assert tracer.n_rays(ST.ALIVE) == n
    offs, cnts, depths, pos = tracer.sample_on_segments(0.05)
    assert offs.dtype == torch.int32 and cnts.dtype == torch.int32 and tuple(offs.shape) == (n,) == tuple(cnts.shape)
    c = cnts.cpu().numpy().astype(np.int64)
    assert_mixed(c)
    assert np.array_equal(c > 0, hit)
    want_pi, want_total = R.pack_infos_from_counts(c)
    assert depths.shape[0] == want_total == pos.shape[0]
    assert np.array_equal(offs.cpu().numpy().astype(np.int64), want_pi[:, 0])


# ---- g. marching cubes above the smallest class: Nx * Ny rows are scanned (scan<int64, int64>, twice) -------------------------------------------
@pytest.mark.parametrize("shape", [(41, 25, 3), (64, 33, 2)], ids=lambda s: "x".join(map(str, s)))
def test_marching_cubes_rows(dev, shape):
    from nr3d_lib_amd.bindings._marching_cubes import marching_cubes
    rows = shape[0] * shape[1]
    assert small_per(rows) == {1025: 2, 2112: 4}[rows]
    vol = np.random.default_rng(rows).standard_normal(shape).astype(np.float32)
    want_v, want_f = MC.marching_cubes(vol, 0.0)
    got_v, got_f = marching_cubes(_dev(vol, dev), 0.0)
    assert want_f.shape[0] > rows                            # most rows carry triangles: the prefix matters at every row
    _eq(got_f, want_f)
    _eq(got_v.view(torch.int32), want_v.view(np.int32))
