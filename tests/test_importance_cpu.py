"""CPU: models/importance.py without a kernel -- the chain against what the reference's own classes returned (tests/golden/
ref_importance.npz, recorded by tests/golden/make_golden_importance.py, whose ``scenario`` runs here on the package), the restatement
the GPU tests compare bytes with (tests/importance_ref.py) pinned on literals written out by hand and on the chain, and the new
entries of the C boundary."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import importance_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_importance as gold  # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ref_importance.npz")))


@pytest.fixture(scope="module")
def replayed():
    from nr3d_lib_amd.models import importance
    assert importance.FUSED_IMPORTANCE in (True, False) and importance.CHECK_VAL is True
    return gold.scenario(importance)


def test_cpu_route_equals_every_recorded_array(recorded, replayed):
    """a seeded CPU run of the package returns the reference's own numbers, bit for bit: updates, CDFs, every sampler, the schedule"""
    assert sorted(recorded) == sorted(replayed)
    for k in sorted(recorded):
        a, b = torch.from_numpy(recorded[k]), torch.from_numpy(np.asarray(replayed[k]))
        assert a.dtype == b.dtype and torch.equal(a, b), k
    # what was recorded is what the issue lists
    assert all(recorded[f"{n}x{h}x{w}/{c}/clean_equal"].tolist() == [1, 1] for (n, h, w) in gold.SHAPES for c in gold.CDF_CONFIGS)
    assert recorded["schedule/max"].shape == (600, 2) and recorded["schedule/max"][:, 0].max() == 50
    assert recorded["schedule/nomax"][:, 0].max() > 50
    assert recorded["imp/13/i"].shape == (13,) and recorded["imp/1000/xy"].shape == (1000, 2)


def test_recorded_state_dicts_load_strict(recorded):
    from nr3d_lib_amd.models.importance import ErrorMap, ImpSampler
    sd = {k.split("/", 2)[2]: torch.from_numpy(v) for k, v in recorded.items() if k.startswith("errmap/state_dict/")}
    assert list(sd) == ["error_map"]
    m = ErrorMap(3, (5, 7))
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.error_map, sd["error_map"])
    assert list(m.state_dict()) == ["error_map"]
    assert sorted(n for n, _ in m.named_buffers()) == ["error_map", "min_cdf_img", "min_cdf_x_cond_y", "min_cdf_y"]
    sd = {k.split("/", 2)[2]: torch.from_numpy(v) for k, v in recorded.items() if k.startswith("imp/state_dict/")}
    s = ImpSampler({"a": (ErrorMap(3, (5, 7)), 0.3), "b": (ErrorMap(3, (9, 4), min_pdf=0.0), 0.2)}, frac_uniform=0.5)
    s.load_state_dict(sd, strict=True)
    assert sorted(sd) == ["error_maps.a.error_map", "error_maps.b.error_map"]
    # the fused update's scratch is a plain attribute: an update changes no key
    m.update_error_map(0, torch.tensor([[0.5, 0.5]]), torch.tensor([1.0]))
    assert list(m.state_dict()) == ["error_map"]


def test_module_surface():
    from nr3d_lib_amd.models import importance as I
    m = I.ErrorMap(2, (4, 6), min_pdf=0.02, max_pdf=3.0, n_steps_init=7, n_steps_max=9, n_steps_growth_factor=2.0)
    assert (m.n_images, m.res_y, m.res_x, m.min_pdf, m.max_pdf) == (2, 4, 6, 0.02, 3.0)
    assert (m.n_steps_between_update, m.n_steps_since_update, m.n_steps_max, m.n_steps_growth_factor) == (7, 0, 9, 2.0)
    assert m.cdf_x_cond_y is None and m.cdf_y is None and m.cdf_img is None and m.device == torch.device("cpu")
    for name in ("update_error_map", "get_normalized_error_map", "construct_cdf", "construct_cdf_and_clean_error_map", "step_error_map",
                 "get_pdf_image", "sample_pixel", "sample_img", "sample_img_pixel"):
        assert callable(getattr(m, name))
    assert I.UPDATE_SCRATCH_MAX_BYTES == 2 ** 30
    with pytest.raises(AssertionError):
        m.update_error_map(0, torch.tensor([[0.5, 0.5]]), torch.tensor([-1.0]))
    saved = I.CHECK_VAL
    I.CHECK_VAL = False
    try:
        m.update_error_map(0, torch.tensor([[0.5, 0.5]]), torch.tensor([-1.0]))      # the chain then writes what it is given
        assert float(m.error_map.sum()) == -1.0
    finally:
        I.CHECK_VAL = saved
    assert I.imp_segments(13, 0.5, [0.3, 0.2]) == (6, [3, 4]) and I.imp_segments(3, 0.5, [0.1, 0.4]) == (1, [0, 2])


# ---- the restatement, pinned by hand -----------------------------------------------------------------------------------------------
def test_restatement_update_literals():
    """a 1 x 2 x 2 map, two samples in its one cell: every contribution is a dyadic number, so the sums are exact"""
    m0 = np.array([[[1.0, 2.0], [3.0, 4.0]]], F)
    # x = 0.25 -> wf = 0.5, w = 0, w_w = 0.5; y = 0.125 -> hf = 0.25, h = 0, w_h = 0.25; val = 8:
    #   (h, w) 0.75 * 0.5 * 8 = 3;  (h+1, w) 0.25 * 0.5 * 8 = 1;  (h, w+1) 3;  (h+1, w+1) 1
    # x = 0.5 -> wf = 1, w = 1, w_w = 0, clamped to w = 0; y = 0 -> h = 0, w_h = 0; val = 0.5: (h, w) 0.5, nothing elsewhere
    got = ref.update(m0, 0, [[0.25, 0.125], [0.5, 0.0]], [8.0, 0.5])
    assert got.tolist() == [[[4.5, 5.0], [4.0, 5.0]]]
    assert ref.cells_touched_twice(0, [[0.25, 0.125], [0.5, 0.0]], [8.0, 0.5], 1, 2, 2)
    assert not ref.cells_touched_twice(0, [[0.25, 0.125]], [8.0], 1, 2, 2)
    # x == 1: wf = 2, w_w = 0 BEFORE the clamp to column res_x - 2 = 0, so the whole value lands in column 0 (the reference's quirk)
    assert ref.update(np.zeros((1, 2, 2), F), 0, [[1.0, 0.0]], [2.0]).tolist() == [[[2.0, 0.0], [0.0, 0.0]]]
    # dropped: frames outside [0, N), non-finite x / val, negative val
    for i, xy, v in ((-1, [0.5, 0.5], 1.0), (1, [0.5, 0.5], 1.0), (0, [np.nan, 0.5], 1.0), (0, [0.5, 0.5], np.inf), (0, [0.5, 0.5], -1.0)):
        assert np.array_equal(ref.update(m0, i, [xy], [v]), m0)
    # fixed point: 2^-32 units, half to even, the clamp at 2^16
    assert ref.fix(F(1.0)) == 2 ** 32 and ref.fix(F(2.0 ** -33)) == 0 and ref.fix(F(3 * 2.0 ** -33)) == 2 and ref.fix(F(1e9)) == 2 ** 48
    assert ref.fix(F(-0.5)) == -2 ** 31 and ref.unfix(2 ** 32 + 2 ** 31) == F(1.5)
    # 40 000 samples into one cell: two chunks, each sum exact
    n = 40000
    got = ref.update(np.zeros((1, 2, 2), F), 0, np.zeros((n, 2), F), np.full(n, 0.25, F))
    assert got[0, 0, 0] == F(n * 0.25)


def test_restatement_scan_literals():
    # Kogge-Stone over 4 of the 64 lanes: ((a) , (a+b), (b+c)+a, ((c+d) + (a+b))) -- the tree, not left to right
    a, b, c, d = F(1.0), F(2.0 ** -24), F(2.0 ** -24), F(2.0 ** -24)
    s, total = ref.scan(np.array([a, b, c, d], F))
    assert s.tolist() == [1.0, 1.0, float(F(F(b + c) + a)), float(F(F(c + d) + F(a + b)))]
    assert s[2] == F(1.0 + 2.0 ** -23) and s[3] == F(1.0 + 2.0 ** -23) and total == s[3]
    # integers: exact, and the carry crosses the chunks
    s, total = ref.scan(np.ones((2, 130), F))
    assert np.array_equal(s, np.tile(np.arange(1, 131, dtype=F), (2, 1))) and total.tolist() == [130.0, 130.0]
    # a uniform 1 x 2 x 2 map with min_pdf 0.5: every CDF is the ramp
    cx, cy, ci, e = ref.construct_cdf(np.ones((1, 2, 2), F), 0.5)
    assert cx.tolist() == [[[0.5, 1.0], [0.5, 1.0]]] and cy.tolist() == [[0.5, 1.0]] and ci.tolist() == [1.0]
    cx, _, _, e = ref.construct_cdf(np.array([[[1.0, 3.0], [5.0, 1.0]]], F), 0.0, max_pdf=1.0)
    assert e.tolist() == [[[1.0, 1.0], [1.0, 1.0]]] and cx.tolist() == [[[0.5, 1.0], [0.5, 1.0]]]


def test_restatement_search_literals():
    row = np.array([0.25, 0.5, 0.5, 1.0], F)
    assert [ref.lower(row, F(u)) for u in (0.1, 0.25, 0.3, 0.5, 0.75, 1.0, 2.0)] == [0, 0, 1, 1, 3, 3, 3]
    k, v = ref.invert(row, F(0.375))            # bin 1: (0.375 - 0.25) / 0.25 = 0.5 -> (0.5 + 1) / 4
    assert (k, float(v)) == (1, 0.375)
    k, v = ref.invert(row, F(0.125))            # bin 0, prev = 0
    assert (k, float(v)) == (0, 0.125)
    cdf_img = np.array([0.5, 1.0], F)
    cdf_y = np.array([[0.5, 1.0], [0.25, 1.0]], F)
    cdf_x = np.tile(np.array([0.5, 1.0], F), (2, 2, 1))
    i, xy = ref.sample(cdf_img, cdf_y, cdf_x, None, [0.75], [0.25], [0.625])
    # image 1; y: bin 1 of [0.25, 1]: (0.625 - 0.25) / 0.75 = 0.5 -> 0.75; x: bin 0: 0.5 -> 0.25
    assert i.tolist() == [1] and xy.tolist() == [[0.25, 0.75]]
    assert ref.sample(None, cdf_y, cdf_x, -1, None, [0.25], [0.625])[0].tolist() == [1]


# ---- the chain against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 3, 130), (4, 65, 9), (1, 8, 8)])
@pytest.mark.parametrize("per_sample_frames", [False, True])
def test_chain_update_equals_the_restatement_on_lattice_inputs(shape, per_sample_frames):
    from nr3d_lib_amd.models.importance import errmap_update
    N, H, W = shape
    i, xy, val = ref.lattice_update(N, H, W, 5, per_sample_frames)
    assert len(val) >= 4 and not ref.cells_touched_twice(i, xy, val, N, H, W)
    m0 = (np.random.default_rng(1).integers(0, 64, shape) / 16.0).astype(F)
    got = torch.from_numpy(m0.copy())
    errmap_update(got, torch.from_numpy(i) if per_sample_frames else i, torch.from_numpy(xy), torch.from_numpy(val))
    want = ref.update(m0, i, xy, val)
    assert not np.array_equal(want, m0) and torch.equal(got, torch.from_numpy(want))


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 3, 130), (1, 4, 64)])
def test_chain_sampling_equals_the_restatement(shape):
    """the searches and the two inversions on the CPU chain helper, CDFs from the chain's own construct_cdf"""
    from nr3d_lib_amd.models.importance import errmap_construct_cdf, errmap_sample_from_uniform
    g = torch.Generator().manual_seed(3)
    e = torch.empty(shape).uniform_(0.2, 1, generator=g)
    cx, cy, ci = errmap_construct_cdf(e, 0.01)
    u = torch.rand(3, 200, generator=g).clamp_(1e-6, 1 - 1e-6)
    u[0, :shape[0]], u[2, :shape[1]], u[1, :7] = ci, cy[0], cx[0, 0, :7]            # exact CDF elements: ties take the first index
    u.clamp_(1e-6, 1 - 1e-6)
    i, xy = errmap_sample_from_uniform(ci, cy, cx, None, u[0], u[1], u[2])
    ri, rxy = ref.sample(ci.numpy(), cy.numpy(), cx.numpy(), None, u[0].numpy(), u[1].numpy(), u[2].numpy())
    assert torch.equal(i, torch.from_numpy(ri)) and torch.equal(xy, torch.from_numpy(rxy))
    frames = torch.randint(shape[0], [200], generator=g)
    for f in (shape[0] - 1, frames):
        _, xy = errmap_sample_from_uniform(None, cy, cx, f, None, u[1], u[2])
        _, rxy = ref.sample(None, cy.numpy(), cx.numpy(), f if isinstance(f, int) else f.numpy(), None, u[1].numpy(), u[2].numpy())
        assert torch.equal(xy, torch.from_numpy(rxy))


def test_restatement_cdf_is_close_to_the_chain_and_float64():
    """the fixed scan order against torch's serial CPU cumsum and a float64 evaluation, within the bound the GPU test uses"""
    from nr3d_lib_amd.models.importance import errmap_construct_cdf
    for shape, kw in (((3, 5, 7), dict(min_pdf=0.01)), ((2, 3, 130), dict(min_pdf=0.0)), ((4, 65, 9), dict(min_pdf=0.01, max_pdf=0.7))):
        e = torch.empty(shape).uniform_(0.2, 1, generator=torch.Generator().manual_seed(4))
        want = ref.construct_cdf(e.numpy(), **kw)
        exact = ref.construct_cdf_f64(e.numpy(), **kw)
        chain = errmap_construct_cdf(e.clone(), kw["min_pdf"], kw.get("max_pdf"))
        for w, x, c in zip(want, exact, chain):
            L = w.shape[-1]
            bound = (9 + -(-L // 64)) * 2.0 ** -24
            assert np.all(np.abs(w - x) <= bound * np.abs(x))
            assert np.all(np.abs(c.numpy() - x) <= (9 + L) * 2.0 ** -24 * np.abs(x))
            assert np.all(np.diff(w, axis=-1) >= 0)


# ---- the C boundary ----------------------------------------------------------------------------------------------------------------
def test_abi_has_the_entry_points_and_keeps_its_number():
    from nr3d_lib_amd import _abi
    assert _abi.ABI_VERSION == 30
    header = open(os.path.join(ROOT, "include", "nr3d_hip.h")).read()
    assert re.search(r"#define\s+NR3D_ABI_VERSION\s+30\b", header)
    for name in ("nr3d_importance_sample", "nr3d_importance_update", "nr3d_importance_construct_cdf"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert _abi.SIGNATURES[name][0] == "int" and _abi.SIGNATURES[name][1][-1] == "ptr"
    assert _abi.SIGNATURES["nr3d_importance_sample"][1] == ["uint32_t", "uint32_t", "uint32_t", "int", "ptr", "ptr", "ptr", "ptr", "int",
                                                            "int64_t", "ptr", "ptr", "ptr", "ptr"]
    assert _abi.SIGNATURES["nr3d_importance_update"][1] == ["uint32_t"] * 4 + ["int64_t"] + ["ptr"] * 6
    assert _abi.SIGNATURES["nr3d_importance_construct_cdf"][1] == (["uint32_t"] * 3 + ["ptr", "float", "float", "int", "float", "int"]
                                                                   + ["ptr"] * 6)
    assert "importance.hip" in open(os.path.join(ROOT, "nr3d_lib_amd", "csrc", "Makefile")).read()
    from nr3d_lib_amd.bindings import _importance as B
    assert (B.MAX_MAPS, B.UPDATE_CHUNK) == (8, 2 ** 15)
    assert re.search(r"#define\s+NR3D_IMPORTANCE_MAX_MAPS\s+8\b", header) and re.search(r"#define\s+NR3D_IMPORTANCE_UPDATE_CHUNK\s+32768\b", header)
    import ctypes
    assert ctypes.sizeof(B._CMap) == 40


def test_binding_refuses_cpu_tensors():
    from nr3d_lib_amd.bindings import _importance as B
    e = torch.zeros(2, 3, 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        B.construct_cdf(e, 0.01)
    with pytest.raises(RuntimeError, match="GPU only"):
        B.update(e, torch.zeros(2, 3, 4, dtype=torch.int64), 0, torch.zeros(1, 2), torch.zeros(1))
    with pytest.raises(RuntimeError, match="GPU only"):
        B.sample([(torch.zeros(2), torch.zeros(2, 3), e)], [0], 0, 2, torch.zeros(5), torch.zeros(5), torch.zeros(5))
