"""CPU: the argument checks of nr3d_lotd_bwd_dparam, the one dL/dparam entry of a single block (include/nr3d_hip.h, ABI 20).  Every
call has n_points = 0 and the address of a host float wherever a pointer must not be NULL: the checks come before the early return
and before any pointer is read, so no GPU call is reached."""
import ctypes as C
import re
import subprocess

import pytest

from nr3d_lib_amd import _hip as H

# the level-range, typed and second-order twins of ABI 19 (in pieces: a search of the tree for the old names finds nothing)
REMOVED = ["nr3d_lotd_" + a + "_" + b for a, b in (("bwd_dparam", "levels"), ("bwd_dparam", "typed"), ("bwd_bwd", "dparam"))]


@pytest.fixture(scope="module")
def call(hiplib):
    from nr3d_lib_amd.bindings import _lotd
    m = _lotd.LoDMeta(3, [8, 11, 15, 21], [2] * 4, ["Dense", "Dense", "Hash", "Hash"], 2 ** 12)
    host = C.c_float(0.0)
    a = C.addressof(host)
    base = dict(grad_dtype=H.F32, dL_ddLdx=None, param_dtype=H.F32, batch_inds=None, batch_offsets=None, batch_data_size=0,
                n_batches=1, min_level=0, max_level=m.n_levels, out_dtype=H.F32, assign=0, fold=None)

    def call_(**kw):
        k = dict(base, **{n: (a if v is True else v) for n, v in kw.items()})
        rc = hiplib.nr3d_lotd_bwd_dparam(
            C.byref(m._cmeta()), a, 0, k["grad_dtype"], a, m.n_encoded_dims, 1, k["dL_ddLdx"], a, k["param_dtype"], a,
            k["batch_inds"], k["batch_offsets"], k["batch_data_size"], k["n_batches"], k["min_level"], k["max_level"],
            k["out_dtype"], k["assign"], a, None, 0, k["fold"], None)
        return rc, hiplib.nr3d_last_error().decode()
    return call_


# (arguments, True standing for a non-NULL pointer; what the message has to name)
REFUSALS = {
    "second order with a level range": (dict(dL_ddLdx=True, min_level=1), ["min_level", "dL_ddLdx"]),
    "second order with half dL_dy": (dict(dL_ddLdx=True, grad_dtype=H.F16), ["grad_dtype", "dL_ddLdx"]),
    "second order with half dL_dparam": (dict(dL_ddLdx=True, out_dtype=H.F16), ["out_dtype", "dL_ddLdx"]),
    "half dL_dy with a level range": (dict(grad_dtype=H.F16, min_level=2), ["grad_dtype", "min_level"]),
    "half dL_dparam with a level range": (dict(out_dtype=H.F16, min_level=2), ["out_dtype", "min_level"]),
    "half dL_dy with batch_inds": (dict(grad_dtype=H.F16, batch_inds=True), ["grad_dtype", "batch_inds"]),
    "half dL_dparam with batch_offsets": (dict(out_dtype=H.F16, batch_offsets=True), ["out_dtype", "batch_offsets"]),
    "half dL_dy with batch_data_size": (dict(grad_dtype=H.F16, batch_data_size=4), ["grad_dtype", "batch_data_size"]),
    "half dL_dparam with n_batches": (dict(out_dtype=H.F16, n_batches=2), ["out_dtype", "n_batches"]),
    "second order with fold": (dict(dL_ddLdx=True, fold=True), ["fold", "dL_ddLdx"]),
    "fold with a level range": (dict(fold=True, min_level=1), ["fold", "min_level"]),
    "negative min_level": (dict(min_level=-1), ["min_level"]),
    "grad_dtype not f32 / f16": (dict(grad_dtype=H.F64), ["grad_dtype"]),
    "param_dtype not f32 / f16": (dict(param_dtype=H.I32), ["param_dtype"]),
    "out_dtype not f32 / f16": (dict(out_dtype=H.F64), ["out_dtype"]),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refused_combinations_name_the_argument(call, what):
    kw, names = REFUSALS[what]
    rc, msg = call(**kw)
    assert rc != 0, what
    for n in names:
        assert n in msg, (what, msg)


@pytest.mark.parametrize("kw", [dict(), dict(dL_ddLdx=True), dict(min_level=1, max_level=2), dict(min_level=3, max_level=1),
                                dict(max_level=-1), dict(param_dtype=H.F16)],
                         ids=["first order", "second order", "level range", "empty range", "max_level -1", "half tables"])
def test_legal_empty_calls_return_zero(call, kw):
    rc, msg = call(**kw)
    assert rc == 0, msg


def test_the_twin_entries_are_gone(hiplib):
    from nr3d_lib_amd import _abi
    nm = subprocess.run(["nm", "-D", "--defined-only", H.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (nr3d_[A-Za-z0-9_]+)", nm))
    assert "nr3d_lotd_bwd_dparam" in exported and "nr3d_lotd_bwd_dparam" in _abi.SIGNATURES
    for name in REMOVED:
        assert name not in exported and name not in _abi.SIGNATURES and not hasattr(hiplib, name), name
    assert _abi.ABI_VERSION >= 20 and len(_abi.SIGNATURES["nr3d_lotd_bwd_dparam"][1]) == 24
