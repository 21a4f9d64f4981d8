"""What the five kinds of cvr_precond share, pinned on the 12 x 12 tridiagonal Laplacian: the texts by which an entry point declines an object of a
kind it does not take (written from the kinds' names, so every kind's text is spelled out here), the constructors' shared staging of a CSR view --
host arrays and device arrays give the same object, and the checks both forms share return the same codes and texts -- and that a constructor whose
build fails hands back the build's own message behind the teardown of the half-made object."""
import ctypes as C

import numpy as np
import pytest
import torch

import cvr_amd
from cvr_amd import capi

pytestmark = pytest.mark.gpu

N = 12
KINDS = {"block-Jacobi": 0, "Chebyshev": 1, "ILU(0)": 2, "FSAI": 3, "AMG": 4}
AMG_OPTIONS = dict(coarse_size=3)          # three levels (12, 4, 2 rows): level 1 gets a handle of the object's own


def laplacian(dtype=np.float64):
    rp, ci, va = [0], [], []
    for i in range(N):
        for j in (i - 1, i, i + 1):
            if 0 <= j < N:
                ci.append(j)
                va.append(2.0 if j == i else -1.0)
        rp.append(len(ci))
    return np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.array(va, dtype=dtype)


def on_device(*arrays):
    out = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def system():
    rp, ci, va = laplacian()
    A = cvr_amd.CvrMatrix(N, N, rp, ci, va)
    objs = {"block-Jacobi": capi.Precond.block_jacobi(rp, ci, va, 4), "Chebyshev": capi.Precond.chebyshev(A, 3, 0.1, 4.0), "ILU(0)": capi.Precond.ilu0(rp, ci, va),
            "FSAI": capi.Precond.fsai(rp, ci, va), "AMG": capi.Precond.amg(A, rp, ci, va, **AMG_OPTIONS)}
    yield A, objs
    for p in objs.values():
        p.close()
    A.close()


# ---- the texts of the entry points that decline a kind ----
def test_every_kind_is_declined_in_the_same_words(system):
    A, objs = system
    L = capi.lib()
    b, x = on_device(np.ones(N), np.zeros(N))
    hb, hx, out = np.ones(N), np.zeros(N), np.zeros(64)
    opt, res = capi.CgOptions(), capi.CgResult()
    L.cvr_cg_default_options(C.byref(opt))
    only_jacobi = {
        "cvr_precond_export": lambda p: L.cvr_precond_export(p, out.ctypes.data),
        "cvr_precond_apply_multi_device": lambda p: L.cvr_precond_apply_multi_device(p, b.data_ptr(), 1, x.data_ptr(), 1, 1, None),
        "cvr_pcg_multi": lambda p: L.cvr_pcg_multi_device(A._h, p, b.data_ptr(), 1, x.data_ptr(), 1, 1, C.byref(opt), C.byref(res), None),
        "cvr_pcg_multi ": lambda p: L.cvr_pcg_multi(A._h, p, hb.ctypes.data, hx.ctypes.data, 1, C.byref(opt), C.byref(res)),
    }
    jacobi_or_ilu0 = {
        "cvr_pbicgstab": lambda p: L.cvr_pbicgstab_device(A._h, p, b.data_ptr(), x.data_ptr(), C.byref(opt), C.byref(res), None),
        "cvr_pbicgstab ": lambda p: L.cvr_pbicgstab(A._h, p, hb.ctypes.data, hx.ctypes.data, C.byref(opt), C.byref(res)),
        "cvr_pgmres": lambda p: L.cvr_pgmres_device(A._h, p, b.data_ptr(), x.data_ptr(), 30, C.byref(opt), C.byref(res), None),
        "cvr_pgmres ": lambda p: L.cvr_pgmres(A._h, p, hb.ctypes.data, hx.ctypes.data, 30, C.byref(opt), C.byref(res)),
    }
    for name, kind in KINDS.items():
        p = objs[name]._p
        if name != "block-Jacobi":
            for entry, call in only_jacobi.items():
                assert call(p) == capi.ERR_STATE, (name, entry)
                assert capi.last_error() == f"{entry.strip()}: the preconditioner is of kind {kind} ({name}): this entry point takes block-Jacobi objects (kind 0) only"
        if name not in ("block-Jacobi", "ILU(0)"):
            for entry, call in jacobi_or_ilu0.items():
                assert call(p) == capi.ERR_STATE, (name, entry)
                assert capi.last_error() == (f"{entry.strip()}: the preconditioner is of kind {kind} ({name}): this entry point takes block-Jacobi and ILU(0) objects "
                                             "(kinds 0 and 2) only")
    torch.cuda.synchronize()
    assert not x.cpu().numpy().any() and not hx.any() and not out.any()          # nothing ran


def test_every_typed_call_names_the_kind_it_was_given(system):
    _, objs = system
    L = capi.lib()
    buf = np.zeros(256)
    ptr = buf.ctypes.data
    typed = {
        "Chebyshev": {"cvr_precond_chebyshev_info": lambda p: L.cvr_precond_chebyshev_info(p, C.byref(capi.ChebyshevInfo()))},
        "ILU(0)": {"cvr_precond_ilu0_info": lambda p: L.cvr_precond_ilu0_info(p, C.byref(capi.Ilu0Info())),
                   "cvr_precond_ilu0_export": lambda p: L.cvr_precond_ilu0_export(p, ptr)},
        "FSAI": {"cvr_precond_fsai_info": lambda p: L.cvr_precond_fsai_info(p, C.byref(capi.FsaiInfo())),
                 "cvr_precond_fsai_export": lambda p: L.cvr_precond_fsai_export(p, ptr, ptr, ptr, ptr)},
        "AMG": {"cvr_precond_amg_info": lambda p: L.cvr_precond_amg_info(p, C.byref(capi.AmgInfo())),
                "cvr_precond_amg_smoothed_info": lambda p: L.cvr_precond_amg_smoothed_info(p, C.byref(capi.AmgSmoothedInfo())),
                "cvr_precond_amg_export_level": lambda p: L.cvr_precond_amg_export_level(p, 0, ptr, ptr, ptr, ptr, ptr, None),
                "cvr_precond_amg_export_prolongator": lambda p: L.cvr_precond_amg_export_prolongator(p, 0, ptr, ptr, ptr)},
    }
    article = {"ILU(0)": "an", "FSAI": "an", "AMG": "an"}
    for owner, calls in typed.items():
        for name, kind in KINDS.items():
            if name == owner:
                continue
            for entry, call in calls.items():
                assert call(objs[name]._p) == capi.ERR_INVALID, (entry, name)
                if owner == "Chebyshev":
                    want = f"{entry}: the preconditioner is of kind {kind} ({name}), not a Chebyshev object"
                else:
                    want = f"{entry}: the preconditioner is of kind {kind}, not {article[owner]} {owner} object (kind {KINDS[owner]})"
                assert capi.last_error() == want, (entry, name)
    assert not buf.any()


# ---- one staging of the view for all constructors ----
def _amg_bytes(P):
    info, parts = P.amg_info(), []
    for level in range(info.levels):
        e = P.amg_export_level(level)
        parts += [a.tobytes() for a in (e.rp, e.ci, e.va, e.dinv, e.agg, e.winv) if a is not None]
    s = P.amg_smoothed_info()
    if s.smoothed:
        for level in range(info.levels - 1):
            e = P.amg_export_prolongator(level)
            parts += [e.rp.tobytes(), e.ci.tobytes(), e.va.tobytes()]
    return info.levels, parts


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_arrays_and_device_arrays_build_the_same_object(dtype):
    rp, ci, va = laplacian(dtype)
    f32 = dtype == np.float32
    d = on_device(rp, ci, va)
    dp = [t.data_ptr() for t in d]
    A = cvr_amd.CvrMatrix(N, N, rp, ci, va)
    made = []
    try:
        def pair(host, device):
            made.extend((host, device))
            return host, device

        h, g = pair(capi.Precond.block_jacobi(rp, ci, va, 4), capi.Precond.block_jacobi_from_device(N, *dp, 4, is_f32=f32))
        assert h.export().tobytes() == g.export().tobytes() and h.export().any()
        h, g = pair(capi.Precond.ilu0(rp, ci, va), capi.Precond.ilu0_from_device(N, *dp, is_f32=f32))
        assert h.ilu0_export().tobytes() == g.ilu0_export().tobytes() and h.ilu0_export().any()
        h, g = pair(capi.Precond.fsai(rp, ci, va), capi.Precond.fsai_from_device(N, *dp, is_f32=f32))
        assert [a.tobytes() for a in h.fsai_export()] == [a.tobytes() for a in g.fsai_export()] and h.fsai_export()[2].any()
        h, g = pair(capi.Precond.amg(A, rp, ci, va, **AMG_OPTIONS), capi.Precond.amg_from_device(A, N, *dp, is_f32=f32, **AMG_OPTIONS))
        assert _amg_bytes(h) == _amg_bytes(g) and _amg_bytes(h)[0] == 3
        h, g = pair(capi.Precond.amg_smoothed(A, rp, ci, va, **AMG_OPTIONS), capi.Precond.amg_smoothed_from_device(A, N, *dp, is_f32=f32, **AMG_OPTIONS))
        assert _amg_bytes(h) == _amg_bytes(g) and _amg_bytes(h)[0] >= 2
    finally:
        for p in made:
            p.close()
        A.close()


def _constructors(A):
    L = capi.lib()
    return {
        "block-Jacobi": lambda p, v: L.cvr_precond_block_jacobi(C.byref(p), C.byref(v), 4, 0, None),
        "ILU(0)": lambda p, v: L.cvr_precond_ilu0(C.byref(p), C.byref(v), 0, None),
        "FSAI": lambda p, v: L.cvr_precond_fsai(C.byref(p), C.byref(v), 0, None),
        "AMG": lambda p, v: L.cvr_precond_amg(C.byref(p), A._h, C.byref(v), None, None),
        "smoothed AMG": lambda p, v: L.cvr_precond_amg_smoothed(C.byref(p), A._h, C.byref(v), None, 0.0, None),
    }


def _declined(make, view):
    p = C.c_void_p()
    rc = make(p, view)
    assert not p.value
    return rc, capi.last_error()


def test_the_shared_checks_of_the_view_in_both_forms(system):
    A, _ = system
    rp, ci, va = laplacian()
    far = ci.copy()
    far[3] = N                     # a column >= ncols
    down = rp.copy()
    down[5] = rp[4] - 1            # row_ptr decreases at row 4
    d_rp, d_ci, d_va, d_far, d_down = on_device(rp, ci, va, far, down)
    host = lambda r, c: capi.CsrView(N, N, None if r is None else r.ctypes.data, c.ctypes.data, va.ctypes.data, 0, 0)          # noqa: E731
    device = lambda r, c: capi.CsrView(N, N, None if r is None else r.data_ptr(), c.data_ptr(), d_va.data_ptr(), 0, 1)          # noqa: E731
    for name, make in _constructors(A).items():
        assert _declined(make, host(None, ci)) == (capi.ERR_INVALID, "row_ptr is null"), name
        assert _declined(make, device(None, d_ci)) == (capi.ERR_INVALID, "row_ptr is null"), name
        assert _declined(make, host(rp, far)) == (capi.ERR_INVALID, "col_idx[3] = 12 outside [0, 12)"), name
        assert _declined(make, device(d_rp, d_far)) == (capi.ERR_INVALID, "col_idx holds 0 .. 12, outside [0, 12)"), name
        assert _declined(make, host(down, ci)) == (capi.ERR_INVALID, "row_ptr decreases at row 4"), name
        assert _declined(make, device(d_down, d_ci)) == (capi.ERR_INVALID, "row_ptr decreases at row 4"), name


# ---- a failed build's message outlives the teardown ----
def test_a_failed_build_returns_its_own_message(system):
    A, _ = system
    rp, ci, va = laplacian()
    make = _constructors(A)
    diag = np.flatnonzero(ci == np.repeat(np.arange(N), np.diff(rp)))
    indefinite = va.copy()
    indefinite[diag[5]] = -2.0          # FSAI: rows 5 and 6 break down, the lowest is named; AMG: the diagonal of row 5 is not > 0
    zero_pivot = va.copy()
    zero_pivot[diag[1]] = 0.5           # ILU(0): u_11 = 0.5 - (-1 / 2) * (-1) = 0
    for v, form in ((indefinite, "host"), (indefinite, "device"), (zero_pivot, "host"), (zero_pivot, "device")):
        if form == "host":
            keep = (rp, ci, v)
            view = capi.CsrView(N, N, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, 0, 0)
        else:
            keep = on_device(rp, ci, v)
            view = capi.CsrView(N, N, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), 0, 1)
        if v is indefinite:
            assert _declined(make["FSAI"], view) == (capi.ERR_STATE, "cvr_precond_fsai: the pivot of row 5 is not finite or not > 0"), form
            assert _declined(make["AMG"], view) == (capi.ERR_STATE, "cvr_precond_amg: level 0: the diagonal entry of row 5 is not finite or not > 0"), form
            assert _declined(make["smoothed AMG"], view) == (capi.ERR_STATE, "cvr_precond_amg_smoothed: level 0: the diagonal entry of row 5 is not finite or not > 0"), form
        else:
            assert _declined(make["ILU(0)"], view) == (capi.ERR_STATE, "cvr_precond_ilu0: the pivot of row 1 is zero or not finite"), form
        del keep
