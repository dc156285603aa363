"""CPU: Clean-KID's host side -- the subsets are drawn in the package's order, the restatement (tests/kid_ref.py) cancels where it must,
the library exports the two new entries and refuses bad arguments before any launch, and the kid kernels use no scratch."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import kid_ref as K


def _package_draws(n1, n2, num_subsets, cap):
    """the package's loop on numpy's global stream: per subset the x side (feats2) first"""
    m = min(n1, n2, cap)
    i1, i2 = [], []
    for _ in range(num_subsets):
        i2.append(np.random.choice(n2, m, replace=False))
        i1.append(np.random.choice(n1, m, replace=False))
    return np.stack(i1), np.stack(i2)


@pytest.mark.parametrize("n1,n2,num_subsets,cap", [(9, 7, 4, 1000), (12, 20, 3, 5), (30, 30, 2, 30)])
def test_subsets_are_the_package_draws(n1, n2, num_subsets, cap):
    from mv_ldm_amd.cleanfid import kid_subsets
    np.random.seed(5)
    w1, w2 = _package_draws(n1, n2, num_subsets, cap)
    m = min(n1, n2, cap)
    for how in ("int", "state", "global"):
        if how == "global":
            np.random.seed(5)
        i1, i2 = kid_subsets(n1, n2, num_subsets, cap, seed={"int": 5, "state": np.random.RandomState(5), "global": None}[how])
        assert i1.dtype == i2.dtype == torch.int32 and tuple(i1.shape) == tuple(i2.shape) == (num_subsets, m) and not i1.is_cuda
        assert np.array_equal(i1.numpy(), w1) and np.array_equal(i2.numpy(), w2), how
        assert all(len(set(r.tolist())) == m for r in i1) and int(i1.max()) < n1 and int(i2.max()) < n2
    before = np.random.get_state()[1].copy()
    kid_subsets(n1, n2, num_subsets, cap, seed=5)                                  # a private stream leaves the global one alone
    assert np.array_equal(before, np.random.get_state()[1])


def test_too_small_a_side_raises():
    from mv_ldm_amd.cleanfid import kid_subsets
    for n1, n2, cap in ((1, 5, 1000), (5, 1, 1000), (5, 5, 1), (0, 0, 10)):
        with pytest.raises(ValueError, match="two images a side"):
            kid_subsets(n1, n2, 3, cap, seed=0)


def test_constant_features_cancel_in_the_restatement():
    n1, n2, d, cap, S = K.CASES[1]
    m = min(n1, n2, cap)
    f1, f2 = np.full((n1, d), 0.75), np.full((n2, d), 0.75)
    idx1, idx2 = K.make_subsets(n1, n2, m, S)
    kid, per, scale = K.kernel_distance(f1, f2, idx1, idx2)
    g = K.gamma(d, m, S)
    assert bool((np.abs(per) <= 2 * g * scale).all()) and abs(kid) <= 2 * g * scale.mean() / m
    assert float(scale.min()) > 1.0                                                # the bound is no triviality: each term is 4 m (1.5625)^3


def test_restatement_matches_the_formula_written_out():
    """the estimator as the package writes it, on the smallest case"""
    c = K.case(*K.CASES[0])
    d, m, t = 64, c["m"], 0.0
    for s in range(3):
        x, y = c["f2"][c["idx2"][s]], c["f1"][c["idx1"][s]]
        a = (x @ x.T / d + 1) ** 3 + (y @ y.T / d + 1) ** 3
        b = (x @ y.T / d + 1) ** 3
        t += (a.sum() - np.diag(a).sum()) / (m - 1) - b.sum() * 2 / m
    assert m == 5 and abs(t / 3 / m - c["kid"]) <= 2 * c["gamma"] * c["scale"].mean() / m


@pytest.fixture(scope="module")
def lib():
    from mv_ldm_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_library_exports_the_kid_entries(lib):
    from mv_ldm_amd import _lib, ops
    for n in ("mvldm_kid_workspace_bytes", "mvldm_kid_compute"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.mvldm_abi_version() == _lib.ABI_VERSION == 7 and ops.KID_INFO == 4
    # one double a tile (pairs a <= b of two symmetric Grams + the cross Gram), two a subset
    for m, tiles in ((2, 3), (64, 3), (65, 10), (150, 21), (1000, 2 * 136 + 256)):
        assert lib.mvldm_kid_workspace_bytes(m, 7) == 7 * (tiles + 2) * 8 == ops.kid_workspace_bytes(m, 7)
    assert lib.mvldm_kid_workspace_bytes(1, 7) == 0 and lib.mvldm_kid_workspace_bytes(5, 0) == 0


def test_bad_arguments_are_refused_on_the_host(lib):
    """nothing here reaches a launch: every call is refused by a check that comes before"""
    ERR_ARG, ERR_UNSUPPORTED = -1, -3                                              # MVLDM_ERR_* of include/mvldm.h
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    p += -p % 16
    err = lambda: lib.mvldm_last_error()
    call = lambda f1=p, n1=10, f2=p, n2=10, d=64, i1=p, i2=p, S=2, m=5, ws=p, wsb=1 << 20, sc=p, per=None, info=p: \
        lib.mvldm_kid_compute(f1, n1, f2, n2, d, i1, i2, S, m, ws, wsb, sc, per, info, None)
    assert call(m=1) == ERR_ARG and b"two a side" in err()
    assert call(m=11) == ERR_ARG and call(n1=4) == ERR_ARG and b"out of" in err()
    assert call(S=0) == ERR_ARG and b"subsets" in err()
    assert call(wsb=lib.mvldm_kid_workspace_bytes(5, 2) - 8) == ERR_ARG and b"workspace" in err()
    for kw in (dict(f1=None), dict(f2=None), dict(i1=None), dict(i2=None), dict(ws=None), dict(sc=None), dict(info=None), dict(f1=p + 8), dict(per=p + 4)):
        assert call(**kw) == ERR_ARG and b"null or unaligned" in err(), kw
    for d in (0, 32, 96, 2112, 4096):
        assert call(d=d) == ERR_UNSUPPORTED and b"multiples of 64" in err(), d


def test_host_wrappers_refuse_before_the_device():
    from mv_ldm_amd import cleanfid
    f = torch.zeros(4, 64, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="HIP device"):
        cleanfid.kernel_distance(f, f)
    m = cleanfid.CleanFID.__new__(cleanfid.CleanFID)                                # the refusals need no state
    torch.nn.Module.__init__(m)
    m.keep_features = False
    with pytest.raises(RuntimeError, match="keep_features"):
        m.compute_kid()
    with pytest.raises(RuntimeError, match="keep_features"):
        m.features(True)


@pytest.fixture(scope="module")
def resources():
    from mv_ldm_amd import _build
    _build.build()
    if not _build.RES.exists():
        _build.build(force=True)
    return json.loads(_build.RES.read_text())


def test_kid_kernels_use_no_scratch(resources):
    kid = {k: v for k, v in resources.items() if "kid_" in k}
    for name in ("kid_tile_kernel", "kid_subset_kernel", "kid_final_kernel"):
        assert any(name in k for k in kid), name
    bad = {k: v for k, v in kid.items() if v["scratch"] or v.get("vgpr_spill", 0)}
    assert not bad, bad
