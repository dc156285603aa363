"""CPU: Clean-FID's restatement (tests/cleanfid_ref.py) against PIL's own resize (tests/golden/cleanfid_resize.npz, and live PIL where it
imports), the weight loader's refusals, the new entries of the library with their host-side refusals, and what stays refused."""
import ctypes as C
import json
import warnings

import numpy as np
import pytest
import torch

import cleanfid_ref as R
from conftest import GOLDEN


def _ulp32(v):
    """one float32 step at max(|v|, 1)"""
    return np.spacing(np.maximum(np.abs(v), 1).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("h,w,oh,ow", R.RESIZE_CASES, ids=str)
def test_restatement_resizes_like_pil(h, w, oh, ow):
    g = np.load(GOLDEN / "cleanfid_resize.npz", allow_pickle=False)
    src, want = g[f"src_{h}x{w}_{oh}x{ow}"], g[f"out_{h}x{w}_{oh}x{ow}"]
    assert np.array_equal(src, R.resize_inputs(h, w).numpy())                     # the inputs are the seeded ones
    got = R.resize_clean(src.astype(np.float32), oh, ow)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert bool((np.abs(got.astype(np.float64) - want) <= _ulp32(want)).all())
    if (h, w) == (oh, ow):
        assert np.array_equal(got, src.astype(np.float32))                        # both passes skipped
    assert float(want.max()) > 255 or float(want.min()) < 0 or (h, w) == (oh, ow) or oh < h     # the cubic overshoots where it enlarges: the clip matters
    try:
        live = R.resize_pil(src.astype(np.float32), oh, ow)
    except ImportError:
        return
    assert bool((np.abs(got.astype(np.float64) - live) <= _ulp32(live)).all())


def test_prep_clips_and_centres():
    src = R.resize_inputs(13, 17)
    x = R.prep(src, 29, 23)
    assert x.dtype == torch.float64 and tuple(x.shape) == (4, 3, 29, 23)
    assert float(x.min()) >= -1.0 and float(x.max()) <= 127 / 128 and float(x.min()) == -1.0 and float(x.max()) == 127 / 128
    flt = (src.float() / 255).contiguous()
    assert torch.equal(flt * 255, src.float())                                    # k / 255 * 255 == k in fp32 for every byte
    assert torch.equal(R.prep(flt, 29, 23), x)


def _model(**kw):
    from mv_ldm_amd.cleanfid import InceptionPool3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return InceptionPool3(**kw)


def test_loader_reads_the_package_file_and_refuses_others(tmp_path):
    sd = R.make_weights()
    m = _model(allow_random_init=True)
    assert sorted(m.state_dict()) == sorted(sd) and len(sd) == 94 * 5
    m.load_weights(R.with_other_layers(sd))
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    torch.save(R.with_other_layers(sd, "inception."), tmp_path / "w.pth")
    m2 = _model(weights=str(tmp_path / "w.pth"))
    assert all(torch.equal(v, sd[k]) for k, v in m2.state_dict().items())
    before = {k: v.clone() for k, v in m.state_dict().items()}
    for bad, exc, word in (({k: v for k, v in sd.items() if k != "Mixed_6b.branch7x7_2.conv.weight"}, KeyError, "Mixed_6b.branch7x7_2.conv.weight"),
                           ({**sd, "Mixed_8a.conv.weight": torch.zeros(1)}, KeyError, "Mixed_8a.conv.weight"),
                           ({**sd, "Mixed_6b.branch7x7_2.conv.weight": torch.zeros(128, 128, 7, 1)}, ValueError, "shape"),
                           ({**sd, "Mixed_7c.branch_pool.bn.running_var": torch.full((192,), -1e-3)}, ValueError, "not positive")):
        with pytest.raises(exc, match=word):
            m.load_weights(bad)
        assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())  # a refused file changes nothing
    with pytest.raises(TypeError):
        m.load_weights(3)
    with pytest.raises(TypeError):
        _model(dtype=torch.float64, allow_random_init=True)
    with pytest.warns(UserWarning, match="RANDOM"):
        from mv_ldm_amd.cleanfid import InceptionPool3
        InceptionPool3()
    a, b = _model(allow_random_init=True), _model(allow_random_init=True)
    a.reset_parameters(5)
    b.reset_parameters(5)
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())


def test_the_layer_table_is_inception_v3():
    from mv_ldm_amd.cleanfid import LAYERS
    assert [tuple(r) for r in LAYERS] == [tuple(r) for r in R.LAYERS] and len(LAYERS) == 94
    unfolded = [r for r in LAYERS if not (r[3][0] == r[3][1] and r[3][0] in (1, 3))]
    assert len(unfolded) == 37 and all(r[1] % 16 == 0 and r[4] == 1 and r[5] == (r[3][0] // 2, r[3][1] // 2) for r in unfolded)
    assert all(r[2] % 16 == 0 for r in LAYERS)


def test_cpu_inputs_and_other_taps_stay_refused():
    from mv_ldm_amd.cleanfid import CleanFID
    from mv_ldm_amd.fid import FrechetInceptionDistance
    m = _model(allow_random_init=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.features(torch.zeros(2, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1))
    for feature in (192, 768, 2048):
        with pytest.raises(NotImplementedError, match="feature=64"):
            FrechetInceptionDistance(feature=feature)
    metric = CleanFID.__new__(CleanFID)                                           # the refusal below needs no state: host counters only
    torch.nn.Module.__init__(metric)
    metric._n = {True: 1, False: 5}
    with pytest.raises(RuntimeError, match="More than one sample"):
        metric.compute()


def test_compute_fid_refuses_empty_and_missing_folders(tmp_path):
    from mv_ldm_amd import cleanfid
    from mv_ldm_amd.image_io import save_image
    (tmp_path / "a" / "sub").mkdir(parents=True)
    (tmp_path / "b").mkdir()
    (tmp_path / "b" / "notes.txt").write_text("no image")
    save_image(torch.rand(3, 5, 4), tmp_path / "a" / "sub" / "x.png")
    with pytest.raises(ValueError, match="no \\*.png"):
        cleanfid.compute_fid(tmp_path / "a", tmp_path / "b", R.make_weights())
    with pytest.raises(FileNotFoundError):
        cleanfid.compute_fid(tmp_path / "a", tmp_path / "nowhere", R.make_weights())
    with pytest.raises(ValueError, match="no \\*.png"):
        cleanfid.main([str(tmp_path / "b"), str(tmp_path / "a"), "--weights", str(tmp_path / "none.pth")])
    save_image(torch.rand(3, 5, 4), tmp_path / "a" / "a.png")
    save_image(torch.rand(3, 7, 4), tmp_path / "a" / "sub" / "b.png")
    assert [p.name for p in cleanfid.list_images(tmp_path / "a")] == ["a.png", "b.png", "x.png"]
    batches = list(cleanfid.iter_batches(tmp_path / "a", batch=1))
    assert [tuple(b.shape) for b in batches] == [(1, 3, 5, 4), (1, 3, 5, 4), (1, 3, 7, 4)] and batches[0].dtype == torch.uint8


# ---- the library ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mv_ldm_amd import _build, _lib
    _build.build()
    return _lib.load()


NEW = ("mvldm_inception_workspace_bytes", "mvldm_inception_prep", "mvldm_inception_unfold", "mvldm_inception_maxpool", "mvldm_inception_avgpool",
       "mvldm_inception_concat", "mvldm_inception_features", "mvldm_frechet_accumulate", "mvldm_frechet_workspace_bytes", "mvldm_frechet_compute")


def test_library_exports_the_new_entries_and_keeps_its_version(lib):
    from mv_ldm_amd import _lib
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.mvldm_abi_version() == _lib.ABI_VERSION == 7


def test_workspace_sizes_and_shape_rules(lib):
    assert lib.mvldm_frechet_workspace_bytes(2048) == (16 + 4 * 2048 + 4 * 2048 * 2048) * 8
    assert lib.mvldm_frechet_workspace_bytes(64) == (16 + 4 * 64 + 4 * 64 * 64) * 8
    for d in (0, 32, 96, 2112, 4096, -64):
        assert lib.mvldm_frechet_workspace_bytes(d) == 0
    assert lib.mvldm_inception_workspace_bytes(5, 64, 299) == 5 * 3 * 64 * 299 * 4
    assert lib.mvldm_inception_workspace_bytes(0, 64, 299) == 0 and lib.mvldm_inception_workspace_bytes(2, 0, 299) == 0
    # the existing entries keep their limits
    assert lib.mvldm_fid_pool_slots(9, 9, 576) == 0 and lib.mvldm_fid_compute(None, None, 2048, None, None, None) < 0
    assert b"64" in lib.mvldm_last_error()


def test_bad_arguments_are_refused_on_the_host(lib):
    """nothing here reaches a launch: every pointer is either null or a host buffer the checks refuse for another reason first"""
    from mv_ldm_amd import _lib as L
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    err = lambda: lib.mvldm_last_error()
    assert lib.mvldm_inception_prep(None, 1, None, 2, 8, 8, 4, 4, 4, L.F32, None, 1 << 20, None) < 0 and b"null" in err()
    assert lib.mvldm_inception_prep(p, 1, p, 2, 8, 8, 4, 4, 4, L.F32, p, 8, None) < 0 and b"workspace" in err()
    assert lib.mvldm_inception_prep(p, 1, p, 2, 8, 8, 0, 4, 4, L.F32, p, 1 << 20, None) < 0 and b"edge below 1" in err()
    assert lib.mvldm_inception_prep(p, 1, p, 2, 8, 8, 4, 4, 8, L.F32, p, 1 << 20, None) < 0 and b"c_pad" in err()
    assert lib.mvldm_inception_prep(p, 2, p, 2, 8, 8, 4, 4, 4, L.F32, p, 1 << 20, None) < 0 and b"src_u8" in err()
    assert lib.mvldm_inception_prep(p, 1, p, 2, 8, 8, 4, 4, 4, 7, p, 1 << 20, None) < 0 and b"dtype" in err()
    assert lib.mvldm_inception_prep(p, 1, p + 4, 2, 8, 8, 4, 4, 4, L.F32, p, 1 << 20, None) < 0 and b"unaligned" in err()
    assert lib.mvldm_inception_unfold(p, p, 2, 9, 11, 16, 2, 7, 1, 3, L.F32, None) < 0 and b"odd" in err()
    assert lib.mvldm_inception_unfold(p, p, 2, 9, 11, 16, 1, 9, 0, 4, L.F32, None) < 0 and b"up to 7" in err()
    assert lib.mvldm_inception_unfold(p, p, 2, 9, 11, 16, 1, 7, 0, 0, L.F32, None) < 0 and b"padding" in err()
    assert lib.mvldm_inception_unfold(p, p, 2, 9, 11, 6, 1, 7, 0, 3, L.F32, None) < 0 and b"16-byte" in err()
    assert lib.mvldm_inception_unfold(p, p, 400, 147, 147, 64, 5, 5, 2, 2, L.F32, None) < 0 and b"32-bit offset" in err()
    assert lib.mvldm_inception_unfold(None, p, 2, 9, 11, 16, 1, 7, 0, 3, L.F32, None) < 0 and b"null" in err()
    assert lib.mvldm_inception_maxpool(p, p, 2, 8, 9, 16, 3, 0, 16, 0, L.F32, None) < 0 and b"stride" in err()
    assert lib.mvldm_inception_maxpool(p, p, 2, 2, 9, 16, 2, 0, 16, 0, L.F32, None) < 0 and b"3 x 3 window" in err()
    assert lib.mvldm_inception_maxpool(p, p, 2, 8, 9, 16, 2, 0, 24, 12, L.F32, None) < 0 and b"do not fit" in err()
    assert lib.mvldm_inception_maxpool(p, p, 2, 8, 9, 16, 2, 0, 32, 6, L.F32, None) < 0 and b"do not fit" in err()
    assert lib.mvldm_inception_maxpool(p, None, 2, 8, 9, 16, 2, 0, 32, 16, L.F32, None) < 0 and b"null" in err()
    assert lib.mvldm_inception_avgpool(p, p, 2, 3, 3, 16, 8, 0, L.F16, None) < 0 and b"do not fit" in err()
    assert lib.mvldm_inception_avgpool(p, p + 8, 2, 3, 3, 16, 16, 0, L.F16, None) < 0 and b"unaligned" in err()
    assert lib.mvldm_inception_concat(p, p, 10, 16, 16, 4, 0, L.F32, None) < 0 and b"do not fit" in err()
    assert lib.mvldm_inception_concat(p, p, 10, 16, 32, 16, 2, L.F32, None) < 0 and b"relu" in err()
    assert lib.mvldm_inception_concat(p, p, 1 << 30, 16, 32, 16, 0, L.F32, None) < 0 and b"32-bit offset" in err()
    assert lib.mvldm_inception_features(None, 2, 8, 8, 2048, L.F32, p, None) < 0 and b"null" in err()
    assert lib.mvldm_inception_features(p, 2, 8, 8, 2050, L.F32, p, None) < 0 and b"16-byte" in err()
    assert lib.mvldm_frechet_accumulate(p, 3, 96, p, None) < 0 and b"multiples of 64" in err()
    assert lib.mvldm_frechet_accumulate(p, 3, 4096, p, None) < 0 and b"2048" in err()
    assert lib.mvldm_frechet_accumulate(None, 3, 128, p, None) < 0 and b"null" in err()
    assert lib.mvldm_frechet_accumulate(p, 3, 128, p + 4, None) < 0 and b"unaligned" in err()
    need = lib.mvldm_frechet_workspace_bytes(128)
    assert lib.mvldm_frechet_compute(p, p, 100, p, need, p, p, None) < 0 and b"multiples of 64" in err()
    assert lib.mvldm_frechet_compute(p, p, 128, p, need - 8, p, p, None) < 0 and b"workspace" in err()
    assert lib.mvldm_frechet_compute(p, p, 128, None, need, p, p, None) < 0 and b"null" in err()
    assert lib.mvldm_frechet_compute(p, p, 128, p, need, p + 2, p, None) < 0 and b"unaligned" in err()
    # nothing to do is no error and no launch
    assert lib.mvldm_inception_prep(None, 1, None, 0, 8, 8, 4, 4, 4, L.F32, None, 0, None) == 0
    assert lib.mvldm_frechet_accumulate(None, 0, 128, None, None) == 0


def test_emulation_of_the_solve_meets_the_symmetric_route():
    """the numpy model of the device's one-sided Jacobi at d = 128: the analytic pair to round-off, the rank-deficient pair within the
    class the recorded bounds file states, both solves converged well below the sweep cap"""
    emu = json.loads((GOLDEN / "cleanfid_cpu_emulation.json").read_text())["solve"]
    for name in ("analytic", "deficient"):
        cls, s1, s2, c = R.synthetic_cases(128)[name]
        got, info = R.hestenes_emulation(s1, s2)
        sc = R.scale(s1, s2)
        want = R.frechet_sym(s1, s2) if c is None else sc - 2 * c
        assert info[4] == 0 and info[0] < R.SWEEP_CAP // 2 and info[2] < R.SWEEP_CAP // 2
        assert abs(got - want) / sc <= 10 * emu["worst"]["128"][cls]
        assert abs(want - emu["cases"][f"{name}/128"]["want"]) <= 1e-6 * sc
