"""GPU: Clean-KID on the device (`csrc/kid.hip`, `mv_ldm_amd.cleanfid.kernel_distance`) against the fp64 restatement of tests/kid_ref.py.

Bounds (derived in kid_ref, valid for any summation order): |t_s - ref_s| <= 2 gamma scale_s for a subset's value and
|kid - ref| <= 2 gamma mean(scale_s) / m for the score, gamma = (3 (d + 3) + m^2 + S) 2^-53."""
import json

import numpy as np
import pytest
import torch

import cleanfid_ref as R
import kid_ref as K
from conftest import record_err

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
GATHER = K.CASES[1]


def _run(f1, f2, idx1, idx2, ws=None, per=True):
    """the raw `ops.kid_compute` on host arrays -> (score [1] fp32, per_subset [S], info [4]) on the host"""
    from mv_ldm_amd import ops
    dev = lambda a: a if isinstance(a, torch.Tensor) else torch.tensor(a).cuda()
    out = torch.full((1,), SENTINEL, device="cuda")
    info = torch.full((ops.KID_INFO,), SENTINEL, dtype=torch.float64, device="cuda")
    ps = torch.full((idx1.shape[0],), SENTINEL, dtype=torch.float64, device="cuda") if per else None
    ops.kid_compute(dev(f1), dev(f2), dev(idx1), dev(idx2), out, info, ps, ws)
    return out.cpu(), (ps.cpu().numpy() if per else None), info.cpu().numpy()


def _check(tag, got_kid, got_per, c, want_kid=None, want_per=None, scale=None):
    want_kid = c["kid"] if want_kid is None else want_kid
    want_per = c["per"] if want_per is None else want_per
    scale = c["scale"] if scale is None else scale
    m, g = c["m"], c["gamma"]
    e_per = float((np.abs(got_per - want_per) / scale).max())
    e_kid = abs(got_kid - want_kid) / (scale.mean() / m)
    record_err(f"kid/{tag}/per_subset_over_gamma", e_per / g)
    record_err(f"kid/{tag}/kid_over_gamma", e_kid / g)
    print(f"kid {tag}: per-subset err {e_per:.3e}, score err {e_kid:.3e}, bound {2 * g:.3e} (kid {want_kid:.6e})")
    assert e_per <= 2 * g, (tag, e_per, 2 * g)
    assert e_kid <= 2 * g, (tag, e_kid, 2 * g)


@pytest.mark.parametrize("n1,n2,d,cap,S", K.CASES, ids=str)
def test_score_and_subsets_are_the_restatement(n1, n2, d, cap, S):
    from mv_ldm_amd import ops
    c = K.case(n1, n2, d, cap, S)
    m = c["m"]
    need = ops.kid_workspace_bytes(m, S)
    wbuf = torch.full((need // 8 + 128,), SENTINEL, dtype=torch.float64, device="cuda")
    out, per, info = _run(c["f1"], c["f2"], c["idx1"], c["idx2"], ws=wbuf[64:64 + need // 8])
    assert bool((wbuf[:64] == SENTINEL).all()) and bool((wbuf[64 + need // 8:] == SENTINEL).all())      # the workspace is all it writes
    _check(f"{d}x{m}", float(info[0]), per, c)
    assert float(out) == float(np.float32(info[0])) and info[2] == m and info[3] == 0
    assert abs(info[1] - c["scale"].mean() / m) <= 2 * c["gamma"] * c["scale"].mean() / m
    # without per_subset the values stay in the workspace; the module-level call draws nothing when the subsets are given
    out2, _, info2 = _run(c["f1"], c["f2"], c["idx1"], c["idx2"], per=False)
    assert torch.equal(out, out2) and np.array_equal(info, info2)
    from mv_ldm_amd.cleanfid import kernel_distance
    got = kernel_distance(torch.tensor(c["f1"]).cuda(), torch.tensor(c["f2"]).cuda(), subsets=(c["idx1"], c["idx2"]))
    assert got.shape == () and got.dtype == torch.float32 and got.is_cuda and torch.equal(got.cpu().view(1), out)


def test_constant_features_cancel():
    n1, n2, d, cap, S = GATHER
    c = K.case(*GATHER)
    m = c["m"]
    f1, f2 = np.full((n1, d), 0.75), np.full((n2, d), 0.75)
    _, _, scale = K.kernel_distance(f1, f2, c["idx1"], c["idx2"])
    out, per, info = _run(f1, f2, c["idx1"], c["idx2"])
    assert bool((np.abs(per) <= 2 * c["gamma"] * scale).all())
    assert abs(info[0]) <= 2 * c["gamma"] * scale.mean() / m and np.isfinite(float(out))


def test_same_bits_every_call_and_any_order_within_a_subset():
    c = K.case(*K.CASES[3])
    a = _run(c["f1"], c["f2"], c["idx1"], c["idx2"])
    b = _run(c["f1"], c["f2"], c["idx1"], c["idx2"])
    assert torch.equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    rng = np.random.RandomState(3)
    idx1, idx2 = c["idx1"].copy(), c["idx2"].copy()
    idx1[1] = idx1[1][rng.permutation(c["m"])]
    idx2[1] = idx2[1][rng.permutation(c["m"])]
    _, per, _ = _run(c["f1"], c["f2"], idx1, idx2)
    assert bool((np.abs(per - a[1]) <= 2 * c["gamma"] * c["scale"]).all())
    assert np.array_equal(np.delete(per, 1), np.delete(a[1], 1))                   # the other subsets: the same bits


def test_gather_against_permuted_rows():
    n1, n2, d, cap, S = GATHER
    c = K.case(*GATHER)
    rng = np.random.RandomState(4)
    p1, p2 = rng.permutation(n1), rng.permutation(n2)                              # new row p[i] holds old row i
    f1, f2 = np.empty_like(c["f1"]), np.empty_like(c["f2"])
    f1[p1], f2[p2] = c["f1"], c["f2"]
    base = _run(c["f1"], c["f2"], c["idx1"], c["idx2"])
    out, per, info = _run(f1, f2, p1[c["idx1"]].astype(np.int32), p2[c["idx2"]].astype(np.int32))
    assert bool((np.abs(per - base[1]) <= 2 * c["gamma"] * c["scale"]).all())
    assert abs(info[0] - base[2][0]) <= 2 * c["gamma"] * c["scale"].mean() / c["m"]
    _check("permuted", float(info[0]), per, c)


def test_an_index_out_of_range_is_confined():
    """the raw path, which the host check of `kernel_distance` does not guard: the subset is NaN, counted, and the others stand.  The
    features are the first rows of allocations that hold 8 rows more, so the row the bad index names exists."""
    from mv_ldm_amd.cleanfid import kernel_distance
    n1, n2, d, cap, S = GATHER
    c = K.case(*GATHER)
    big1 = torch.zeros(n1 + 8, d, dtype=torch.float64, device="cuda")
    big2 = torch.zeros(n2 + 8, d, dtype=torch.float64, device="cuda")
    big1[:n1].copy_(torch.tensor(c["f1"]))
    big2[:n2].copy_(torch.tensor(c["f2"]))
    idx1 = c["idx1"].copy()
    idx1[2, 17] = n1
    out, per, info = _run(big1[:n1], big2[:n2], idx1, c["idx2"])
    assert np.isnan(per[2]) and info[3] == 1 and bool(torch.isnan(out).all()) and np.isnan(info[0])
    keep = np.arange(S) != 2
    assert bool((np.abs(per[keep] - c["per"][keep]) <= 2 * c["gamma"] * c["scale"][keep]).all())
    idx1[2, 17] = -1
    _, per, info = _run(big1[:n1], big2[:n2], idx1, c["idx2"])
    assert np.isnan(per[2]) and info[3] == 1 and not np.isnan(per[keep]).any()
    with pytest.raises(IndexError, match="idx1"):
        kernel_distance(big1[:n1], big2[:n2], subsets=(idx1, c["idx2"]))


@pytest.fixture(scope="module")
def model():
    from mv_ldm_amd.cleanfid import InceptionPool3
    return InceptionPool3(weights=R.make_weights()).cuda()


def test_metric_keeps_features_and_scores_them(model):
    from mv_ldm_amd import ops
    from mv_ldm_amd.cleanfid import CleanFID, kid_subsets
    real, fake = R.case_sets("other", 3, 3, 64, 48)
    metric, plain = CleanFID(model, keep_features=True), CleanFID(model)
    for mt in (metric, plain):
        mt.update(real[:2].cuda(), real=True)
        mt.update(real[2:].cuda(), real=True)
        mt.update(fake.cuda(), real=False)
    assert torch.equal(metric.compute(), plain.compute()) and torch.equal(metric.info, plain.info)      # the flag changes no FID bit
    fr, ff = metric.features(True), metric.features(False)
    assert fr.shape == ff.shape == (3, 2048) and fr.dtype == torch.float64 and fr.is_cuda
    assert torch.equal(fr, torch.cat([model.features(real[:2].cuda()), model.features(real[2:].cuda())])) and float(fr.min()) >= 0      # call by call
    info = torch.empty(ops.KID_INFO, dtype=torch.float64, device="cuda")
    per = torch.empty(4, dtype=torch.float64, device="cuda")
    got = metric.compute_kid(num_subsets=4, seed=1, info=info, per_subset=per)
    idx1, idx2 = kid_subsets(3, 3, 4, 1000, seed=1)
    kid, want_per, scale = K.kernel_distance(ff.cpu().numpy(), fr.cpu().numpy(), idx1.numpy(), idx2.numpy())      # fake = feats1, real = feats2
    c = dict(m=3, gamma=K.gamma(2048, 3, 4))
    _check("metric", float(info[0]), per.cpu().numpy(), c, kid, want_per, scale)
    assert float(got) == float(np.float32(float(info[0]))) and got.shape == () and int(info[2]) == 3
    metric.reset()
    assert metric.features(True).shape == (0, 2048) and metric.features(False).shape == (0, 2048) and metric._n == {True: 0, False: 0}
    with pytest.raises(RuntimeError, match="keep_features"):
        plain.compute_kid()
    with pytest.raises(RuntimeError, match="keep_features"):
        plain.features(True)
    with pytest.raises(ValueError, match="two images a side"):
        metric.compute_kid()                                                       # nothing kept after the reset


def test_folders_and_the_command_line(model, tmp_path, capsys):
    from mv_ldm_amd import cleanfid
    from mv_ldm_amd.image_io import save_image
    for i, img in enumerate(R.make_images(3, 32, 24, seed=41)):
        save_image(img, tmp_path / "one" / f"{i:03d}.png")
    for i, img in enumerate(R.make_images(4, 32, 24, seed=42)):
        save_image(img, tmp_path / "two" / f"{i:03d}.png")
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    want = cleanfid.compute_kid(one, two, model, num_subsets=5, seed=1)
    assert np.isfinite(want) and want == cleanfid.compute_kid(one, two, model, num_subsets=5, seed=1)
    torch.save(R.with_other_layers(R.make_weights()), tmp_path / "inception.pth")
    args = [one, two, "--weights", str(tmp_path / "inception.pth")]
    assert cleanfid.main(args + ["--json", str(tmp_path / "plain.json")]) == 0
    plain_line = capsys.readouterr().out
    plain = json.loads((tmp_path / "plain.json").read_text())
    assert sorted(plain) == ["fidclean", "n1", "n2", "solve"] and "kidclean" not in plain_line
    assert cleanfid.main(args + ["--kid", "--kid-seed", "1", "--kid-subsets", "5", "--json", str(tmp_path / "kid.json")]) == 0
    line = capsys.readouterr().out
    rec = json.loads((tmp_path / "kid.json").read_text())
    assert sorted(rec) == ["fidclean", "kid", "kidclean", "n1", "n2", "solve"]
    assert rec["kidclean"] == want and rec["fidclean"] == plain["fidclean"] and rec["solve"] == plain["solve"]
    assert sorted(rec["kid"]) == ["fp64", "m", "scale", "seed", "subsets"]
    assert rec["kid"]["m"] == 3 and rec["kid"]["subsets"] == 5 and rec["kid"]["seed"] == 1 and float(np.float32(rec["kid"]["fp64"])) == want
    assert "kidclean" in line and line.startswith(plain_line.rstrip("\n"))


def test_a_captured_call_replays_to_the_eager_bits():
    from mv_ldm_amd import ops
    c = K.case(*K.CASES[3])
    S, m = c["idx1"].shape
    f1, f2 = torch.tensor(c["f1"]).cuda(), torch.tensor(c["f2"]).cuda()
    idx1, idx2 = torch.tensor(c["idx1"]).cuda(), torch.tensor(c["idx2"]).cuda()
    eager = _run(f1, f2, idx1, idx2)
    ws = torch.empty(ops.kid_workspace_bytes(m, S), dtype=torch.uint8, device="cuda")
    out = torch.zeros(1, device="cuda")
    info = torch.zeros(ops.KID_INFO, dtype=torch.float64, device="cuda")
    per = torch.zeros(S, dtype=torch.float64, device="cuda")
    buf1 = torch.rand(f1.shape, dtype=torch.float64, device="cuda")                # captured on other contents
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.kid_compute(buf1, f2, idx1, idx2, out, info, per, ws)                  # warm-up: the library is loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                  # one stream: a single-branch graph
        ops.kid_compute(buf1, f2, idx1, idx2, out, info, per, ws)
    buf1.copy_(f1)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), eager[0]) and np.array_equal(per.cpu().numpy(), eager[1]) and np.array_equal(info.cpu().numpy(), eager[2])
