"""The four metric networks share their code (mv_ldm_amd/_metric_nets.py); what a file on disk and a seeded init see of them is pinned
against fixtures recorded before the sharing (tests/golden/make_metric_nets_golden.py names the commit).  No GPU."""
import json
import re
import sys
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
PACKAGE = Path(__file__).resolve().parent.parent / "mv_ldm_amd"
sys.path.insert(0, str(GOLDEN))
import make_metric_nets_golden as G  # noqa: E402

NAMES = ("LPIPS", "DISTS", "FrechetInceptionDistance", "InceptionPool3")


@pytest.fixture(scope="module")
def modules():
    return G.modules()


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_keys_and_shapes_in_order(modules, name):
    want = json.loads((GOLDEN / "metric_state_keys.json").read_text())
    assert sorted(want["modules"]) == sorted(NAMES) and len(want["commit"]) == 40
    assert G.keys_and_shapes(modules[name]) == want["modules"][name]


@pytest.mark.parametrize("name", NAMES)
def test_reset_parameters_draws_in_the_recorded_order(modules, name):
    want = json.loads((GOLDEN / "metric_reset_sha256.json").read_text())
    assert want["seed"] == G.SEED == 7 and sorted(want["modules"]) == sorted(NAMES)
    assert G.reset_sha256(modules[name], 7) == want["modules"][name]


def test_fid_takes_its_three_layers_from_the_one_table():
    from mv_ldm_amd import cleanfid, fid
    assert len(fid.LAYERS) == 3 and len(cleanfid.LAYERS) == 94
    assert all(a is b for a, b in zip(fid.LAYERS, cleanfid.LAYERS[:3]))
    assert fid.FrechetInceptionDistance.LAYERS is fid.LAYERS and cleanfid.InceptionPool3.LAYERS is cleanfid.LAYERS


def test_the_slice_table_is_one_object_under_its_old_names():
    from mv_ldm_amd import dists, lpips
    assert lpips.VGG_SLICES is dists.VGG_STAGES and lpips.VGG_WIDTH is dists.VGG_WIDTH


def test_no_metric_module_imports_a_private_name_from_a_sibling():
    private = re.compile(r"from \.\w+ import .*\b_[A-Za-z]")
    for name in ("lpips.py", "dists.py", "fid.py", "cleanfid.py", "_metric_nets.py"):
        hits = [line for line in (PACKAGE / name).read_text().splitlines() if private.search(line)]
        assert not hits, (name, hits)


def test_relu_keeps_its_old_name():
    from mv_ldm_amd import ops
    assert ops.lpips_relu is ops.relu_
