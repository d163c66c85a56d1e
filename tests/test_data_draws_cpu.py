"""hcflow_amd.data under fixed seeds and the two C entries of hcf_data.hip under compound faults, against what the commit before
the single and the paired path were folded together gave (tests/golden/data_draws.json, written by make_data_draws.py on that
commit). No tolerance: every table, index order, path list and return code is reproduced exactly. No GPU needed."""
import importlib.util as ilu
import json
import os

import pytest

from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "data_draws.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def now():
    spec = ilu.spec_from_file_location("make_data_draws", os.path.join(GOLDEN, "make_data_draws.py"))
    mod = ilu.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return json.loads(json.dumps(mod.record()))          # tuples -> lists, as the stored file has them


def test_draws_and_loader_orders_are_pinned(recorded, now):
    """draw_crops and draw_paired_crops under every gate and both rules; the index order, crop tables and path lists of the
    first two batches of BankLoader and of PairedBankLoader at world 1 and 2, epoch 0 and 1: one torch.rand(B, 5) per draw, the
    permutation before the crops."""
    keys = ("draw_crops", "draw_paired_crops", "bank_loader", "paired_loader")
    assert len(recorded["draw_crops"]) == 5 and len(recorded["draw_paired_crops"]) == 8 and len(recorded["paired_loader"]) == 6
    assert all(len(v["batches"]) == 2 for v in recorded["paired_loader"].values()) and len(recorded["bank_loader"]) == 2
    for k in keys:
        names = recorded[k] if isinstance(recorded[k], dict) else range(len(recorded[k]))
        assert len(now[k]) == len(recorded[k])
        for name in names:
            assert now[k][name] == recorded[k][name], (k, name)


def test_compound_faults_return_the_pinned_codes(recorded, now):
    """Inputs that break two rules at once: which of the two codes comes out is the order of the host checks (image by image:
    dimensions and offset sign, then HCF_ERR_SHAPE, then the byte range; tables before pairs before crops; within a record:
    index, origin, flags, rot90, window)."""
    want = recorded["return_codes"]
    assert len(want) >= 12 and set(want.values()) == {0, -1, -5}
    assert set(now["return_codes"]) == set(want)
    for name, code in want.items():
        assert now["return_codes"][name] == code, name
