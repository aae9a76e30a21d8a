"""CPU: the host half of the SGDET / SGCLS device metrics - ``pairs.sg_target_table`` against the oracle's literal
``match_target_sgd`` loop, and the properties of the synthetic fixtures the GPU kernel test runs on."""
import os

import numpy as np
import pytest
import torch

from oracle import relhead_oracle as ro
from tests import sg_metrics_cases as SG
from tests import sgdet_case
from tests.golden_cases import GOLDEN


def _stored_case():
    cfg, _, batch, _, _ = sgdet_case.make_case()
    sgdet_case.apply_stored_targets(batch, np.load(os.path.join(GOLDEN, "sgdet_vg.npz")))
    return batch


def _ragged_case():
    from scene_graph_commonsense_amd.synthetic import HeadConfig, make_scene_batch
    return make_scene_batch(HeadConfig(), (5, 2, 4, 1, 3), seed=23, connect_frac=0.6)


def _relations(batch):
    """(all relations of the input, those whose graph object is the image's last object)."""
    total = last = 0
    for b, dirs in enumerate(batch.subj_or_obj):
        for g, flag in enumerate(dirs, start=1):
            n = int(((np.asarray(flag)[:g] == 1) | (np.asarray(flag)[:g] == 0)).sum())
            total += n
            last += n if g == len(dirs) else 0
    return total, last


@pytest.mark.parametrize("case", ["stored_sgdet", "ragged"])
def test_sg_target_table_matches_the_oracle_lists(case):
    from scene_graph_commonsense_amd.pairs import sg_target_table
    batch = _stored_case() if case == "stored_sgdet" else _ragged_case()
    args = (batch.relationships, batch.subj_or_obj, batch.categories, batch.bbox)
    image, rel, scat, ocat, sbox, obox = sg_target_table(*args)
    assert (image.dtype, rel.dtype, scat.dtype, ocat.dtype, sbox.dtype, obox.dtype) == (np.int32, np.int64, np.int64, np.int64,
                                                                                      np.float32, np.float32)
    cs, co, bs, bo, rt = ro.match_target_sgd(*args)
    have = [b for b in range(len(rt)) if rt[b] is not None]
    cat = lambda lst: np.concatenate([np.asarray(lst[b]).reshape(len(rt[b]), -1) for b in have]) if have else np.zeros((0, 1))
    np.testing.assert_array_equal(image, np.concatenate([np.full(len(rt[b]), b) for b in have]))
    np.testing.assert_array_equal(rel, cat(rt).reshape(-1))
    np.testing.assert_array_equal(scat, cat(cs).reshape(-1))
    np.testing.assert_array_equal(ocat, cat(co).reshape(-1))
    np.testing.assert_array_equal(sbox, cat(bs).astype(np.float32))
    np.testing.assert_array_equal(obox, cat(bo).astype(np.float32))
    total, last = _relations(batch)
    assert len(rel) == total - last                          # the reference's loop bound: relations on an image's last object are dropped
    if case == "ragged":
        assert last >= 1 and total > last                    # ... and the quirk is visible in this input
        assert set(image.tolist()) < set(range(5))           # images without (collected) relations contribute no rows


def test_sg_target_table_of_nothing_is_empty():
    from scene_graph_commonsense_amd.pairs import sg_target_table
    t = sg_target_table([[], []], [[], []], [torch.tensor([3]), torch.tensor([4])], [torch.zeros(1, 4), torch.zeros(1, 4)])
    assert [a.shape for a in t] == [(0,), (0,), (0,), (0,), (0, 4), (0, 4)]


def test_fixtures_reach_every_case():
    missing = [k for k, v in SG.fixture_properties().items() if not v]
    assert not missing, missing


def test_equivalence_table_is_the_reference_predicate():
    """The [160,160] table the kernel reads says what ``compare_object_cat`` says, for every pair of classes."""
    from scene_graph_commonsense_amd.evaluator import _equiv_matrix
    m = _equiv_matrix()
    want = np.array([[ro.compare_object_cat(a, b) for b in range(m.shape[1])] for a in range(m.shape[0])])
    np.testing.assert_array_equal(m, want)
