"""The plug-and-play head's commonsense penalty and filter (run modes train_cs / eval_cs): the launchers are declared, the call forms
refuse CPU tensors and wrong arguments, and the golden cases have the properties the GPU tests rely on (recomputed in float64 from
tests/head_cs_cases.py, without the reference)."""
import os
import re

import numpy as np
import pytest
import torch

from scene_graph_commonsense_amd.commonsense import TripletBitmaps
from scene_graph_commonsense_amd.model import BayesianHead
from tests.golden_cases import GOLDEN
from tests.head_cs_cases import C, GAP_TOL, LAMBDA_STRONG, LAMBDA_WEAK, R, cs_case, flags, penalty64, top2_gaps
from tests.head_train_cases import CASES, SPLIT, TEMPS

PARAMS = ("fc3_1.weight", "fc3_1.bias", "fc3_2.weight", "fc3_2.bias", "fc3_3.weight", "fc3_3.bias", "fc5.weight", "fc5.bias")


def test_commonsense_entry_points_are_declared():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgc_relhead.h")).read()
    names = set(re.findall(r"\bint\s+(sgc_\w+)\s*\(", hdr))
    assert {"sgc_bayes_head_any_loss_cs", "sgc_bayes_head_any_loss_cs_bwd", "sgc_bayes_head_any_candidates_cs"} <= names


def _cpu_inputs(M=2, D=32):
    head = BayesianHead(input_dim=D)
    bm = TripletBitmaps([(1, 2, 3)], [(4, 5, 6)], C, R, "cpu")
    cat = torch.zeros(M, dtype=torch.int64)
    return head, torch.zeros(M, D), torch.zeros(M, dtype=torch.int64), bm, cat


def test_the_three_call_forms_are_gpu_only():
    head, h, tgt, bm, cat = _cpu_inputs()
    with pytest.raises(RuntimeError, match="GPU"):
        head.hierarchical_nll(h, tgt, commonsense=bm, subject_cat=cat, object_cat=cat)
    with pytest.raises(RuntimeError, match="GPU"):
        head.commonsense_penalty(h, cat, cat, bm)
    with pytest.raises(RuntimeError, match="GPU"):
        head.candidates(h, commonsense=bm, subject_cat=cat, object_cat=cat.int())


def _forms(head, h, tgt):
    return (lambda **kw: head.hierarchical_nll(h, tgt, **kw),
            lambda commonsense=None, subject_cat=None, object_cat=None: head.commonsense_penalty(h, subject_cat, object_cat, commonsense),
            lambda **kw: head.candidates(h, **kw))


def test_wrong_commonsense_arguments_are_value_errors():
    head, h, tgt, bm, cat = _cpu_inputs()
    other_r = TripletBitmaps([], [], C, R + 1, "cpu")
    for call in _forms(head, h, tgt):
        with pytest.raises(ValueError):                           # the bitmaps' R is not the head's
            call(commonsense=other_r, subject_cat=cat, object_cat=cat)
        with pytest.raises(ValueError):                           # no TripletBitmaps
            call(commonsense={(1, 2, 3): 1}, subject_cat=cat, object_cat=cat)
        for kw in (dict(), dict(subject_cat=cat), dict(object_cat=cat)):
            with pytest.raises(ValueError):                       # commonsense without both category tensors
                call(commonsense=bm, **kw)
        for bad in (cat.float(), cat.to(torch.int16), cat[:1], cat[:, None], cat.tolist(), np.zeros(2, dtype=np.int64)):
            with pytest.raises(ValueError):                       # not [M] int64 / int32 tensors
                call(commonsense=bm, subject_cat=bad, object_cat=cat)
            with pytest.raises(ValueError):
                call(commonsense=bm, subject_cat=cat, object_cat=bad)


def test_from_masks_packs_the_layout_of_the_key_lists():
    g = torch.Generator().manual_seed(0)
    al, vi = torch.rand(7, 5, 7, generator=g) < 0.6, torch.rand(7, 5, 7, generator=g) < 0.1
    a = TripletBitmaps.from_masks(al, vi, "cpu")
    b = TripletBitmaps([tuple(k) for k in torch.nonzero(al).tolist()], [tuple(k) for k in torch.nonzero(vi).tolist()], 7, 5, "cpu")
    assert (a.C, a.R) == (7, 5) and torch.equal(a.aligned, b.aligned) and torch.equal(a.violated, b.violated)
    with pytest.raises(ValueError):
        TripletBitmaps.from_masks(al, vi[:, :4], "cpu")


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_cases_have_the_properties_the_gpu_tests_rely_on(name):
    gold = dict(np.load(os.path.join(GOLDEN, "head_cs.npz")))
    D, M, _ = CASES[name]
    h, sd, _, _, sc, oc, aligned, violated = cs_case(name)
    params = [sd[n] for n in PARAMS]
    pred, gap, big = top2_gaps(h, params)
    assert pred.shape == gap.shape == (M, 3)
    assert float(gap.min()) > GAP_TOL * big                      # every arg-max is decided well above the head's f32 error
    weak, strong = flags(pred, sc, oc, aligned, violated)
    n_w, n_s = int(weak.sum()), int(strong.sum())
    assert n_w >= 5 and n_s >= 5 and int((weak & strong).sum()) >= 1
    out_of_range = (sc < 0) | (sc >= C) | (oc < 0) | (oc >= C)
    assert int(out_of_range.sum()) >= 1
    assert bool(weak[out_of_range].all()) and not bool(strong[out_of_range].any())       # in neither set
    assert gold[name + "__counts"].tolist() == [n_w, n_s]
    # the reference's numbers agree with the float64 restatement (f32 against f64: 1e-5 of the value is generous for 3M <= 192 terms)
    pen, dh, dps = penalty64(h, params, pred, weak, strong, LAMBDA_WEAK, LAMBDA_STRONG, TEMPS)
    assert abs(float(pen) - float(gold[name + "__penalty"][0])) <= 1e-5 * abs(float(pen))
    assert abs(float(dh.norm()) - float(gold[name + "__dh__l2"][0])) <= 1e-5 * float(dh.norm())
    assert np.array_equal(gold[name + "__ev_relation_pred"], pred.T.reshape(-1).numpy())
    assert np.array_equal(np.isneginf(gold[name + "__ev_confidence"]), (weak | strong).T.reshape(-1).numpy())
    assert not bool(dps[6].any()) and not bool(dps[7].any())     # the penalty does not reach fc5
    assert SPLIT == (15, 11, 24)
