"""CPU tests of the commonsense candidate mining (run_mode prepare_cs): the host yardstick against the real reference's outputs
(``golden/mined_candidates.npz``, written by ``golden/make_mining_golden.py``), the step-2 triplet bookkeeping, the name tables."""
import os

import numpy as np
import pytest
import torch

from tests import mining_cases as MC


@pytest.fixture(scope="module")
def fx():
    return MC.load_fixture()


@pytest.mark.parametrize("top_k", [10, 30])
def test_host_loop_reproduces_the_reference(fx, top_k):
    """Pins ``mining_cases.related_top_k_host`` - the yardstick of the GPU property test - to what the reference's own
    ``get_related_top_k_predictions_parallel`` returned and saved on the fixture's evaluator state."""
    st = MC.fixture_state(fx)
    names = (fx["object_names"].tolist(), fx["relation_names"].tolist())
    ref_preds, ref_graphs, ref_saved = MC.fixture_lists(fx, top_k)
    stats = {}
    picks = MC.related_top_k_host(st, top_k, names, stats)
    preds, graphs = MC.lists_from_picks(st, picks, names)
    assert preds == ref_preds
    assert len(graphs) == len(ref_graphs) and all(MC.edges_equal(a, b) for a, b in zip(graphs, ref_graphs))
    assert MC.related_top_k_host(st, top_k) == picks                 # unique names: the id triple is the same key as the string
    assert stats["duplicates"] > 0
    saved = {}
    for row, (p, g) in enumerate(zip(preds, graphs)):
        if g:
            resp = MC.crc_judge(p)
            stem = "image_%d_pseudo_annotations.pkl" % row
            saved[os.path.join("cs_aligned_top%d_gpt3p5_temp" % top_k, stem)] = [e for e, r in zip(g, resp) if r == 1]
            saved[os.path.join("cs_violated_top%d_gpt3p5_temp" % top_k, stem)] = [e for e, r in zip(g, resp) if r != 1]
    assert sorted(saved) == sorted(ref_saved)
    assert all(MC.edges_equal(saved[k], ref_saved[k]) for k in saved)


def test_fixture_reaches_the_cut_and_stays_below_it(fx):
    counts = np.concatenate([fx["k10_count"], fx["k30_count"]])
    assert counts.max() >= 10 and counts.min() < 10 and counts.max() <= 11
    for image in np.unique(fx["ref_which"]):                          # no ties inside any top-30 window
        c = np.sort(fx["ref_conf"][fx["ref_which"] == image])[::-1][:31]
        assert np.isfinite(c).all() and (np.diff(c) < 0).all()


def test_name_tables_hold_unique_names(fx):
    """The reference de-duplicates an image's edges on the printed string; the kernel does it on the id triple.  The two agree
    because no two classes and no two predicates share a name."""
    assert len(fx["object_names"]) == 150 and len(set(fx["object_names"].tolist())) == 150
    assert len(fx["relation_names"]) == 50 and len(set(fx["relation_names"].tolist())) == 50
    pg = np.load(os.path.join(MC.GOLDEN, "predicted_graph.npz"))
    assert pg["object_names"].tolist() == fx["object_names"].tolist() and pg["relation_names"].tolist() == fx["relation_names"].tolist()


def test_triplet_sets_match_the_reference_dictionaries(fx, tmp_path):
    from scene_graph_commonsense_amd.commonsense import TripletSets
    _, _, saved = MC.fixture_lists(fx, 10)
    ts = TripletSets()
    for b, n in enumerate(fx["num_objects"].tolist()):
        stem = "image_%d_pseudo_annotations.pkl" % b
        yes = saved.get(os.path.join("cs_aligned_top10_gpt3p5_temp", stem))
        no = saved.get(os.path.join("cs_violated_top10_gpt3p5_temp", stem))
        if yes is None or no is None:
            continue
        rel, dr = torch.from_numpy(fx["tri_rel_%d" % b]), torch.from_numpy(fx["tri_dir_%d" % b])
        rows = [slice(g * (g - 1) // 2, g * (g + 1) // 2) for g in range(1, n)]
        ts.add_image(torch.from_numpy(fx["cats_%d" % b]), [rel[r] for r in rows], [dr[r] for r in rows], torch.from_numpy(fx["bbox_%d" % b]), yes, no)
    table = lambda a: {(int(s), int(r), int(o)): int(c) for s, r, o, c in a}
    assert ts.triplets_train_gt == table(fx["trip_gt"])
    ts.finalize().finalize()                                          # the merge happens once
    assert ts.commonsense_aligned_triplets == table(fx["trip_aligned"])
    assert ts.commonsense_violated_triplets == table(fx["trip_violated"])
    pa, pv = ts.save(str(tmp_path), "gpt3.5")
    assert os.path.basename(pa) == "commonsense_aligned_triplets_gpt3p5_temp.pt" and os.path.basename(pv) == "commonsense_violated_triplets_gpt3p5_temp.pt"
    assert torch.load(pa) == ts.commonsense_aligned_triplets and torch.load(pv) == ts.commonsense_violated_triplets
    assert all(isinstance(k, tuple) and all(type(x) is int for x in k) for k in torch.load(pa))
    with pytest.raises(RuntimeError):
        ts.add_image(torch.zeros(2), [], [], torch.zeros(2, 4), [], [])


def test_triplet_sets_skip_unmatched_and_self_edges():
    from scene_graph_commonsense_amd.commonsense import TripletSets
    cats = torch.tensor([7, 8, 9])
    bbox = torch.tensor([[0, 4, 0, 4], [0, 4, 0, 4], [5, 9, 5, 9]])          # objects 0 and 1 share a box: the first one matches
    ts = TripletSets()
    ts.add_image(cats, [torch.tensor([3]), torch.tensor([-1, 5])], [torch.tensor([1.0]), torch.tensor([-1.0, 0.0])], bbox,
                 [[[0, 4, 0, 4], 2, [5, 9, 5, 9], -1.0, 0], [[0, 4, 0, 4], 2, [0, 4, 0, 4], -1.0, 1], [[1, 2, 3, 4], 2, [5, 9, 5, 9], -1.0, 2]],
                 [[[5, 9, 5, 9], 6, [0, 4, 0, 4], -2.0, 3], [[0, 4, 0, 4], 3, [5, 9, 5, 9], -2.0, 4], [[9, 9, 9, 9], 1, [8, 8, 8, 8], -2.0, 5]])
    assert ts.triplets_train_gt == {(8, 3, 7): 1, (8, 5, 9): 1}
    assert ts.commonsense_aligned_triplets == {(7, 2, 9): 1}
    assert ts.commonsense_violated_triplets == {(9, 6, 7): 1, (7, 3, 9): 1}
