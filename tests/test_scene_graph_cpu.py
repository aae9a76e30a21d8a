"""Scene-graph inference, host side: ``SceneGraphs.to_list`` reproduces the reference's ``predicted_graph``
(``evaluator.py:482-503``) recorded in tests/golden/predicted_graph.npz (tests/golden/make_graph_golden.py), the kernel's entry point
is declared and exported, and the device functions refuse CPU tensors."""
import os
import re

import numpy as np
import pytest
import torch

from tests.golden_cases import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _graphs_from_fixture(gold):
    from scene_graph_commonsense_amd.scene_graph import SceneGraphs
    ids, raw = torch.from_numpy(gold["ids"]), torch.from_numpy(gold["raw_boxes"])
    B, K = ids.shape[:2]
    z = torch.full((B, K), -1, dtype=torch.int32)
    return SceneGraphs(pair=z, slot=z, predicate=ids[..., 1].int(), subject=z, object=z, score=torch.zeros(B, K),
                       count=torch.from_numpy(gold["count"]).int(), n_finite=torch.from_numpy(gold["count"]).int(),
                       subject_cat=ids[..., 0], object_cat=ids[..., 2], subject_box=raw[:, :, 0], object_box=raw[:, :, 1],
                       image=torch.from_numpy(gold["image"]).int(), feature_size=int(gold["feature_size"][0]))


def test_to_list_reproduces_the_reference_predicted_graph():
    gold = dict(np.load(os.path.join(GOLDEN, "predicted_graph.npz")))
    heights, widths = gold["heights"].tolist(), gold["widths"].tolist()
    assert any(h != w for h, w in zip(heights, widths))                      # the x-by-height / y-by-width quirk is visible
    names = (gold["object_names"].tolist(), gold["relation_names"].tolist())
    graphs = _graphs_from_fixture(gold)
    got = graphs.to_list(heights, widths, names=names)
    assert len(got) == len(gold["count"]) and int(gold["count"].sum()) > 0
    for b, graph in enumerate(got):
        assert len(graph) == int(gold["count"][b])
        for r, edge in enumerate(graph):
            assert list(edge) == ["edge", "subject_id", "relation_id", "object_id", "bbox_sub", "bbox_obj"]
            assert edge["edge"] == str(gold["edges"][b, r])
            assert [edge["subject_id"], edge["relation_id"], edge["object_id"]] == gold["ids"][b, r].tolist()
            assert edge["bbox_sub"] == gold["pixel_boxes"][b, r, 0].tolist()
            assert edge["bbox_obj"] == gold["pixel_boxes"][b, r, 1].tolist()
            assert all(type(v) is int for v in edge["bbox_sub"] + edge["bbox_obj"] + [edge["subject_id"], edge["relation_id"], edge["object_id"]])
    # without names: the same dicts without "edge"; the inputs are left untouched
    plain = graphs.to_list(heights, widths)
    assert [[{k: v for k, v in e.items() if k != "edge"} for e in g] for g in got] == plain
    np.testing.assert_array_equal(graphs.subject_box.numpy(), gold["raw_boxes"][:, :, 0])


def test_to_list_scales_x_by_height_and_y_by_width():
    from scene_graph_commonsense_amd.scene_graph import SceneGraphs
    z = torch.zeros(1, 2, dtype=torch.int32)
    g = SceneGraphs(pair=z, slot=z, predicate=z + 3, subject=z, object=z, score=torch.zeros(1, 2), count=torch.tensor([1], dtype=torch.int32),
                    n_finite=torch.tensor([1], dtype=torch.int32), subject_cat=torch.tensor([[7, -1]]), object_cat=torch.tensor([[9, -1]]),
                    subject_box=torch.tensor([[[1, 5, 2, 31], [-1, -1, -1, -1]]]), object_box=torch.tensor([[[0.5, 32, 0, 7.25], [-1, -1, -1, -1]]]),
                    image=torch.tensor([1], dtype=torch.int32), feature_size=32)
    (graph,) = g.to_list([100, 300], [100, 200])
    assert graph == [dict(subject_id=7, relation_id=3, object_id=9, bbox_sub=[10, 47, 13, 194], bbox_obj=[5, 300, 0, 46])]


def test_scene_graph_entry_point_is_declared_and_exported():
    from scene_graph_commonsense_amd import _lib
    hdr = open(os.path.join(REPO, "include", "sgc_relhead.h")).read()
    assert "sgc_scene_graph_topk" in set(re.findall(r"\bint\s+(sgc_\w+)\s*\(", hdr))
    assert "evaluator.py:125-134,160-194,292-316,465-503" in hdr
    assert hasattr(_lib.load(), "sgc_scene_graph_topk")


def test_ranking_is_gpu_only_and_bounds_top_k():
    from scene_graph_commonsense_amd.scene_graph import rank_scene_graphs
    conf, pred, conn, ptr = torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4), torch.tensor([0, 4], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        rank_scene_graphs(conf, pred, conn, ptr)
    with pytest.raises(ValueError, match="top_k"):
        rank_scene_graphs(conf, pred, conn, ptr, top_k=129)
