"""Host-side checks of the input-gradient feature (no GPU): the C ABI declares the two kernels' launchers, the public calls take the
switch, and the property the GPU tests rely on - the reference's own input gradient vanishes outside the union of an image's boxes -
holds for the oracle's autograd."""
import dataclasses
import inspect
import os
import re

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_input_gradient_launchers():
    hdr = open(os.path.join(REPO, "include", "sgc_relhead.h")).read()
    names = set(re.findall(r"\bint\s+(sgc_\w+)\s*\(", hdr))
    assert "sgc_conv1_dgrad" in names and "sgc_generic_conv1_dgrad" in names
    doc = hdr[:hdr.index("int sgc_conv1_dgrad(")][-1500:]
    assert "model.py:139-140" in doc and "train_test.py:194-195" in doc            # the reference lines whose backward it is
    assert os.path.exists(os.path.join(REPO, "scene_graph_commonsense_amd", "csrc", "kernels_inputgrad.hip"))


def test_public_calls_take_the_switch_and_default_to_off():
    from scene_graph_commonsense_amd.engine_bwd import BackwardMixin
    from scene_graph_commonsense_amd.model import _RelationBase
    from scene_graph_commonsense_amd.pair_loop import train_minibatch
    assert inspect.signature(train_minibatch).parameters["input_grads"].default is False
    assert inspect.signature(_RelationBase.training_step).parameters["input_grads"].default is False
    assert inspect.signature(BackwardMixin.train_backward).parameters["input_grads"].default is None


def test_oracle_input_gradient_vanishes_outside_the_union_of_boxes():
    from oracle import relhead_oracle as O
    from scene_graph_commonsense_amd.synthetic import HeadConfig, make_scene_batch, make_state_dict, predicate_counts
    cfg = HeadConfig(hidden_dim=16, feature_size=8)
    sd = make_state_dict(cfg, seed=21, head_gain=4.0)
    batch = make_scene_batch(cfg, (4, 3, 2), seed=21, connect_frac=0.6, edge_boxes=True)
    feat, depth = batch.image_feature.clone().requires_grad_(True), batch.image_depth.clone().requires_grad_(True)
    out = O.run_pair_loop(sd, dataclasses.replace(batch, image_feature=feat, image_depth=depth), cfg, mode="train",
                          weights=O.class_weights(predicate_counts(cfg)))
    out["losses"].backward()
    F = cfg.feature_size
    outside = ~torch.stack([O.build_masks(b, F).any(dim=0) for b in batch.bbox])
    assert bool(outside.any()) and bool((~outside).any())
    for g in (feat.grad, depth.grad):
        assert bool((g.permute(1, 0, 2, 3)[:, outside] == 0).all())
        assert bool((g.permute(1, 0, 2, 3)[:, ~outside] != 0).any())
