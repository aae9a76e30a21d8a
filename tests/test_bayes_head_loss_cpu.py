"""The plug-and-play head's fused loss and candidate scoring: the launchers are declared, and both methods refuse CPU tensors."""
import os
import re

import pytest
import torch

from scene_graph_commonsense_amd.model import BayesianHead


def test_loss_and_candidate_entry_points_are_declared():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgc_relhead.h")).read()
    names = set(re.findall(r"\bint\s+(sgc_\w+)\s*\(", hdr))
    assert {"sgc_bayes_head_any_loss", "sgc_bayes_head_any_loss_bwd", "sgc_bayes_head_any_candidates"} <= names


def test_both_methods_are_gpu_only():
    head = BayesianHead(input_dim=32)
    with pytest.raises(RuntimeError, match="GPU"):
        head.hierarchical_nll(torch.zeros(2, 32), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU"):
        head.candidates(torch.zeros(2, 32))
