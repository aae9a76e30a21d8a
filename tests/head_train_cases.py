"""Seeded inputs and losses of the BayesianHead training goldens (tests/golden/make_head_train_golden.py runs the REAL reference on
them, tests/test_bayes_head_train_gpu.py the HIP head)."""
import numpy as np
import torch
import torch.nn.functional as F

from scene_graph_commonsense_amd.synthetic import hash_normal, hash_randint, hash_uniform

SPLIT = (15, 11, 24)
TEMPS = (1.0, 2.0, 0.5)
CASES = {"d512": (512, 40, 11), "d1024": (1024, 64, 12)}    # name: (input_dim, rows, seed)
SGD_LR, SGD_STEPS = 0.5, 3
SAMPLE = 509                                                  # entries kept of a large tensor (boundary.npz's stepgrad_sample form)


def head_case(name):
    """h [M,D] (non-negative: the head sits behind a ReLU), a BayesianHead state_dict, fixed upstream weights on the four outputs,
    relation targets [M] and the class weights of the hierarchical NLL."""
    D, M, seed = CASES[name]
    h = torch.from_numpy(np.maximum(hash_normal(seed, M * D), 0).reshape(M, D))
    a = float(2.0 / np.sqrt(D))
    sd = {}
    for k, (n, rows) in enumerate((("fc3_1", SPLIT[0]), ("fc3_2", SPLIT[1]), ("fc3_3", SPLIT[2]), ("fc5", 3))):
        sd[n + ".weight"] = torch.from_numpy(hash_uniform(seed * 7 + k, rows * D, -a, a).reshape(rows, D))
        sd[n + ".bias"] = torch.from_numpy(hash_uniform(seed * 7 + k + 100, rows, -0.5, 0.5))
    R = sum(SPLIT)
    up = [torch.from_numpy(hash_uniform(seed * 13 + k, M * c, -1, 1).reshape(M, c)) for k, c in enumerate(SPLIT + (3,))]
    tgt = torch.from_numpy(hash_randint(seed * 17, M, 0, R))
    counts = torch.from_numpy(hash_uniform(seed * 19, R, 10.0, 1000.0))
    return h, sd, up, tgt, 1 - counts / counts.sum()


def upstream_loss(outs, up):
    """Fixed random weights on all four outputs."""
    return sum((o * u).sum() for o, u in zip(outs, up))


def hierarchical_nll(outs, tgt, class_weight):
    """The reference's class-weighted hierarchical loss (train_test.py:105-117, train_utils.py:131-151): NLL of the super category
    plus the class-weighted NLL of each block on the rows whose target lies in it."""
    r1, r2, r3, sup = outs
    off = (0, SPLIT[0], SPLIT[0] + SPLIT[1], sum(SPLIT))
    st = (tgt >= off[1]).long() + (tgt >= off[2]).long()
    loss = F.nll_loss(sup, st)
    for k, r in enumerate((r1, r2, r3)):
        idx = torch.nonzero(st == k).flatten()
        if idx.numel():
            loss = loss + F.nll_loss(r[idx], tgt[idx] - off[k], weight=class_weight[off[k]:off[k + 1]].to(r.device))
    return loss


def sample(t):
    flat = t.detach().flatten()
    stride = max(1, flat.numel() // SAMPLE)
    return flat[::stride][:SAMPLE]
