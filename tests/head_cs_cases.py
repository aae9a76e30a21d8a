"""Seeded categories and commonsense triplet sets on top of tests/head_train_cases.py, and the commonsense penalty of run_mode train_cs
(reference train_utils.py:36-60, hierarchical branch) restated in float64.  tests/golden/make_head_cs_golden.py runs the REAL reference
on these inputs, tests/test_bayes_head_cs_gpu.py the HIP head; tests/test_bayes_head_cs_cpu.py checks the cases themselves."""
import numpy as np
import torch
import torch.nn.functional as F

from scene_graph_commonsense_amd.synthetic import hash_randint, hash_uniform
from tests.head_train_cases import CASES, SPLIT, TEMPS, head_case

C = 150                                                       # object classes of the triplet sets
R = sum(SPLIT)
OFF = (0, SPLIT[0], SPLIT[0] + SPLIT[1], R)
LAMBDA_WEAK, LAMBDA_STRONG = 0.1, 10.0                        # the reference's config.yaml:68-69
GAP_TOL = 2e-5                                                # top-2 gap bar: 2 x the head tests' 1e-5, x the largest |log-prob|


def cs_sets(seed, p_aligned=0.6, p_violated=0.1):
    """bool [C, R, C] x 2: triplet (s, r, o) is aligned / violated; independent, so some triplets are both."""
    n = C * R * C
    aligned = hash_uniform(seed * 23 + 1, n, 0.0, 1.0) < p_aligned
    violated = hash_uniform(seed * 23 + 2, n, 0.0, 1.0) < p_violated
    return torch.from_numpy(aligned.reshape(C, R, C)), torch.from_numpy(violated.reshape(C, R, C))


def cs_case(name):
    """head_case(name) plus subject / object categories [M] int64 (a few outside [0, C): in neither set) and the two sets."""
    _, M, seed = CASES[name]
    h, sd, _, tgt, cw = head_case(name)
    sc, oc = hash_randint(seed * 29, M, 0, C), hash_randint(seed * 31, M, 0, C)
    sc[3::11] = C + 7                                          # past the bitmap
    oc[5::13] = -3                                             # negative
    aligned, violated = cs_sets(seed)
    return h, sd, tgt, cw, torch.from_numpy(sc), torch.from_numpy(oc), aligned, violated


def lookup(mask, s, r, o):
    """mask[s, r, o] for long tensors of one shape; False where a label is outside the mask (the reference's ``tuple in dict``)."""
    Cn, Rn = mask.shape[0], mask.shape[1]
    ok = (s >= 0) & (s < Cn) & (o >= 0) & (o < Cn) & (r >= 0) & (r < Rn)
    return mask[s.clamp(0, Cn - 1), r.clamp(0, Rn - 1), o.clamp(0, Cn - 1)] & ok


def flags(pred, sc, oc, aligned, violated):
    """(weak, strong) bool [M, 3] of the candidates (sc[m], pred[m, k], oc[m]): not aligned / violated."""
    s, o = sc.long()[:, None].expand(-1, 3), oc.long()[:, None].expand(-1, 3)
    return ~lookup(aligned, s, pred.long(), o), lookup(violated, s, pred.long(), o)


def logits64(x, ps, temps=TEMPS):
    """Float64 tempered logits of the three blocks and the module's four log-prob outputs (model.py:24-34); ps = fc3_1.weight,
    fc3_1.bias, ..., fc5.weight, fc5.bias."""
    sup = F.log_softmax(x @ ps[6].T + ps[7], dim=1)
    zs = [(x @ ps[2 * k].T + ps[2 * k + 1]) / temps[k] for k in range(3)]
    return zs, [F.log_softmax(z, dim=1) + sup[:, k:k + 1] for k, z in enumerate(zs)] + [sup]


def top2_gaps(h, params, temps=TEMPS):
    """Float64 (arg-max [M, 3] with the block offsets, top-2 gap of the log-probs [M, 3], largest |log-prob|)."""
    with torch.no_grad():
        _, outs = logits64(h.double(), [p.detach().double() for p in params], temps)
    pred, gap = [], []
    for k in range(3):
        top = torch.topk(outs[k], 2, dim=1)
        pred.append(top.indices[:, 0] + OFF[k])
        gap.append(top.values[:, 0] - top.values[:, 1])
    big = max(float(o.abs().max()) if o.numel() else 0.0 for o in outs)
    return torch.stack(pred, 1), torch.stack(gap, 1), big


def penalty64(h, params, pred, weak, strong, lambda_weak=LAMBDA_WEAK, lambda_strong=LAMBDA_STRONG, temps=TEMPS):
    """train_utils.py:56-60 in float64 with the predicates as an input: p = softmax(z_k / T_k)[pred] (a gather, no max), the mean of p
    over the weak candidates times lambda_weak plus the mean over the strong ones times lambda_strong, a term with no candidate
    dropped.  (penalty, dh, [dW1, db1, ..., dW5, db5]) - the arg-max is a constant, so fc5 gets zeros."""
    x = h.detach().double().requires_grad_(True)
    ps = [p.detach().double().requires_grad_(True) for p in params]
    zs, _ = logits64(x, ps, temps)
    p = torch.stack([F.softmax(z, dim=1).gather(1, (pred[:, k].long() - OFF[k])[:, None])[:, 0] for k, z in enumerate(zs)], 1)
    pen = x.sum() * 0
    if int(weak.sum()) > 0:
        pen = pen + lambda_weak * p[weak].mean()
    if int(strong.sum()) > 0:
        pen = pen + lambda_strong * p[strong].mean()
    grads = torch.autograd.grad(pen, [x] + ps, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, [x] + ps)]
    return pen.detach(), grads[0], grads[1:]
