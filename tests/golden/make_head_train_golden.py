#!/usr/bin/env python3
"""Training goldens of the plug-and-play ``BayesianHead`` (model.py:9-34) from the REAL reference (build container only; needs the
reference): for input_dim 512 and 1024 (tests/head_train_cases.py) the four outputs, the gradients dh / dW / db of two losses (fixed
upstream weights on all four outputs; the class-weighted hierarchical NLL of train_test.py:105-117) and the weights after three
plain SGD steps on the NLL.  Large tensors are stored as their L2 norm plus a fixed sample of entries.  Only data is stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_head_train_golden.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G                      # noqa: E402  (stubs + reference import helpers of the main generator)

import numpy as np                           # noqa: E402
import torch                                 # noqa: E402

sys.path.insert(0, G.REPO)
from tests.head_train_cases import (CASES, SGD_LR, SGD_STEPS, SPLIT, TEMPS, head_case, hierarchical_nll,  # noqa: E402
                                    sample, upstream_loss)


def _store(out, key, t, whole):
    t = t.detach()
    if whole:
        out[key] = t.numpy().copy()
    else:
        out[key + "__l2"] = np.array([float(t.double().norm())])
        out[key + "__sample"] = sample(t).numpy().copy()


def main():
    ref_model, _, _ = G.import_reference()
    out = {}
    for name, (D, M, _) in CASES.items():
        h, sd, up, tgt, cw = head_case(name)
        head = ref_model.BayesianHead(input_dim=D, num_geometric=SPLIT[0], num_possessive=SPLIT[1], num_semantic=SPLIT[2],
                                      T1=TEMPS[0], T2=TEMPS[1], T3=TEMPS[2])
        head.load_state_dict(sd)
        with torch.no_grad():
            outs = head(h)
        for k, o in enumerate(outs):
            out["%s__out%d" % (name, k)] = o.numpy().copy()
        for lname, fn in (("up", lambda o: upstream_loss(o, up)), ("nll", lambda o: hierarchical_nll(o, tgt, cw))):
            head.zero_grad()
            x = h.clone().requires_grad_(True)
            loss = fn(head(x))
            loss.backward()
            out["%s__%s__loss" % (name, lname)] = np.array([float(loss)])
            _store(out, "%s__%s__dh" % (name, lname), x.grad, False)
            for pn, p in head.named_parameters():
                _store(out, "%s__%s__d_%s" % (name, lname, pn.replace(".", "_")), p.grad, pn.endswith("bias"))
        opt = torch.optim.SGD(head.parameters(), lr=SGD_LR)
        for _ in range(SGD_STEPS):
            opt.zero_grad()
            hierarchical_nll(head(h), tgt, cw).backward()
            opt.step()
        for pn, p in head.named_parameters():
            _store(out, "%s__sgd__%s" % (name, pn.replace(".", "_")), p, pn.endswith("bias"))
    path = os.path.join(HERE, "head_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
