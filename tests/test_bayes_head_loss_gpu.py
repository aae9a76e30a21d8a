"""``BayesianHead.hierarchical_nll`` (the reference's class-weighted hierarchical loss, train_utils.py:116-157, fused into the head's
forward and backward) and ``BayesianHead.candidates`` (evaluator.py:160-174) on the HIP head kernels (csrc/kernels_head.hip): against
the goldens of the REAL reference (tests/golden/head_train.npz), a float64 restatement written here, the unfused path on the device,
and the evaluator fed both ways.  Every bar is 1e-5 x the largest |value| of the compared tensor unless stated."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.golden_cases import GOLDEN
from tests.head_train_cases import CASES, SGD_LR, SGD_STEPS, SPLIT, TEMPS, head_case, hierarchical_nll, sample

pytestmark = pytest.mark.gpu
TOL = 1e-5
PARAMS = ("fc3_1.weight", "fc3_1.bias", "fc3_2.weight", "fc3_2.bias", "fc3_3.weight", "fc3_3.bias", "fc5.weight", "fc5.bias")
R = sum(SPLIT)
OFF = (0, SPLIT[0], SPLIT[0] + SPLIT[1], R)
SHAPES = [(D, M) for D in (1, 100, 512, 4096) for M in (0, 1, 37, 4099, 65536)]


def _close(got, ref, what, tol=TOL):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.numel() == 0:
        return
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    print(what, "err %.3e scale %.3e" % (err, scale))
    assert err <= tol * scale, (what, err, scale)


def _head(D, split=SPLIT, temps=TEMPS, seed=0):
    from scene_graph_commonsense_amd.model import BayesianHead
    torch.manual_seed(seed)
    return BayesianHead(D, *split, T1=temps[0], T2=temps[1], T3=temps[2]).cuda()


def _targets(M, gen, empty_block=None):
    """[M] int64 on the device: 3 rows in 10 negative ("no relation"), 2 in block 0, 2 in block 1, 3 in block 2, classes uniform
    inside the block, rows shuffled; row pattern starts with a connected row so that M = 1 has one.  ``empty_block``: its rows
    become "no relation"."""
    if M == 0:
        return torch.zeros(0, dtype=torch.int64, device="cuda")
    slot = (torch.arange(M, device="cuda") + 3) % 10
    blk = torch.where(slot < 3, -1, torch.where(slot < 5, 0, torch.where(slot < 7, 1, 2)))
    u = torch.rand(M, device="cuda", generator=gen)
    size = torch.tensor(SPLIT, device="cuda")[blk.clamp(min=0)]
    cls = torch.tensor(OFF[:3], device="cuda")[blk.clamp(min=0)] + (u * size).long().clamp(max=size - 1)
    neg = -1 - (u * 7).long()                                    # any negative value means "no relation"
    tgt = torch.where(blk < 0, neg, cls)
    if empty_block is not None:
        tgt = torch.where(blk == empty_block, neg, tgt)
    return tgt[torch.randperm(M, device="cuda", generator=gen)]


def _loss64(h, params, temps, tgt, cw):
    """The reference's loss in float64: the module (model.py:24-34), the selection of the connected rows (train_utils.py:118-125) and
    the criteria (tests/head_train_cases.py:hierarchical_nll).  (loss, dh, [dW1, db1, ..., dW5, db5])."""
    x = h.detach().double().requires_grad_(True)
    ps = [p.detach().double().requires_grad_(True) for p in params]
    sup = F.log_softmax(x @ ps[6].T + ps[7], dim=1)
    outs = [F.log_softmax((x @ ps[2 * k].T + ps[2 * k + 1]) / temps[k], dim=1) + sup[:, k:k + 1] for k in range(3)] + [sup]
    idx = torch.nonzero(tgt >= 0).flatten()
    w = torch.ones(R, dtype=torch.float64, device=h.device) if cw is None else cw.to(h.device).double()
    if idx.numel() == 0:
        loss = x.sum() * 0
    else:
        loss = hierarchical_nll([o[idx] for o in outs], tgt[idx].long(), w)
    grads = torch.autograd.grad(loss, [x] + ps, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, [x] + ps)]
    return loss.detach(), grads[0], grads[1:]


def _check_grads(x, head, ref_dh, ref_dp, tag, tol=TOL):
    _close(x.grad, ref_dh, ("dh",) + tag, tol)
    for pn, p, r in zip(PARAMS, head._params(), ref_dp):
        _close(p.grad, r, (pn,) + tag, tol)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "head_train.npz")))


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_loss_trains_like_the_reference(gold, name):
    D = CASES[name][0]
    h, sd, _, tgt, cw = head_case(name)
    head = _head(D)
    head.load_state_dict(sd)
    x, tgt, cw = h.cuda(), tgt.cuda(), cw.cuda()
    xg = x.clone().requires_grad_(True)
    loss = head.hierarchical_nll(xg, tgt, cw)
    assert loss.dim() == 0 and loss.grad_fn is not None
    loss.backward()
    _close(loss.detach(), gold[name + "__nll__loss"][0], "loss")
    key = name + "__nll__dh"
    _close(xg.grad.double().norm(), gold[key + "__l2"][0], key + " l2")
    _close(sample(xg.grad), gold[key + "__sample"], key)
    for pn, p in zip(PARAMS, head._params()):
        key = "%s__nll__d_%s" % (name, pn.replace(".", "_"))
        if pn.endswith("bias"):
            _close(p.grad, gold[key], key)
        else:
            _close(p.grad.double().norm(), gold[key + "__l2"][0], key + " l2")
            _close(sample(p.grad), gold[key + "__sample"], key)
    opt = torch.optim.SGD(head.parameters(), lr=SGD_LR)
    for _ in range(SGD_STEPS):
        opt.zero_grad()
        head.hierarchical_nll(x.clone().requires_grad_(True), tgt, cw).backward()
        opt.step()
    for pn, p in zip(PARAMS, head._params()):
        key = "%s__sgd__%s" % (name, pn.replace(".", "_"))
        if pn.endswith("bias"):
            _close(p, gold[key], key)
        else:
            _close(sample(p), gold[key + "__sample"], key)


@pytest.mark.parametrize("D,M", SHAPES)
def test_fused_loss_against_float64(D, M):
    i = SHAPES.index((D, M))
    gen = torch.Generator(device="cuda").manual_seed(2000 + i)
    head = _head(D, seed=i)
    h = torch.randn(M, D, device="cuda", generator=gen)
    tgt = _targets(M, gen)
    if M >= 37:
        blk = (tgt >= OFF[1]).long() + (tgt >= OFF[2]).long()
        for k in range(3):
            assert int(((tgt >= 0) & (blk == k)).sum()) >= 0.1 * M
        assert 0.2 * M <= int((tgt < 0).sum()) <= 0.4 * M        # "about 30 %"
    cw = torch.rand(R, device="cuda", generator=gen) + 0.5
    x = h.clone().requires_grad_(True)
    loss = head.hierarchical_nll(x, tgt, cw)
    loss.backward()
    ref_loss, ref_dh, ref_dp = _loss64(h, head._params(), TEMPS, tgt, cw)
    _close(loss, ref_loss, "loss")
    _check_grads(x, head, ref_dh, ref_dp, (D, M))


def _case(D=100, M=4099, seed=50, **kw):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    head = _head(D, seed=seed)
    h = torch.randn(M, D, device="cuda", generator=gen)
    return head, h, _targets(M, gen, **kw), torch.rand(R, device="cuda", generator=gen) + 0.5


@pytest.mark.parametrize("empty", [0, 1, 2])
def test_an_empty_block_drops_its_term(empty):
    head, h, tgt, cw = _case(seed=51 + empty, empty_block=empty)
    blk = (tgt >= OFF[1]).long() + (tgt >= OFF[2]).long()
    assert int(((tgt >= 0) & (blk == empty)).sum()) == 0
    x = h.clone().requires_grad_(True)
    loss = head.hierarchical_nll(x, tgt, cw)
    loss.backward()
    ref_loss, ref_dh, ref_dp = _loss64(h, head._params(), TEMPS, tgt, cw)
    _close(loss, ref_loss, "loss")
    _check_grads(x, head, ref_dh, ref_dp, ("empty", empty))


@pytest.mark.parametrize("M", [1, 37, 4099])
def test_every_row_skipped_gives_zero_loss_and_zero_gradients(M):
    head, h, _, cw = _case(M=M, seed=55)
    tgt = -1 - torch.arange(M, device="cuda") % 5
    x = h.clone().requires_grad_(True)
    loss = head.hierarchical_nll(x, tgt, cw)
    assert float(loss.detach()) == 0.0
    loss.backward()
    assert x.grad is not None and not bool(x.grad.any())
    for p in head._params():
        assert p.grad is not None and not bool(p.grad.any())


def test_class_weight_none_is_all_ones():
    head, h, tgt, _ = _case(seed=56)
    x = h.clone().requires_grad_(True)
    loss = head.hierarchical_nll(x, tgt)
    loss.backward()
    ref_loss, ref_dh, ref_dp = _loss64(h, head._params(), TEMPS, tgt, None)
    _close(loss, ref_loss, "loss")
    _check_grads(x, head, ref_dh, ref_dp, ("cw none",))


def test_int32_target_gives_the_same_bits_as_int64():
    head, h, tgt, cw = _case(seed=57)
    runs = []
    for t in (tgt, tgt.to(torch.int32)):
        head.zero_grad()
        x = h.clone().requires_grad_(True)
        loss = head.hierarchical_nll(x, t, cw)
        loss.backward()
        runs.append([loss.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in head._params()])
    ref_loss, ref_dh, _ = _loss64(h, head._params(), TEMPS, tgt, cw)
    _close(runs[1][0], ref_loss, "loss")
    _close(runs[1][1], ref_dh, "dh")
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_frozen_head_gets_the_input_gradient_only():
    head, h, tgt, cw = _case(seed=58)
    for p in head._params():
        p.requires_grad_(False)
    x = h.clone().requires_grad_(True)
    loss = head.hierarchical_nll(x, tgt, cw)
    loss.backward()
    ref_loss, ref_dh, _ = _loss64(h, head._params(), TEMPS, tgt, cw)
    _close(loss, ref_loss, "loss")
    _close(x.grad, ref_dh, "dh")
    assert all(p.grad is None for p in head._params())


def test_detached_input_gets_the_parameter_gradients_only():
    head, h, tgt, cw = _case(seed=59)
    x = h.clone()
    loss = head.hierarchical_nll(x, tgt, cw)
    assert loss.grad_fn is not None
    loss.backward()
    assert x.grad is None
    ref_loss, _, ref_dp = _loss64(h, head._params(), TEMPS, tgt, cw)
    _close(loss, ref_loss, "loss")
    for pn, p, r in zip(PARAMS, head._params(), ref_dp):
        _close(p.grad, r, pn)


def test_upstream_scalar_scales_every_gradient():
    head, h, tgt, cw = _case(seed=60)
    x = h.clone().requires_grad_(True)
    (3.5 * head.hierarchical_nll(x, tgt, cw)).backward()
    _, ref_dh, ref_dp = _loss64(h, head._params(), TEMPS, tgt, cw)
    _check_grads(x, head, 3.5 * ref_dh, [3.5 * r for r in ref_dp], ("g = 3.5",))


def test_half_precision_input_gets_its_gradient_in_its_own_dtype():
    head, h, tgt, cw = _case(D=256, M=77, seed=61)
    for dt in (torch.float16, torch.bfloat16):
        head.zero_grad()
        x = h.to(dt).requires_grad_(True)
        loss = head.hierarchical_nll(x, tgt, cw)
        assert loss.dtype == torch.float32
        loss.backward()
        assert x.grad is not None and x.grad.dtype == dt
        ref_loss, ref_dh, _ = _loss64(x.detach().float(), head._params(), TEMPS, tgt, cw)
        _close(loss, ref_loss, ("loss", dt))
        _close(x.grad.float(), ref_dh, dt, tol=1e-2)


@pytest.mark.parametrize("D,M", [(100, 4099), (512, 37), (4096, 65536)])
def test_fused_loss_matches_the_unfused_path_on_the_device(D, M):
    head, h, tgt, cw = _case(D=D, M=M, seed=62)
    x = h.clone().requires_grad_(True)
    loss = head.hierarchical_nll(x, tgt, cw)
    loss.backward()
    fused = [x.grad.clone()] + [p.grad.clone() for p in head._params()]
    head.zero_grad()
    x2 = h.clone().requires_grad_(True)
    idx = torch.nonzero(tgt >= 0).flatten()
    loss2 = hierarchical_nll([o[idx] for o in head(x2)], tgt[idx], cw)
    loss2.backward()
    _close(loss, loss2.detach(), "loss")
    for name, a, b in zip(("dh",) + PARAMS, fused, [x2.grad] + [p.grad for p in head._params()]):
        _close(a, b, name)


def test_forward_and_backward_never_wait_for_the_device():
    head, h, tgt, cw = _case(seed=63)
    x = h.clone().requires_grad_(True)
    head.hierarchical_nll(x, tgt, cw).backward()                # library loaded, weights packed
    head.zero_grad()
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = head.hierarchical_nll(x, tgt, cw)
        (2.0 * loss).backward()
        with pytest.raises(RuntimeError):                        # the mode is live on this build: a read-back is refused
            loss.item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ref_loss, ref_dh, _ = _loss64(h, head._params(), TEMPS, tgt, cw)
    _close(loss, ref_loss, "loss")
    _close(x.grad, 2.0 * ref_dh, "dh")


def test_fused_loss_is_bit_identical_between_runs():
    head = _head(1000, seed=5)
    gen = torch.Generator(device="cuda").manual_seed(6)
    h = torch.randn(20000, 1000, device="cuda", generator=gen)
    tgt = _targets(20000, gen)
    cw = torch.rand(R, device="cuda", generator=gen) + 0.5
    runs = []
    for _ in range(2):
        head.zero_grad()
        x = h.clone().requires_grad_(True)
        loss = head.hierarchical_nll(x, tgt, cw)
        loss.backward()
        runs.append([loss.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in head._params()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- candidates
def _check_candidates(head, h):
    with torch.no_grad():
        r1, r2, r3, sup = head(h)
    conf, pred, sup_c = head.candidates(h)
    M = h.shape[0]
    assert conf.shape == (M, 3) and conf.dtype == torch.float32
    assert pred.shape == (M, 3) and pred.dtype == torch.int32
    assert sup_c.shape == (M, 3) and torch.equal(sup_c, sup)
    for k, r in enumerate((r1, r2, r3)):
        if M == 0:
            continue
        mx, am = torch.max(r, dim=1)
        first = (r == mx[:, None]).int().argmax(dim=1)            # the first arg-max, whatever torch.max picks among ties
        assert torch.equal(conf[:, k], mx), k
        assert torch.equal(pred[:, k].long(), first + OFF[k]), k
    return conf, pred


@pytest.mark.parametrize("D,M", SHAPES)
def test_candidates_are_the_block_maxima_of_forward(D, M):
    i = SHAPES.index((D, M))
    gen = torch.Generator(device="cuda").manual_seed(3000 + i)
    head = _head(D, seed=100 + i)
    _check_candidates(head, torch.randn(M, D, device="cuda", generator=gen))


def test_candidates_of_a_tied_block_name_its_first_class():
    head, h, _, _ = _case(D=64, M=300, seed=64)
    with torch.no_grad():
        head.fc3_2.weight.zero_()
        head.fc3_2.bias.zero_()
        h[7] = 0                                                   # and one row whose every logit is its bias
    _, pred = _check_candidates(head, h)
    assert bool((pred[:, 1] == OFF[1]).all())
    assert not h.requires_grad and head.candidates(h.requires_grad_(True))[0].grad_fn is None


def test_evaluator_fed_candidates_equals_evaluator_fed_log_probs():
    """The oracle's pair loop supplies the per-step bookkeeping (images, categories, boxes, targets, overlap mask); the head scores
    random features of each step.  ``accumulate_candidates`` fed ``candidates(h)`` must leave the state and the ``compute()`` tuple
    that ``accumulate`` fed ``forward()``'s log-probs leaves, for Evaluator and Evaluator_Top3."""
    from oracle import relhead_oracle as O
    from scene_graph_commonsense_amd.evaluator import Evaluator, Evaluator_Top3
    from tests.golden_cases import load_case
    from tests.test_evaluator_gpu import FX
    cfg, sd, batch, _ = load_case("vg_small")
    assert (cfg.num_geometric, cfg.num_possessive, cfg.num_semantic) == SPLIT
    args = cfg.args(fixtures=FX)
    mk = lambda: (Evaluator(args, cfg.num_relations, 0.5, [20, 50, 100]), Evaluator_Top3(args, cfg.num_relations, 0.5, [20, 50, 100]))
    (ev_a, t3_a), (ev_b, t3_b) = mk(), mk()
    head = _head(96, seed=65)
    gen = torch.Generator(device="cuda").manual_seed(66)
    calls = []

    class Record:
        def accumulate(self, *a, **k):
            calls.append([x.cuda() if torch.is_tensor(x) else x for x in a])
    with torch.no_grad():
        O.run_pair_loop(sd, batch, cfg, mode="eval", evaluator=Record())
    assert calls
    for which, _, target, _, conn, cs, co, _, _, bs, bo, _, _, iou in calls:
        h = 3 * torch.randn(which.shape[0], 96, device="cuda", generator=gen)
        with torch.no_grad():
            r1, r2, r3, sup = head(h)
        rel = torch.cat((r1, r2, r3), dim=1)
        ev_a.accumulate(which, rel, target, sup, conn, cs, co, cs, co, bs, bo, bs, bo, iou)
        t3_a.accumulate(which, rel, target, sup, conn, cs, co, cs, co, bs, bo, bs, bo, iou)
        conf, pred, _ = head.candidates(h)
        ev_b.accumulate_candidates(which, conf, pred, target, conn, cs, co, bs, bo, iou_mask=iou, call_sizes=[which.shape[0]])
        t3_b.accumulate_candidates(which, conf.max(1)[0], pred, target, conn, cs, co, bs, bo, iou_mask=iou)
    for key in ev_a._l:
        a, b = ev_a._cat(key), ev_b._cat(key)
        assert a is not None and a.dtype == b.dtype and torch.equal(a, b), key
    for key in t3_a._l:
        for a, b in zip(t3_a._l[key], t3_b._l[key]):
            assert a.dtype == b.dtype and torch.equal(a, b), key

    def flat(res):
        return [np.asarray([float(v) for v in x]) if isinstance(x, list) and not torch.is_tensor(x[0])
                else np.stack([v.numpy() for v in x]) for x in res if x is not None]
    for a, b in ((ev_a.compute(per_class=True), ev_b.compute(per_class=True)), (t3_a.compute(per_class=True), t3_b.compute(per_class=True))):
        fa, fb = flat(a), flat(b)
        assert len(fa) == len(fb) and len(fa) > 0
        for u, v in zip(fa, fb):
            np.testing.assert_array_equal(u, v)
    assert ev_a.num_connected_target == ev_b.num_connected_target > 0
