"""``BayesianHead.hierarchical_nll(..., commonsense=)``, ``commonsense_penalty`` and ``candidates(..., commonsense=)``: the penalty of
run_mode train_cs (reference train_utils.py:36-60) and the filter of eval_cs (evaluator.py:189-194) fused into the head kernels
(csrc/kernels_head.hip).  Against the goldens of the REAL reference (tests/golden/head_cs.npz), the float64 restatement of
tests/head_cs_cases.py (which takes the device's predicates), the call without commonsense, and the evaluator fed both ways.  Every
bar is 1e-5 x the largest |value| of the compared tensor unless stated: the epilogue does the same kind of f32 arithmetic on the same
logits as the loss the existing head tests hold to that bar."""
import os

import numpy as np
import pytest
import torch

from tests.golden_cases import GOLDEN
from tests.head_cs_cases import C, GAP_TOL, LAMBDA_STRONG, LAMBDA_WEAK, R, cs_case, cs_sets, flags, penalty64, top2_gaps
from tests.head_train_cases import CASES, TEMPS, sample
from tests.test_bayes_head_loss_gpu import PARAMS, _close, _head, _loss64, _targets

pytestmark = pytest.mark.gpu
SHAPES = [(D, M) for D in (1, 101, 512) for M in (0, 1, 37, 4099)] + [(64, 32805)]      # 32805: the smallest 64-row-tile M + 37
KINDS = ("mixed", "none_fires", "strong_only", "nothing_aligned")
LAM = 0.7                                                          # lambda_commonsense of these tests (the default 1 hides a lost factor)
_SETS = {}


def _sets(kind):
    """(aligned, violated) bool [C, R, C] on the device and their TripletBitmaps, built once per kind."""
    if kind not in _SETS:
        from scene_graph_commonsense_amd.commonsense import TripletBitmaps
        al, vi = cs_sets(77)
        full, none = torch.ones_like(al), torch.zeros_like(al)
        al, vi = {"mixed": (al, vi), "none_fires": (full, none), "strong_only": (full, vi), "nothing_aligned": (none, vi),
                  "weak_only": (al, none)}[kind]
        _SETS[kind] = (al.cuda(), vi.cuda(), TripletBitmaps.from_masks(al, vi, "cuda"))
    return _SETS[kind]


def _cats(M, gen, out_of_range):
    sc = torch.randint(0, C, (M,), device="cuda", generator=gen)
    oc = torch.randint(0, C, (M,), device="cuda", generator=gen)
    if out_of_range:                                               # in neither set: weak, not strong
        sc[3::11] = C + 7
        oc[5::13] = -3
    return sc, oc


def _case(D=101, M=4099, seed=70, kind="mixed"):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    head = _head(D, seed=seed)
    h = torch.randn(M, D, device="cuda", generator=gen)
    tgt = _targets(M, gen)
    cw = torch.rand(R, device="cuda", generator=gen) + 0.5
    sc, oc = _cats(M, gen, kind == "mixed")
    return head, h, tgt, cw, sc, oc


def _run(head, h, fn):
    """loss, (nll, penalty), counts, dh, parameter gradients of one call ``fn(x)`` and its backward."""
    head.zero_grad()
    x = h.clone().requires_grad_(True)
    loss = fn(x)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.grad_fn is not None
    terms, counts = head.last_loss_terms, head.last_cs_counts
    assert all(t.dim() == 0 and not t.requires_grad and t.is_cuda for t in terms)
    assert counts.dtype == torch.int64 and counts.shape == (2,) and counts.is_cuda
    loss.backward()
    return loss.detach().clone(), [t.clone() for t in terms], counts.clone(), x.grad.clone(), [p.grad.clone() for p in head._params()]


def _reference(head, h, tgt, cw, sc, oc, kind, lam=LAM):
    """Float64: (nll, penalty, counts, dh / dparams of the NLL, dh / dparams of the penalty, device predicates)."""
    al, vi, _ = _sets(kind)
    pred = head.candidates(h)[1]
    weak, strong = flags(pred, sc, oc, al, vi)
    pen, dh_p, dps_p = penalty64(h, head._params(), pred, weak, strong, LAMBDA_WEAK, LAMBDA_STRONG, TEMPS)
    nll, dh_n, dps_n = _loss64(h, head._params(), TEMPS, tgt, cw)
    counts = torch.stack((weak.sum(), strong.sum())).cpu()
    return nll, pen, counts, (dh_n, dps_n), (dh_p, dps_p), pred


def _check(got, ref_loss, ref_terms, ref_counts, ref_dh, ref_dps, tag, tol=1e-5):
    loss, terms, counts, dh, dps = got
    _close(loss, ref_loss, ("loss",) + tag, tol)
    _close(terms[0], ref_terms[0], ("nll",) + tag, tol)
    _close(terms[1], ref_terms[1], ("penalty",) + tag, tol)
    assert torch.equal(counts.cpu(), ref_counts), (tag, counts, ref_counts)
    _close(dh, ref_dh, ("dh",) + tag, tol)
    for pn, g, r in zip(PARAMS, dps, ref_dps):
        _close(g, r, (pn,) + tag, tol)


def _both_calls_against_float64(head, h, tgt, cw, sc, oc, kind, tag):
    _, _, bm = _sets(kind)
    nll, pen, counts, (dh_n, dps_n), (dh_p, dps_p), pred = _reference(head, h, tgt, cw, sc, oc, kind)
    got = _run(head, h, lambda x: head.hierarchical_nll(x, tgt, cw, commonsense=bm, subject_cat=sc, object_cat=oc, lambda_commonsense=LAM))
    _check(got, nll + LAM * pen, (nll, pen), counts, dh_n + LAM * dh_p, [a + LAM * b for a, b in zip(dps_n, dps_p)], tag + ("nll+cs",))
    got_p = _run(head, h, lambda x: head.commonsense_penalty(x, sc, oc, bm))
    _check(got_p, pen, (torch.zeros(()), pen), counts, dh_p, dps_p, tag + ("penalty",))
    assert float(got_p[1][0]) == 0.0 and torch.equal(got_p[0], got_p[1][1])       # the penalty alone: no NLL, the result is the term
    assert torch.equal(got[1][1], got_p[1][1])                                     # and the same bits in both calls
    assert not bool(got_p[4][6].any()) and not bool(got_p[4][7].any())             # zero on the three super logits
    return got, pred, counts


# ---------------------------------------------------------------------------------------------------- 1. the real reference
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "head_cs.npz")))


@pytest.mark.parametrize("name", sorted(CASES))
def test_penalty_and_filter_match_the_reference(gold, name):
    from scene_graph_commonsense_amd.commonsense import TripletBitmaps
    D, M, _ = CASES[name]
    h, sd, tgt, cw, sc, oc, aligned, violated = cs_case(name)
    head = _head(D)
    head.load_state_dict(sd)
    bm = TripletBitmaps.from_masks(aligned, violated, "cuda")
    h, sc, oc = h.cuda(), sc.cuda(), oc.cuda()
    loss, terms, counts, dh, dps = _run(head, h, lambda x: head.commonsense_penalty(x, sc, oc, bm))
    _close(loss, gold[name + "__penalty"][0], "penalty")
    assert counts.cpu().tolist() == gold[name + "__counts"].tolist()
    _close(dh.double().norm(), gold[name + "__dh__l2"][0], "dh l2")
    _close(sample(dh), gold[name + "__dh__sample"], "dh")
    fine_scale = 0.0
    for pn, g in zip(PARAMS[:6], dps[:6]):
        key = "%s__d_%s" % (name, pn.replace(".", "_"))
        if pn.endswith("bias"):
            _close(g, gold[key], key)
            fine_scale = max(fine_scale, float(np.abs(gold[key]).max()))
        else:
            _close(g.double().norm(), gold[key + "__l2"][0], key + " l2")
            _close(sample(g), gold[key + "__sample"], key)
            fine_scale = max(fine_scale, float(np.abs(gold[key + "__sample"]).max()))
    # fc5: the penalty does not depend on the super logits (softmax is shift-invariant), so the gradient is exactly zero here; the
    # reference's autograd leaves rounding noise of the sum p (1 - sum softmax), far below the bar on the scale of the other gradients
    assert not bool(dps[6].any()) and not bool(dps[7].any())
    assert float(np.abs(gold[name + "__d_fc5_weight__sample"]).max()) <= 1e-5 * fine_scale
    assert float(np.abs(gold[name + "__d_fc5_bias"]).max()) <= 1e-5 * fine_scale
    # the same term inside hierarchical_nll, and the gradient of the sum against reference NLL + reference penalty (head_train.npz)
    train = dict(np.load(os.path.join(GOLDEN, "head_train.npz")))
    got = _run(head, h, lambda x: head.hierarchical_nll(x, tgt.cuda(), cw.cuda(), commonsense=bm, subject_cat=sc, object_cat=oc))
    assert torch.equal(got[1][1], terms[1]) and torch.equal(got[2], counts)
    _close(got[1][0], train[name + "__nll__loss"][0], "nll")
    _close(got[0], train[name + "__nll__loss"][0] + gold[name + "__penalty"][0], "nll + penalty")
    _close(sample(got[3]), train[name + "__nll__dh__sample"] + gold[name + "__dh__sample"], "dh of the sum")
    # eval_cs: the reference's Evaluator.accumulate keeps its candidates block after block
    conf, pred, _ = head.candidates(h, commonsense=bm, subject_cat=sc, object_cat=oc)
    conf, ref = conf.T.reshape(-1).cpu().numpy(), gold[name + "__ev_confidence"]
    np.testing.assert_array_equal(pred.T.reshape(-1).cpu().numpy(), gold[name + "__ev_relation_pred"])
    np.testing.assert_array_equal(np.isneginf(conf), np.isneginf(ref))
    assert 0 < int(np.isneginf(ref).sum()) < ref.size
    _close(conf[np.isfinite(ref)], ref[np.isfinite(ref)], "confidence")


# ---------------------------------------------------------------------------------------------------- 2. float64, all shapes
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,M", SHAPES)
def test_against_float64(D, M, kind):
    i = SHAPES.index((D, M)) * len(KINDS) + KINDS.index(kind)
    head, h, tgt, cw, sc, oc = _case(D, M, seed=4000 + i, kind=kind)
    got, pred, counts = _both_calls_against_float64(head, h, tgt, cw, sc, oc, kind, (D, M, kind))
    if kind == "none_fires":
        assert counts.tolist() == [0, 0]
    if kind == "strong_only":
        assert int(counts[0]) == 0
    if kind == "nothing_aligned":
        assert int(counts[0]) == 3 * M
    if kind == "mixed" and M >= 37:
        assert int(counts[0]) > 0 and int(counts[1]) > 0
    # the device's predicates are the float64 arg-max wherever float64 decides it above the head's f32 error
    pred64, gap, big = top2_gaps(h, head._params())
    decided = gap > GAP_TOL * big
    assert torch.equal(pred.long()[decided], pred64[decided])
    if M:
        share = 1.0 - float(decided.float().mean())
        print("undecided share", share)
        assert share <= 0.01


# ---------------------------------------------------------------------------------------------------- 3. no flag fires
@pytest.mark.parametrize("D,M", [(101, 4099), (64, 32805)])
def test_no_flag_gives_the_bits_of_the_call_without_commonsense(D, M):
    head, h, tgt, cw, sc, oc = _case(D, M, seed=71, kind="none_fires")
    _, _, bm = _sets("none_fires")
    got = _run(head, h, lambda x: head.hierarchical_nll(x, tgt, cw, commonsense=bm, subject_cat=sc, object_cat=oc, lambda_commonsense=LAM))
    head.zero_grad()
    x = h.clone().requires_grad_(True)
    loss = head.hierarchical_nll(x, tgt, cw)
    loss.backward()
    assert float(got[1][1]) == 0.0 and got[2].tolist() == [0, 0]
    assert torch.equal(got[0], loss.detach()) and torch.equal(got[1][0], loss.detach())
    assert torch.equal(got[3], x.grad)
    for g, p in zip(got[4], head._params()):
        assert torch.equal(g, p.grad)


# ---------------------------------------------------------------------------------------------------- 4. only one term
@pytest.mark.parametrize("kind,empty", [("weak_only", 1), ("strong_only", 0)])
def test_a_term_without_candidates_is_dropped(kind, empty):
    head, h, tgt, cw, sc, oc = _case(seed=72 + empty, kind=kind)
    got, _, counts = _both_calls_against_float64(head, h, tgt, cw, sc, oc, kind, (kind,))
    assert int(counts[empty]) == 0 and int(counts[1 - empty]) > 0
    assert all(bool(torch.isfinite(t).all()) for t in [got[0], got[3]] + got[1] + got[4])


# ---------------------------------------------------------------------------------------------------- 5. no relation target
@pytest.mark.parametrize("M", [1, 37, 4099])
def test_rows_without_a_target_still_carry_the_penalty(M):
    head, h, _, cw, sc, oc = _case(M=M, seed=74, kind="nothing_aligned")
    tgt = -1 - torch.arange(M, device="cuda") % 5
    got, _, counts = _both_calls_against_float64(head, h, tgt, cw, sc, oc, "nothing_aligned", ("no target", M))
    assert float(got[1][0]) == 0.0 and int(counts[0]) == 3 * M and float(got[1][1]) > 0.0
    assert bool(got[3].any())


# ---------------------------------------------------------------------------------------------------- 6. gradient plumbing
def _cs_call(head, tgt, cw, sc, oc, bm):
    return lambda x: head.hierarchical_nll(x, tgt, cw, commonsense=bm, subject_cat=sc, object_cat=oc, lambda_commonsense=LAM)


def test_frozen_head_gets_the_input_gradient_only():
    head, h, tgt, cw, sc, oc = _case(seed=75)
    nll, pen, _, (dh_n, _), (dh_p, _), _ = _reference(head, h, tgt, cw, sc, oc, "mixed")
    for p in head._params():
        p.requires_grad_(False)
    x = h.clone().requires_grad_(True)
    loss = _cs_call(head, tgt, cw, sc, oc, _sets("mixed")[2])(x)
    loss.backward()
    _close(loss, nll + LAM * pen, "loss")
    _close(x.grad, dh_n + LAM * dh_p, "dh")
    assert all(p.grad is None for p in head._params())


def test_detached_input_gets_the_parameter_gradients_only():
    head, h, tgt, cw, sc, oc = _case(seed=76)
    nll, pen, _, (_, dps_n), (_, dps_p), _ = _reference(head, h, tgt, cw, sc, oc, "mixed")
    x = h.clone()
    loss = _cs_call(head, tgt, cw, sc, oc, _sets("mixed")[2])(x)
    assert loss.grad_fn is not None
    loss.backward()
    assert x.grad is None
    _close(loss, nll + LAM * pen, "loss")
    for pn, p, a, b in zip(PARAMS, head._params(), dps_n, dps_p):
        _close(p.grad, a + LAM * b, pn)


def test_upstream_scalar_scales_every_gradient():
    head, h, tgt, cw, sc, oc = _case(seed=77)
    _, _, _, (dh_n, dps_n), (dh_p, dps_p), _ = _reference(head, h, tgt, cw, sc, oc, "mixed")
    call = _cs_call(head, tgt, cw, sc, oc, _sets("mixed")[2])
    got = _run(head, h, lambda x: 3.5 * call(x))
    _close(got[3], 3.5 * (dh_n + LAM * dh_p), "dh")
    for pn, g, a, b in zip(PARAMS, got[4], dps_n, dps_p):
        _close(g, 3.5 * (a + LAM * b), pn)


def test_half_precision_input_gets_its_gradient_in_its_own_dtype():
    head, h, tgt, cw, sc, oc = _case(D=256, M=77, seed=78)
    call = _cs_call(head, tgt, cw, sc, oc, _sets("mixed")[2])
    for dt in (torch.float16, torch.bfloat16):
        head.zero_grad()
        x = h.to(dt).requires_grad_(True)
        loss = call(x)
        assert loss.dtype == torch.float32
        loss.backward()
        assert x.grad is not None and x.grad.dtype == dt
        nll, pen, _, (dh_n, _), (dh_p, _), _ = _reference(head, x.detach().float(), tgt, cw, sc, oc, "mixed")
        _close(loss, nll + LAM * pen, ("loss", dt))
        _close(x.grad.float(), dh_n + LAM * dh_p, dt, tol=1e-2)     # the gradient's 8-11 mantissa bits, not the kernel


def test_int32_categories_give_the_same_bits_as_int64():
    head, h, tgt, cw, sc, oc = _case(seed=79)
    bm = _sets("mixed")[2]
    runs = [_run(head, h, _cs_call(head, tgt, cw, s, o, bm)) for s, o in ((sc, oc), (sc.int(), oc.int()), (sc.int(), oc))]
    cands = [head.candidates(h, commonsense=bm, subject_cat=s, object_cat=o) for s, o in ((sc, oc), (sc.int(), oc.int()))]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            for u, v in zip(a if isinstance(a, list) else [a], b if isinstance(b, list) else [b]):
                assert torch.equal(u, v)
    assert all(torch.equal(u, v) for u, v in zip(*cands))


# ---------------------------------------------------------------------------------------------------- 7. determinism
def test_two_runs_are_bit_identical():
    head, h, tgt, cw, sc, oc = _case(D=1000, M=20000, seed=80)
    call = _cs_call(head, tgt, cw, sc, oc, _sets("mixed")[2])
    a, b = _run(head, h, call), _run(head, h, call)
    for u, v in zip([a[0], a[2], a[3]] + a[1] + a[4], [b[0], b[2], b[3]] + b[1] + b[4]):
        assert torch.equal(u, v)
    assert int(a[2][0]) > 0 and int(a[2][1]) > 0


# ---------------------------------------------------------------------------------------------------- 8. no host synchronisation
def test_nothing_waits_for_the_device():
    head, h, tgt, cw, sc, oc = _case(seed=81)
    bm = _sets("mixed")[2]
    nll, pen, _, (dh_n, _), (dh_p, _), _ = _reference(head, h, tgt, cw, sc, oc, "mixed")
    x = h.clone().requires_grad_(True)
    _cs_call(head, tgt, cw, sc, oc, bm)(x).backward()              # library loaded, weights packed
    head.zero_grad()
    x.grad = None
    x2 = h.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = _cs_call(head, tgt, cw, sc, oc, bm)(x)
        (2.0 * loss).backward()
        head.commonsense_penalty(x2, sc, oc, bm).backward()
        conf, _, _ = head.candidates(h, commonsense=bm, subject_cat=sc, object_cat=oc)
        with pytest.raises(RuntimeError):                          # the mode is live on this build: a read-back is refused
            loss.item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _close(loss, nll + LAM * pen, "loss")
    _close(x.grad, 2.0 * (dh_n + LAM * dh_p), "dh")
    _close(x2.grad, dh_p, "dh of the penalty")
    assert bool(torch.isneginf(conf).any())


# ---------------------------------------------------------------------------------------------------- 9. filtered candidates
@pytest.mark.parametrize("D,M", SHAPES)
def test_filtered_candidates_equal_candidates_then_filter(D, M):
    head, h, _, _, sc, oc = _case(D, M, seed=5000 + SHAPES.index((D, M)))
    bm = _sets("mixed")[2]
    conf0, pred0, sup0 = head.candidates(h)
    conf, pred, sup = head.candidates(h, commonsense=bm, subject_cat=sc, object_cat=oc)
    assert conf.shape == (M, 3) and conf.dtype == torch.float32 and pred.dtype == torch.int32
    assert torch.equal(pred, pred0) and torch.equal(sup, sup0)
    want = conf0.T.reshape(-1).contiguous().clone()               # the evaluator's hstacked order: block after block
    bm.filter_(sc.repeat(3), pred0.T.reshape(-1), oc.repeat(3), want)
    assert torch.equal(conf.T.reshape(-1), want)
    if M >= 37:
        assert 0 < int(torch.isneginf(conf).sum()) < 3 * M
        assert torch.equal(conf[~torch.isneginf(conf)], conf0[~torch.isneginf(conf)])


def test_plain_evaluator_fed_filtered_candidates_equals_eval_cs_evaluator(tmp_path):
    from scene_graph_commonsense_amd.commonsense import TripletBitmaps
    from scene_graph_commonsense_amd.evaluator import Evaluator
    from scene_graph_commonsense_amd.synthetic import HeadConfig
    from tests.test_evaluator_gpu import FX
    n = 12                                                         # the sets live on the first 12 classes: small dicts, dense enough
    al, vi = cs_sets(78)
    keys = [[tuple(k) for k in torch.nonzero(m[:n, :, :n]).tolist()] for m in (al, vi)]
    for name, ks in zip(("aligned", "violated"), keys):
        torch.save({k: 1 for k in ks}, str(tmp_path / (name + ".pt")))
    cfg = HeadConfig()
    args = cfg.args(fixtures=FX)
    args_cs = cfg.args(run_mode="eval_cs", fixtures=FX)
    args_cs["dataset"]["commonsense_aligned_triplets"] = str(tmp_path / "aligned.pt")
    args_cs["dataset"]["commonsense_violated_triplets"] = str(tmp_path / "violated.pt")
    ev_plain, ev_cs = Evaluator(args, R, 0.5, [20, 50, 100]), Evaluator(args_cs, R, 0.5, [20, 50, 100])
    bm = TripletBitmaps(keys[0], keys[1], C, R, "cuda")
    head = _head(96, seed=82)
    gen = torch.Generator(device="cuda").manual_seed(83)
    for M in (61, 200):
        h = 3 * torch.randn(M, 96, device="cuda", generator=gen)
        which = torch.sort(torch.randint(0, 3, (M,), device="cuda", generator=gen))[0]
        sc = torch.randint(0, n + 2, (M,), device="cuda", generator=gen)       # classes n, n + 1: in neither set
        oc = torch.randint(0, n + 2, (M,), device="cuda", generator=gen)
        tgt = torch.randint(-1, R, (M,), device="cuda", generator=gen)
        conn = torch.nn.functional.logsigmoid(torch.randn(M, device="cuda", generator=gen))
        bs, bo = (torch.randint(0, 32, (M, 4), device="cuda", generator=gen).float() for _ in range(2))
        iou = torch.rand(M, device="cuda", generator=gen) < 0.8
        conf, pred, _ = head.candidates(h)
        ev_cs.accumulate_candidates(which, conf, pred, tgt, conn, sc, oc, bs, bo, iou_mask=iou, call_sizes=[M])
        conf_f, pred_f, _ = head.candidates(h, commonsense=bm, subject_cat=sc, object_cat=oc)
        ev_plain.accumulate_candidates(which, conf_f, pred_f, tgt, conn, sc, oc, bs, bo, iou_mask=iou, call_sizes=[M])
    for key in ev_cs._l:
        a, b = ev_cs._cat(key), ev_plain._cat(key)
        assert a is not None and a.dtype == b.dtype and torch.equal(a, b), key
    kept = ~torch.isneginf(ev_cs.confidence)
    assert 0 < int(kept.sum()) < kept.numel()
