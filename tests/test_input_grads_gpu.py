"""Input gradients of the relation head: d loss / d ``image_feature`` / ``image_depth`` / ``image_feature_aug`` of the fused step
(``model.training_step(input_grads=True)``, ``pair_loop.train_minibatch(input_grads=True)``) and d / d ``h_sub`` / ``h_obj`` of the
per-step autograd node, from ``sgc_conv1_dgrad`` (default sizes, bf16 MFMA) and ``sgc_generic_conv1_dgrad`` (other sizes, f32).

1. the kernel alone through the C ABI against float64 on the same bf16 operands;
2. / 3. the fused path against the oracle's autograd at the default and the small sizes;
4. an oracle-free identity between dX and the conv1 weight gradients of one call;
5. the switch changes nothing else (loss and parameter gradients bit for bit);
6. image groups, lanes and the augmented view;
7. the per-step node;
8. the autograd bridge of ``train_minibatch``.

Bars of 2, 3 and 7: the forward is f16 and the gradient tensors bf16, and a per-element input gradient does not average routing flips
of near-zero pre-activations the way a weight gradient does, so they are measured against the oracle on the MI355X (un-routed) and set
to the measured value with a margin of 1.5 (compiler / box differences; the kernels are deterministic, there is no run-to-run noise).
Measured values are the constants (``MEASURED``) and stand in profiles/input_grads_parity.txt.  Whatever is measured: cosine bar >= 0.9, error
bar <= 0.3 - a swapped role, a transposed layout or a shifted image index gives a cosine near 0."""
import ctypes
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
CP = 288                       # 257 channels padded to a multiple of 32

MARGIN = 1.5
# MEASURED on the MI355X against the oracle, un-routed: (relative Frobenius error, 1 - cosine).  The bars are MARGIN x these.
MEASURED = {
    # fused path, default sizes (test 2): f16 forward, bf16 gradient tensors, routing flips of near-zero pre-activations
    ("fused", "hier", "image_feature"): (4.4435e-02, 9.869e-04),
    ("fused", "hier", "image_depth"): (4.5466e-02, 1.034e-03),
    ("fused", "flat", "image_feature"): (3.0218e-02, 4.565e-04),
    ("fused", "flat", "image_depth"): (2.9718e-02, 4.376e-04),
    # fused path, small sizes on the generic f32 trunk (test 3): only dh1 (bf16) and h1 (f16) are 16-bit
    ("small", "hier", "image_feature"): (2.3896e-03, 2.851e-06),
    ("small", "hier", "image_depth"): (2.2125e-03, 2.266e-06),
    ("small", "flat", "image_feature"): (2.5211e-03, 3.156e-06),
    ("small", "flat", "image_depth"): (2.5440e-03, 3.233e-06),
    # per-step node (test 7)
    ("step", "default", "h_sub"): (4.0447e-02, 8.177e-04),
    ("step", "default", "h_obj"): (4.1791e-02, 8.728e-04),
    ("step", "small", "h_sub"): (2.8770e-03, 4.122e-06),
    ("step", "small", "h_obj"): (2.8853e-03, 4.150e-06),
}


def _check_bar(key, got, ref):
    g, r = got.detach().double().cpu().flatten(), ref.detach().double().cpu().flatten()
    err = float((g - r).norm() / r.norm().clamp(min=1e-30))
    cos = float((g * r).sum() / (g.norm() * r.norm()).clamp(min=1e-30))
    bar_err, bar_cos = MARGIN * MEASURED[key][0], 1.0 - MARGIN * MEASURED[key][1]
    print("input-grad parity %s: rel. Frobenius error %.4e (bar %.4e), 1 - cosine %.3e (bar %.3e)" % (key, err, bar_err, 1 - cos, 1 - bar_cos))
    assert bar_err <= 0.3 and bar_cos >= 0.9                                # hold whatever was measured
    assert err <= bar_err, (key, err)
    assert cos >= bar_cos, (key, 1 - cos)


def _model(cfg, sd):
    from scene_graph_commonsense_amd.model import BayesianRelationClassifier, FlatRelationClassifier
    if cfg.hierarchical:
        m = BayesianRelationClassifier(cfg.args(), input_dim=cfg.hidden_dim, feature_size=cfg.feature_size, num_classes=cfg.num_classes,
                                       num_super_classes=cfg.num_super_classes, num_geometric=cfg.num_geometric,
                                       num_possessive=cfg.num_possessive, num_semantic=cfg.num_semantic)
    else:
        m = FlatRelationClassifier(cfg.args(), input_dim=cfg.hidden_dim, output_dim=cfg.num_relations, feature_size=cfg.feature_size,
                                   num_classes=cfg.num_classes, num_super_classes=cfg.num_super_classes)
    m = m.cuda()
    m.load_state_dict(sd)
    m.eval()
    return m


def _union_mask(batch, F):
    """[B,F,F] bool: the union of every image's boxes (the reference's own mask build)."""
    from oracle import relhead_oracle as O
    return torch.stack([O.build_masks(b, F).any(dim=0) if int(b.shape[0]) else torch.zeros(F, F, dtype=torch.bool) for b in batch.bbox])


def _assert_zero_outside(g, batch, F):
    outside = ~_union_mask(batch, F)
    assert bool(outside.any())                                              # the scene leaves pixels uncovered
    vals = g.detach().cpu().permute(1, 0, 2, 3)[:, outside]
    assert bool((vals == 0).all()), "gradient outside the union of the image's boxes"
    assert bool((g.detach().cpu().permute(1, 0, 2, 3)[:, ~outside] != 0).any())


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def _dgrad_operands(n_img, seed):
    g = torch.Generator().manual_seed(seed)
    n_pix = n_img * 1024
    dpre = [torch.randn(n_pix, 128, generator=g) for _ in (0, 1)]
    zero = torch.rand(n_pix, generator=g) < 0.3                             # rows where both roles' gradient is zero
    zero[:40] = True                                                        # a whole 32-pixel tile among them
    wt = []
    for r in (0, 1):
        dpre[r][zero] = 0
        w = torch.zeros(CP, 128)
        w[:257] = torch.randn(257, 128, generator=g)
        wt.append(w.to(torch.bfloat16).cuda())
    return [d.to(torch.bfloat16).cuda() for d in dpre], wt, zero


def _run_dgrad(lib, dp, wt, roles, C0, C1, n_img, accumulate, prefill):
    """Outputs allocated inside one larger sentinel-filled buffer: (out [n_img,257,1024] view order (out0 | out1), whole buffer, spans)."""
    from scene_graph_commonsense_amd import _lib
    n0, n1, guard = n_img * C0 * 1024, n_img * C1 * 1024, 4096
    buf = torch.full((guard + n0 + guard + n1 + guard,), SENTINEL, dtype=torch.float32, device="cuda")
    o0 = buf[guard:guard + n0]
    o1 = buf[2 * guard + n0:2 * guard + n0 + n1] if C1 else None
    if prefill is not None:
        o0.copy_(prefill[:, :C0].reshape(-1))
        if C1:
            o1.copy_(prefill[:, C0:].reshape(-1))
    a = (dp[0], wt[0]) if 0 in roles else (None, None)
    b = (dp[1], wt[1]) if 1 in roles else (None, None)
    st = lib.sgc_conv1_dgrad(_lib.ptr(a[0]), _lib.ptr(a[1]), _lib.ptr(b[0]), _lib.ptr(b[1]), _lib.ptr(o0), C0, _lib.ptr(o1), C1, n_img, 1024,
                             int(accumulate), _lib.stream_ptr())
    assert st == 0, st
    torch.cuda.synchronize()
    out = torch.cat([o0.view(n_img, C0, 1024)] + ([o1.view(n_img, C1, 1024)] if C1 else []), dim=1)
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[guard:guard + n0] = True
    if C1:
        inside[2 * guard + n0:2 * guard + n0 + n1] = True
    assert bool((buf[~inside] == SENTINEL).all()), "a store outside [n_img][C][HW] (padded channels 257..CP-1?)"
    return out


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("split", [(256, 1), (257, 0)])
@pytest.mark.parametrize("roles", [(0, 1), (0,), (1,)])
@pytest.mark.parametrize("n_img", [1, 3])
def test_conv1_dgrad_kernel_matches_float64(n_img, roles, split, accumulate):
    from scene_graph_commonsense_amd import _lib
    lib = _lib.load()
    dp, wt, zero = _dgrad_operands(n_img, seed=100 + n_img)
    C0, C1 = split
    prefill = torch.randn(n_img, 257, 1024, generator=torch.Generator().manual_seed(5)).cuda() if accumulate else None
    out = _run_dgrad(lib, dp, wt, roles, C0, C1, n_img, accumulate, prefill)
    ref = torch.zeros(n_img * 1024, 257, dtype=torch.float64, device="cuda")
    mag = torch.zeros_like(ref)
    for r in roles:                                                          # float64 on the very bf16 values the kernel reads
        ref += dp[r].double() @ wt[r][:257].double().t()
        mag += dp[r].double().abs() @ wt[r][:257].double().abs().t()
    ref = ref.view(n_img, 1024, 257).permute(0, 2, 1)
    mag = mag.view(n_img, 1024, 257).permute(0, 2, 1)
    got = out.double() - (prefill.double() if accumulate else 0)
    worst = float(((got - ref).abs() / mag.clamp(min=1e-300)).max())
    print("conv1_dgrad n_img=%d roles=%s split=%s accumulate=%d: worst |err| / sum|w.dpre| = %.2e" % (n_img, roles, split, accumulate, worst))
    assert bool(((got - ref).abs() <= 4e-5 * mag).all()), worst              # 256 f32 additions at one ulp (2^-23) each
    zr = zero.view(n_img, 1024).cuda()[:, None, :].expand(n_img, 257, 1024)
    assert bool((out[zr] == (prefill[zr] if accumulate else 0.0)).all())      # zero rows of dpre: exactly 0.0 (nothing added)
    again = _run_dgrad(lib, dp, wt, roles, C0, C1, n_img, accumulate, prefill)
    assert torch.equal(out, again)                                            # two runs: identical bits


def test_conv1_dgrad_refuses_bad_arguments():
    from scene_graph_commonsense_amd import _lib
    lib = _lib.load()
    dp, wt, _ = _dgrad_operands(1, seed=3)
    o0, o1 = torch.zeros(257 * 1024, device="cuda"), torch.zeros(1024, device="cuda")
    P, st = _lib.ptr, _lib.stream_ptr()
    call = lambda *a: lib.sgc_conv1_dgrad(*a, st)
    assert call(P(None), P(None), P(None), P(None), P(o0), 257, P(None), 0, 1, 1024, 0) == 1       # no role
    assert call(P(dp[0]), P(None), P(None), P(None), P(o0), 257, P(None), 0, 1, 1024, 0) == 1      # half a role
    assert call(P(dp[0]), P(wt[0]), P(None), P(None), P(o0), 256, P(None), 0, 1, 1024, 0) == 1     # C0 + C1 != 257
    assert call(P(dp[0]), P(wt[0]), P(None), P(None), P(o0), 256, P(None), 1, 1, 1024, 0) == 1     # C1 without out1
    assert call(P(dp[0]), P(wt[0]), P(None), P(None), P(o0), 257, P(o1), 0, 1, 1024, 0) == 1       # out1 without C1
    assert call(P(dp[0]), P(wt[0]), P(None), P(None), P(o0), 257, P(None), 0, 1, 1000, 0) == 1     # HW no multiple of 32
    assert call(P(dp[0]), P(wt[0]), P(None), P(None), P(o0), 257, P(None), 0, -1, 1024, 0) == 1
    torch.cuda.synchronize()
    assert bool((o0 == 0).all())


# ------------------------------------------------------------------------------------------------ 2. / 3. fused path against the oracle
_ORACLE = {}


def _fused_case(size, kind):
    """(cfg, sd, batch, oracle loss, oracle d loss / d image_feature, d loss / d image_depth): computed once, shared, never modified."""
    key = (size, kind)
    if key not in _ORACLE:
        from oracle import relhead_oracle as O
        from scene_graph_commonsense_amd.synthetic import HeadConfig, make_scene_batch, make_state_dict, predicate_counts
        kw = dict(hierarchical=(kind == "hier"))
        if size == "small":
            kw.update(hidden_dim=16, feature_size=8)
        cfg = HeadConfig(**kw)
        sd = make_state_dict(cfg, seed=21, head_gain=4.0)
        batch = make_scene_batch(cfg, (3, 2) if size == "fused" else (4, 3, 2), seed=21, connect_frac=0.6, edge_boxes=True)
        feat, depth = batch.image_feature.clone().requires_grad_(True), batch.image_depth.clone().requires_grad_(True)
        ob = dataclasses.replace(batch, image_feature=feat, image_depth=depth)
        out = O.run_pair_loop(sd, ob, cfg, mode="train", weights=O.class_weights(predicate_counts(cfg)))
        out["losses"].backward()
        _ORACLE[key] = (cfg, sd, batch, float(out["losses"].detach()), feat.grad.detach(), depth.grad.detach())
    return _ORACLE[key]


def _fused_against_oracle(size, kind):
    from scene_graph_commonsense_amd.pair_loop import train_minibatch
    cfg, sd, batch, ref_loss, ref_feat, ref_depth = _fused_case(size, kind)
    model = _model(cfg, sd)
    loss = train_minibatch(model, batch, None, input_grads=True)
    torch.cuda.synchronize()
    assert abs(float(loss) - ref_loss) <= 2e-3 * abs(ref_loss)
    ig = model.last_input_grads
    C2, F, B = 2 * cfg.hidden_dim, cfg.feature_size, len(batch.bbox)
    assert tuple(ig["image_feature"].shape) == (B, C2, F, F) and tuple(ig["image_depth"].shape) == (B, 1, F, F)
    assert ig["image_feature"].dtype == torch.float32 and ig["image_feature_aug"] is None
    _check_bar((size, kind, "image_feature"), ig["image_feature"], ref_feat)
    _check_bar((size, kind, "image_depth"), ig["image_depth"], ref_depth)
    _assert_zero_outside(ig["image_feature"], batch, F)
    _assert_zero_outside(ig["image_depth"], batch, F)


@pytest.mark.oracle_heavy
@pytest.mark.parametrize("kind", ["hier", "flat"])
def test_fused_input_grads_match_oracle_default_sizes(kind):
    _fused_against_oracle("fused", kind)


@pytest.mark.parametrize("kind", ["hier", "flat"])
def test_fused_input_grads_match_oracle_small_sizes(kind):
    from scene_graph_commonsense_amd.engine_generic import GenericTrunkEngine
    cfg, sd = _fused_case("small", kind)[:2]
    assert isinstance(_model(cfg, sd).engine(), GenericTrunkEngine)
    _fused_against_oracle("small", kind)


# ------------------------------------------------------------------------------------------------ 4. oracle-free identity
def _bf16_of_f16(t):
    return t.half().to(torch.bfloat16).double()                # what the packed input is when the weight gradient reads it


def _conv1_identity(model, feats, depth, grads):
    """sum dX . x_b  against  sum_r sum W1_r,b . dW1_r  over the 257 real channels, and the bound 1e-4 |dX| |x_b|."""
    lhs, nx, ng = 0.0, 0.0, 0.0
    for x, g in list(zip(feats, grads[:-1])) + [(depth, grads[-1])]:
        xb, gd = _bf16_of_f16(x.cuda()), g.double()
        lhs += float((gd * xb).sum())
        nx += float(xb.pow(2).sum())
        ng += float(gd.pow(2).sum())
    rhs = sum(float((c.weight.detach().to(torch.bfloat16).double() * c.weight.grad.double()).sum()) for c in (model.conv1_1, model.conv1_2))
    return lhs, rhs, 1e-4 * ng ** 0.5 * nx ** 0.5


def test_input_grads_and_conv1_weight_grads_of_one_call_agree():
    from scene_graph_commonsense_amd.pair_loop import train_minibatch
    from scene_graph_commonsense_amd.synthetic import HeadConfig, make_scene_batch, make_state_dict
    cfg = HeadConfig()
    model = _model(cfg, make_state_dict(cfg, seed=4, head_gain=4.0))
    batch = make_scene_batch(cfg, (6, 5), seed=23, connect_frac=0.5)
    train_minibatch(model, batch, None, input_grads=True)
    torch.cuda.synchronize()
    ig = model.last_input_grads
    lhs, rhs, bound = _conv1_identity(model, [batch.image_feature], batch.image_depth, [ig["image_feature"], ig["image_depth"]])
    print("conv1 identity: sum dX.x = %.6e, sum W.dW = %.6e, |diff| = %.2e, bound = %.2e" % (lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs) > 0 and abs(lhs - rhs) <= bound


# ------------------------------------------------------------------------------------------------ 5. nothing else moves
def test_switch_changes_neither_loss_nor_parameter_gradients():
    from scene_graph_commonsense_amd.pair_loop import train_minibatch
    cfg, sd, batch = _small_default_case()
    model = _model(cfg, sd)
    res = []
    for on in (False, True):
        model.zero_grad(set_to_none=True)
        loss = train_minibatch(model, batch, None, input_grads=on) if on else train_minibatch(model, batch, None)
        torch.cuda.synchronize()
        res.append((loss.clone(), {n: p.grad.clone() for n, p in model.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0])
    for n in res[0][1]:
        assert torch.equal(res[0][1][n], res[1][1][n]), n
    assert model.last_input_grads is not None and float(model.last_input_grads["image_feature"].abs().max()) > 0


def _small_default_case():
    from scene_graph_commonsense_amd.synthetic import HeadConfig, make_scene_batch, make_state_dict
    cfg = HeadConfig()
    return cfg, make_state_dict(cfg, seed=21, head_gain=4.0), make_scene_batch(cfg, (3, 2), seed=21, connect_frac=0.6, edge_boxes=True)


# ------------------------------------------------------------------------------------------------ 6. image groups
def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-30))


def test_image_groups_and_lanes_write_their_image_slices():
    from scene_graph_commonsense_amd.pair_loop import train_minibatch
    from scene_graph_commonsense_amd.synthetic import HeadConfig, make_scene_batch, make_state_dict
    cfg = HeadConfig()
    model = _model(cfg, make_state_dict(cfg, seed=21, head_gain=4.0))
    batch = make_scene_batch(cfg, (4, 1, 3), seed=29, connect_frac=0.6)            # the middle image has no pair
    runs = {}
    for name, kw in (("one", dict(workspace_budget=1e15)), ("groups", dict(workspace_budget=1.0)), ("lanes", dict(workspace_budget=1e15, streams=2))):
        model.zero_grad(set_to_none=True)
        train_minibatch(model, batch, None, input_grads=True, **kw)
        torch.cuda.synchronize()
        runs[name] = (list(model.last_image_groups), {k: (None if v is None else v.clone()) for k, v in model.last_input_grads.items()})
    assert len(runs["one"][0]) == 1 and len(runs["groups"][0]) >= 2 and len(runs["lanes"][0]) >= 2
    one = runs["one"][1]
    assert float(one["image_feature"][0].abs().max()) > 0 and float(one["image_feature"][2].abs().max()) > 0
    assert float(one["image_feature"][1].abs().max()) == 0 and float(one["image_depth"][1].abs().max()) == 0      # image without pairs: zeros
    for name in ("groups", "lanes"):
        for k in ("image_feature", "image_depth"):
            e = _rel(runs[name][1][k], one[k])
            print("input grads, %s vs one pass, %s: %.2e" % (name, k, e))
            assert e <= 2e-4, (name, k, e)          # tests/test_chunking_gpu.py: the one-pass step up to f32 summation order
            assert float(runs[name][1][k][1].abs().max()) == 0


def _depth_identity(share, depth, conv1_grads):
    """Channel 256 of the conv1 identity, which holds per input channel: sum dDepth . depth_b  against  sum_r sum_k W1_r,b[k,256] dW1_r[k,256]
    for ONE backward pass (its depth gradient, its conv1 weight gradients), and the bound 1e-4 |dDepth| |depth_b|."""
    db = _bf16_of_f16(depth.cuda())
    lhs = float((share.double() * db).sum())
    rhs = sum(float((w.detach().to(torch.bfloat16).double().reshape(128, 257)[:, 256] * g.double().reshape(128, 257)[:, 256]).sum())
              for w, g in conv1_grads)
    return lhs, rhs, 1e-4 * float(share.double().norm()) * float(db.norm())


def test_image_groups_with_the_augmented_view():
    from scene_graph_commonsense_amd.engine import RelHeadEngine
    from scene_graph_commonsense_amd.pair_loop import train_minibatch
    from scene_graph_commonsense_amd.synthetic import HeadConfig, hash_normal, make_scene_batch, make_state_dict
    cfg = HeadConfig()
    model = _model(cfg, make_state_dict(cfg, seed=21, head_gain=4.0))
    batch = make_scene_batch(cfg, (4, 3), seed=31, connect_frac=0.6)
    f = batch.image_feature
    aug = (0.9 * f + 0.3 * torch.from_numpy(hash_normal(4242, f.numel()).reshape(f.shape))).cuda()
    # the one-pass run is watched: after each of its two backward passes (main trunk, augmented trunk) the depth gradient as it stands
    # and that pass's own conv1 weight gradients are copied
    passes = []
    orig = RelHeadEngine.train_backward

    def spy(self, *a, **k):
        loss, grads = orig(self, *a, **k)
        torch.cuda.synchronize()
        passes.append((k["input_grads"]["depth"].clone(), [grads["conv1_%d.weight" % r].clone() for r in (1, 2)]))
        return loss, grads

    runs = {}
    for name, budget in (("one", 1e15), ("groups", 1.0)):
        model.zero_grad(set_to_none=True)
        if name == "one":
            RelHeadEngine.train_backward = spy
        try:
            train_minibatch(model, batch, None, input_grads=True, workspace_budget=budget, image_feature_aug=aug, lambda_contrast=0.7)
        finally:
            RelHeadEngine.train_backward = orig
        torch.cuda.synchronize()
        runs[name] = (list(model.last_image_groups), {k: v.clone() for k, v in model.last_input_grads.items()},
                      {n: p.grad.clone() for n, p in model.named_parameters()})
    assert len(runs["one"][0]) == 1 and len(runs["groups"][0]) == 2
    one, many = runs["one"][1], runs["groups"][1]
    g_aug = one["image_feature_aug"]
    assert g_aug is not None and tuple(g_aug.shape) == tuple(f.shape) and bool(torch.isfinite(g_aug).all())
    _assert_zero_outside(g_aug, batch, cfg.feature_size)
    for k in ("image_feature", "image_depth", "image_feature_aug"):
        e = _rel(many[k], one[k])
        print("input grads with the augmented view, groups vs one pass, %s: %.2e" % (k, e))
        assert e <= 1e-4, (k, e)                   # tests/test_chunking_gpu.py: the bar of the conv1 gradients with the coupled terms
    # the depth gradient is the sum of both trunks.  What the main pass left and what the augmented pass added to it are each held
    # against that pass's OWN conv1 weight gradients (channel 256 of the identity of test 4), so a depth gradient that lacks one of
    # them - overwritten instead of accumulated, or never added - misses its check (asserted below: by far more than the bound)
    assert len(passes) == 2
    weights = (model.conv1_1.weight, model.conv1_2.weight)
    main_share, total = passes[0][0], passes[1][0]
    assert torch.equal(total, one["image_depth"])
    checks = {}
    for name, share, dws in (("main", main_share, passes[0][1]), ("augmented", total - main_share, passes[1][1])):
        lhs, rhs, bound = _depth_identity(share, batch.image_depth, list(zip(weights, dws)))
        print("depth gradient, %s trunk's share: sum dDepth.depth = %.6e, sum W.dW (channel 256) = %.6e, |diff| %.2e, bound %.2e"
              % (name, lhs, rhs, abs(lhs - rhs), bound))
        assert abs(lhs - rhs) <= bound, name
        checks[name] = (abs(rhs), bound)
    # power of the two checks (measured: main 3.18e-02 against a bound of 1.2e-04, augmented 1.57e-04 against 7.0e-07).  Without the
    # augmented trunk's addition its check would compare 0 with its share; with the main share overwritten, "total - main" would carry
    # minus the main share into the augmented check, whose bound then is about the main check's
    (main_abs, main_bound), (aug_abs, aug_bound) = checks["main"], checks["augmented"]
    assert aug_abs > 10 * aug_bound and main_abs > 10 * (main_bound + aug_bound), checks
    # and the identity over all 257 channels and both views, against the summed weight gradients the step left in .grad
    for p_, g_ in zip(model.parameters(), runs["one"][2].values()):
        p_.grad = g_
    lhs, rhs, bound = _conv1_identity(model, [batch.image_feature, aug], batch.image_depth, [one["image_feature"], g_aug, one["image_depth"]])
    print("conv1 identity over both views: %.6e vs %.6e, |diff| %.2e, bound %.2e" % (lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound


# ------------------------------------------------------------------------------------------------ 7. per-step node
@pytest.mark.parametrize("size", ["default", "small"])
def test_per_step_node_returns_input_gradients(size):
    from oracle import relhead_oracle as O
    from scene_graph_commonsense_amd.synthetic import HeadConfig, make_state_dict
    cfg = HeadConfig() if size == "default" else HeadConfig(hidden_dim=16, feature_size=8)
    b = 2 if size == "default" else 3
    sd = make_state_dict(cfg, seed=21, head_gain=4.0)
    model = _model(cfg, sd)
    C, F = cfg.hidden_dim, cfg.feature_size
    g = torch.Generator().manual_seed(7)
    hs, ho = torch.randn(b, 2 * C + 1, F, F, generator=g), torch.randn(b, 2 * C + 1, F, F, generator=g)
    hs[:, :, :F // 4, :] = 0                                  # pre-masked crops: zero outside "boxes"
    ho[:, :, :, F // 2 + 1:] = 0
    c1, c2 = torch.randint(0, cfg.num_classes, (b,), generator=g), torch.randint(0, cfg.num_classes, (b,), generator=g)
    s1 = [torch.tensor([int(x) % cfg.num_super_classes]) for x in c1]
    s2 = [torch.tensor([int(x) % cfg.num_super_classes, (int(x) + 3) % cfg.num_super_classes]) for x in c2]
    rs, ro = hs.clone().requires_grad_(True), ho.clone().requires_grad_(True)
    ref_out = O.classifier_forward(sd, rs, ro, c1, c2, s1, s2, cfg.num_classes, cfg.num_super_classes, True)
    wts = [torch.randn(t.shape, generator=g) for t in ref_out]            # the loss: a fixed random projection of the returned tuple
    sum((t * w).sum() for t, w in zip(ref_out, wts)).backward()
    # the device: subject crops as a CUDA f32 leaf, object crops as a CPU f64 leaf - each gets its gradient in its dtype, on its device
    ds, do = hs.clone().cuda().requires_grad_(True), ho.clone().double().requires_grad_(True)
    out = model(ds, do, c1.cuda(), c2.cuda(), s1, s2, 0)
    sum((t * w.cuda()).sum() for t, w in zip(out[:6], wts)).backward()
    torch.cuda.synchronize()
    assert ds.grad is not None and ds.grad.is_cuda and ds.grad.dtype == torch.float32 and tuple(ds.grad.shape) == tuple(hs.shape)
    assert do.grad is not None and not do.grad.is_cuda and do.grad.dtype == torch.float64
    _check_bar(("step", size, "h_sub"), ds.grad, rs.grad)
    _check_bar(("step", size, "h_obj"), do.grad, ro.grad)
    # guard: an input that does not require grad still gets None, and the other one its gradient
    ds2, do2 = hs.clone().cuda().requires_grad_(True), ho.clone().cuda()
    model.zero_grad(set_to_none=True)
    out = model(ds2, do2, c1.cuda(), c2.cuda(), s1, s2, 0)
    sum((t * w.cuda()).sum() for t, w in zip(out[:6], wts)).backward()
    torch.cuda.synchronize()
    assert do2.grad is None and torch.equal(ds2.grad, ds.grad)


# ------------------------------------------------------------------------------------------------ 8. autograd bridge
def test_train_minibatch_drives_the_graph_that_produced_the_features():
    from scene_graph_commonsense_amd.pair_loop import train_minibatch
    cfg, sd, batch = _small_default_case()
    model = _model(cfg, sd)
    torch.manual_seed(11)
    conv = torch.nn.Conv2d(256, 256, 1).cuda()
    twin = torch.nn.Conv2d(256, 256, 1).cuda()
    twin.load_state_dict(conv.state_dict())
    base = batch.image_feature.cuda()
    feat = conv(base)
    assert feat.requires_grad
    train_minibatch(model, dataclasses.replace(batch, image_feature=feat), None, input_grads=True)
    torch.cuda.synchronize()
    g = model.last_input_grads["image_feature"]
    assert conv.weight.grad is not None and float(g.abs().max()) > 0
    twin(base).backward(g)
    torch.cuda.synchronize()
    torch.testing.assert_close(conv.weight.grad, twin.weight.grad, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(conv.bias.grad, twin.bias.grad, rtol=1e-5, atol=1e-6)
