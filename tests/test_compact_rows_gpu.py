"""The COMPACT window-major row space of the second sharing level (``TUNING.compact_object_rows``; csrc/kernels_shared.hip, "fc1 over
shared windows"): a pseudo-pair has rows only inside its window rectangle R_o, everywhere else fc1 and its backward use the background
row of the object's image.  Against the full layout (switch off):

  * the layout tables equal a NumPy restatement;
  * the forward is bit-identical (a row's product does not depend on its position, the prefix sums add the same f32 values in the same
    order);
  * the backward differs only where the gradient of a background row is now summed BEFORE the grouped GEMMs (f32 sum, one bf16
    rounding) instead of after them: every tensor that does not pass through that sum keeps its bits, the others stay inside the
    arithmetic bound against the oracle with the device's routes injected (``tests/test_backward_gpu.py``: 5e-3, 7e-3 below conv3).

Shapes: 2 images with 5 and 6 objects whose boxes include a full-image box (R_o = all 64 windows: no background row used), a box of
ONE window, an empty box (R_o empty: every row is a background row), two overlapping and two disjoint boxes; and 3 images x 2 objects
(more background rows than object rows in most groups).  Full-size model."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROUTED_TOL = 5e-3        # tests/test_backward_gpu.py: head, fc2, fc1, conv3 with the device's routes injected; 7e-3 below conv3

# x0, x1, y0, y1 on the 32-grid (slice semantics)
BOXES = {
    "mixed": ([5, 6], [[[0, 32, 0, 32], [31, 32, 31, 32], [10, 10, 4, 9], [12, 20, 12, 20], [14, 24, 10, 18]],
                       [[0, 6, 0, 6], [24, 32, 24, 32]]]),
    "bg_heavy": ([2, 2, 2], [[[3, 9, 20, 27]], [[0, 1, 0, 1], [9, 3, 5, 8]], []]),
}


def _tol(name):
    return 7e-3 if name.split(".")[0] in ("conv2_1", "conv1_1", "conv1_2") else ROUTED_TOL


@pytest.fixture(autouse=True)
def _always_shared(monkeypatch):
    """Full-image boxes next to tiny ones make many windows pair-specific; the shared path is the subject here."""
    from scene_graph_commonsense_amd import engine
    monkeypatch.setattr(engine.TUNING, "shared_max_fraction", 2.0)


def _case(name):
    from scene_graph_commonsense_amd.synthetic import HeadConfig, make_scene_batch, make_state_dict
    nobj, special = BOXES[name]
    cfg = HeadConfig()
    batch = make_scene_batch(cfg, nobj, seed=17, connect_frac=0.4)
    for b, rows in zip(batch.bbox, special):
        if rows:
            b[:len(rows)] = torch.tensor(rows).to(b.dtype)
    return cfg, make_state_dict(cfg, seed=3, head_gain=4.0), batch


_STEPS = {}


def _step(name, compact, keep_routes=False):
    """One training step of the case on the device (what tests/train_case.run_train_gpu does) with the switch on / off; keeps the
    window-major buffers of the backward.  Computed once per (case, switch)."""
    key = (name, compact)
    if key in _STEPS and (not keep_routes or _STEPS[key]["routes"] is not None):
        return _STEPS[key]
    from scene_graph_commonsense_amd import engine
    from scene_graph_commonsense_amd.engine import RelHeadEngine, csr_by, loss_coefficients
    from scene_graph_commonsense_amd.model import _shared_hint
    from scene_graph_commonsense_amd.pairs import flatten_scene, pair_targets
    from scene_graph_commonsense_amd.synthetic import predicate_counts
    from tests.train_case import device_routes
    cfg, sd, batch = _case(name)
    dev = "cuda:0"
    with engine.tuning(compact_object_rows=compact):
        eng = RelHeadEngine(cfg, dev)
        eng.load_weights(sd)
        eng.prep_bwd_weights(sd)
        sc = flatten_scene(cfg, batch, dev)
        pidx = sc.pidx
        directed, _ = pair_targets(batch.relationships, batch.subj_or_obj, pidx)
        counts = predicate_counts(cfg).numpy()
        coefs = loss_coefficients(cfg, pidx.step, len(pidx.call_sizes), directed, 1 - counts / counts.sum())
        coefs_d = tuple(torch.from_numpy(c).to(dev) for c in coefs)
        n_obj = int(sc.obj_img.shape[0])
        sub_csr = tuple(torch.from_numpy(a).to(dev) for a in csr_by(pidx.sub, n_obj))
        obj_csr = tuple(torch.from_numpy(a).to(dev) for a in csr_by(pidx.obj, n_obj))
        img_ptr = torch.from_numpy(pidx.obj_offset.astype(np.int32)).to(dev)
        P = sc.n_pairs
        # NaN bit patterns in what the backward writes row by row: a row nobody wrote shows up
        ctx = eng.train_forward(sc.image_feature, sc.image_depth, sc.obj_img, sc.bbox, sc.cats, sc.super_mh, sc.sub_idx, sc.obj_idx,
                                dropout=True, seeds=(11, 12), dense=(sc.img_ptr, sc.pid, sc.max_n), shared_windows=_shared_hint(sc))
        torch.cuda.synchronize()
        wm = ctx.shared["wm"]
        assert (wm["prow"] is not None) == compact
        routes = device_routes(ctx) if keep_routes else None
        fwd = dict(h1=ctx.h1[:P * 4096].clone(), p=ctx.p[:P * 512].clone())
        runs = []
        for _ in range(2):
            for nm in ("gwm", "dywm"):
                if nm in eng.scratch.bufs:
                    eng.scratch.bufs[nm].view(torch.int16).fill_(0x7FC0)
            loss, grads = eng.train_backward(ctx, coefs_d, sub_csr, obj_csr, img_ptr)
            torch.cuda.synchronize()
            runs.append((float(loss), {k: v.clone() for k, v in grads.items()}, eng.scratch.bufs["gwm"][:wm["rows"] * 4096].clone(),
                         eng.scratch.bufs["dywm"][:wm["rows"] * 1024].clone()))
        dh1 = eng.scratch.bufs["dh1"][:P * 4096].clone().view(P, 4096)
    out = dict(cfg=cfg, sd=sd, batch=batch, sc=sc, wm={k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in wm.items()}, fwd=fwd,
               runs=runs, dh1=dh1, routes=routes, bbox=sc.bbox.cpu().numpy(), obj_img=sc.obj_img.cpu().numpy(),
               sub=sc.sub_idx.cpu().numpy(), obj=sc.obj_idx.cpu().numpy(), n_img=len(batch.bbox), P=P,
               E_total=wm["E_total"], gather=ctx.shared.get("gather_all", ctx.shared["gather"])[:wm["E_total"]].cpu().numpy())
    _STEPS[key] = out
    return out


def _inside(bbox):
    """[n_obj, 64] bool: window w inside R_o (host replica of object_windows)."""
    from scene_graph_commonsense_amd.pairs import object_window_rects
    r = object_window_rects(bbox)
    wy, wx = np.divmod(np.arange(64), 8)
    return (wx[None] >= r[:, 0:1]) & (wx[None] < r[:, 1:2]) & (wy[None] >= r[:, 2:3]) & (wy[None] < r[:, 3:4])


@pytest.mark.parametrize("name", list(BOXES))
def test_layout_equals_the_numpy_restatement(name):
    s = _step(name, True)
    wm, inside, n_img = s["wm"], _inside(s["bbox"]), s["n_img"]
    n_obj = inside.shape[0]
    if name == "mixed":                        # the cases the boxes were chosen for
        sizes = inside.sum(1)
        assert 64 in sizes and 1 in sizes and 0 in sizes
        assert (inside[3] & inside[4]).any() and not (inside[5] & inside[6]).any()
    in2 = np.concatenate([inside, inside])                          # pseudo-pair ps = role * n_obj + o
    code = s["gather"]
    E = wm["E"]
    xcount = np.bincount(code[:E] & 63, minlength=64)
    lead = n_img + in2.sum(0)
    size = (lead + xcount + 255) // 256 * 256
    goff = np.concatenate([[0], np.cumsum(size)])
    assert np.array_equal(wm["goff"], goff) and wm["rows"] == goff[64]
    assert np.array_equal(wm["gend"], goff[:64] + lead + xcount)
    assert np.array_equal(wm["tile_group"], np.repeat(np.arange(64), size // 256))
    rank = np.cumsum(in2, 0) - in2                                    # pseudo-pairs in front with the window inside their rectangle
    img2 = np.concatenate([s["obj_img"], s["obj_img"]])
    want = np.where(in2, goff[None, :64] + n_img + rank, goff[None, :64] + img2[:, None])
    assert np.array_equal(wm["prow"].reshape(2 * n_obj, 64), want)
    # X entries: behind the per-object rows of their group in list order; the pseudo-pairs' own windows: their prow
    dest = wm["dest"]
    xw = code[:E] & 63
    order = np.argsort(xw, kind="stable")
    first = np.concatenate([[0], np.cumsum(xcount)[:-1]])
    want_x = np.empty(E, dtype=np.int64)
    want_x[order] = (goff[:64] + lead)[xw[order]] + np.arange(E) - first[xw[order]]
    assert np.array_equal(dest[:E], want_x)
    ps_code = code[E:] - 64 * s["P"]
    assert np.array_equal(dest[E:s["E_total"]], want.reshape(-1)[ps_code])
    assert in2.reshape(-1)[ps_code].all() and len(ps_code) == in2.sum()
    full = _step(name, False)["wm"]
    assert wm["rows"] <= full["rows"]
    print(name, "rows", wm["rows"], "against", full["rows"], "pseudo rows", int(in2.sum()), "of", in2.size)


@pytest.mark.parametrize("name", list(BOXES))
def test_forward_is_bit_identical_with_the_switch_on_and_off(name):
    from scene_graph_commonsense_amd import engine
    from scene_graph_commonsense_amd.model import BayesianRelationClassifier
    from scene_graph_commonsense_amd.pairs import flatten_scene
    on, off = _step(name, True), _step(name, False)
    for k in on["fwd"]:                                               # training forward (dropout on): h1 and fc2's output
        assert torch.equal(on["fwd"][k].view(torch.int16 if k == "h1" else torch.int32),
                           off["fwd"][k].view(torch.int16 if k == "h1" else torch.int32)), k
    assert on["runs"][0][0] == off["runs"][0][0]                    # the loss
    cfg, sd, batch = _case(name)
    model = BayesianRelationClassifier(cfg.args()).cuda()
    model.load_state_dict(sd)
    model.eval()
    sc = flatten_scene(cfg, batch, "cuda:0")
    eng = model.refresh_weights()
    outs = []
    for compact in (False, True):
        for nm in ("h1", "owm", "oxh", "fc1_S", "ywm"):
            for ws in (eng.ws, eng.scratch):
                if nm in ws.bufs:
                    ws.bufs[nm].view(torch.int16).fill_(0x7E00 if nm in ("h1", "ywm", "oxh") else -1)      # NaN bit patterns
        with engine.tuning(compact_object_rows=compact):
            o = model.forward_pairs(sc)
            torch.cuda.synchronize()
            outs.append((o, eng.ws.bufs["h1"][:sc.n_pairs * 4096].clone()))
    (a, ha), (b, hb) = outs
    assert torch.isfinite(hb.float()).all() and torch.equal(ha.view(torch.int16), hb.view(torch.int16))
    for f in ("relation", "super_relation", "connectivity", "hidden", "cand_conf", "cand_pred"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        if x is not None:
            assert torch.equal(x, y), f


@pytest.mark.parametrize("name", list(BOXES))
def test_backward_keeps_the_bits_outside_the_background_sum(name):
    """Bit-identical with the switch on and off: the gradients of the head (fc3_*, fc4, fc5), of fc2 and fc1.bias (all computed from
    dh1 and above), every row of gwm / dywm that is not a background row - the X rows and the pseudo-pairs' rows inside R_o.
    Re-associated: fc1.weight (the background rows' term), conv3_1 and everything below it (through the background maps)."""
    on, off = _step(name, True), _step(name, False)
    g_on, g_off = on["runs"][0][1], off["runs"][0][1]
    same = [n for n in g_on if not n.startswith(("fc1.weight", "conv"))]
    assert {"fc1.bias", "fc2.weight", "fc2.bias"} <= set(same) and len(same) >= 7
    for n in same:
        assert torch.equal(g_on[n], g_off[n]), n
    E = on["E_total"]
    d_on, d_off = torch.from_numpy(on["wm"]["dest"][:E]).long().cuda(), torch.from_numpy(off["wm"]["dest"][:E]).long().cuda()
    for k, width in ((2, 4096), (3, 1024)):                           # gwm, dywm
        a = on["runs"][0][k].view(-1, width).view(torch.int16)[d_on]
        b = off["runs"][0][k].view(-1, width).view(torch.int16)[d_off]
        assert torch.equal(a, b), ("gwm", "dywm")[k - 2]
    for n in g_on:
        if n not in same:
            ref = g_off[n].double()
            print(name, n, "on vs off %.2e" % float((g_on[n].double() - ref).norm() / ref.norm().clamp(min=1e-30)))


def test_reassociated_gradients_stay_inside_the_arithmetic_bound_of_the_oracle():
    """With the device's routes and dropout masks injected the oracle's gradients and the device's differ by arithmetic only: the bound
    of tests/test_backward_gpu.py / tests/test_training_mode_gpu.py, with the compact rows as with the full ones."""
    from tests.train_case import fro, oracle_train
    on, off = _step("mixed", True, keep_routes=True), _step("mixed", False)
    _, g_ref, _ = oracle_train(on["cfg"], on["sd"], on["batch"], on["sc"], dropout_seeds=(11, 12), routes=on["routes"])
    g_on, g_off = on["runs"][0][1], off["runs"][0][1]
    bad = []
    for n, ref in g_ref.items():
        e_on, e_off = fro(g_on[n].float().cpu(), ref), fro(g_off[n].float().cpu(), ref)
        d = fro(g_on[n].float().cpu(), g_off[n].float().cpu())
        print("%-16s oracle vs on %.2e  vs off %.2e  on vs off %.2e  bound %.0e" % (n, e_on, e_off, d, _tol(n)))
        if not e_on <= _tol(n):
            bad.append((n, e_on))
    assert not bad, bad


@pytest.mark.parametrize("name", list(BOXES))
def test_background_gradient_row_is_the_f32_sum_rounded_once(name):
    """gwm[goff[w] + b] = bf16(sum over the subjects i of image b with w outside R_i of G_i[w]), G_i[w] = the f32 sum of dh1 over the
    pairs (i, j) with w outside R_j - what sgc_fc1_gsum accumulates for (0, i, w) before it rounds.  The restatement adds the same bf16
    values in f32 in another order: apart by the one rounding to bf16 (half an ulp: 2^-8 relative) and by the f32 summation error of
    the n terms on both sides, (2n + 2) * 2^-23 of the sum of the magnitudes with room to spare."""
    s = _step(name, True)
    inside = torch.from_numpy(_inside(s["bbox"])).cuda()
    sub, obj = torch.from_numpy(s["sub"]).long().cuda(), torch.from_numpy(s["obj"]).long().cuda()
    img = torch.from_numpy(s["obj_img"]).long().cuda()
    dh = s["dh1"].float()
    goff = torch.from_numpy(s["wm"]["goff"][:64]).long().cuda()
    gwm = s["runs"][0][2].view(-1, 4096).float()
    mask = (~inside[sub] & ~inside[obj]).float()                      # [P, 64]: the pair's row feeds the background row of window w
    worst = 0.0
    for b in range(s["n_img"]):
        m = mask * (img[sub] == b).float()[:, None]
        want = m.t() @ dh                                              # [64, 4096] f32
        mag = m.t() @ dh.abs()
        got = gwm[goff + b]
        n = float(m.sum(0).max())
        bound = 2.0 ** -8 * want.abs() + (2 * n + 2) * 2.0 ** -23 * mag + 1e-38
        assert ((got - want).abs() <= bound).all(), (b, float(((got - want).abs() - bound).max()))
        worst = max(worst, float(((got - want).abs() / want.abs().clamp(min=1e-30))[want.abs() > 1e-20].max()) if (want.abs() > 1e-20).any() else 0.0)
    print(name, "worst relative distance %.2e (half a bf16 ulp: 3.9e-3)" % worst)


@pytest.mark.parametrize("name", list(BOXES))
def test_two_backward_runs_give_identical_bits(name):
    s = _step(name, True)
    (l0, g0, gwm0, dy0), (l1, g1, gwm1, dy1) = s["runs"]
    assert l0 == l1
    for n in g0:
        assert torch.isfinite(g0[n]).all(), n
        assert torch.equal(g0[n], g1[n]), n
    assert torch.equal(gwm0.view(torch.int16), gwm1.view(torch.int16)) and torch.equal(dy0.view(torch.int16), dy1.view(torch.int16))
