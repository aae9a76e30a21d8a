"""Self-test of tests/step_glue_cases.py without a device: every definitional reference against an independent formulation - torch's
max_pool2d and float64 autograd, torch.optim.SGD, torch.as_strided, np.sum - so that a reference cannot be wrong the way its kernel is."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import shared_glue_cases as G
from tests import step_glue_cases as S

torch.set_grad_enabled(True)
M32 = S.window_major_rows(32)


def _maps(rows):
    """window-major rows [n, 1024, C] -> torch maps [n, C, 32, 32]."""
    return torch.from_numpy(np.ascontiguousarray(rows[:, M32].transpose(0, 3, 1, 2)))


def _codes_from_indices(val, idx, width):
    """torch max_pool2d indices (flat over the input map) -> routing codes dy 2 + dx, 4 where the pooled value is 0."""
    y, x = idx // width, idx % width
    return torch.where(val > 0, (y & 1) * 2 + (x & 1), torch.full_like(idx, 4))


def _tie_free(rng, shape):
    v = rng.permutation(int(np.prod(shape))).astype(np.float64).reshape(shape)
    return (v - v.mean()) / 64.0                                           # all distinct, exact in float64, both signs


def _expand_case(seed=1, n=4, C=6):
    rng = np.random.default_rng(seed)
    U = _tie_free(rng, (n, 1024, C))
    V = _tie_free(rng, (n, 1024, C)) * 2.0 + 1.0 / 256                     # u + v distinct within a window with overwhelming margin
    sub, obj = np.array([0, 0, 1, 2, 3, 3, 2]), np.array([1, 2, 0, 3, 0, 2, 1])
    return U, V, sub, obj


def test_window_major_rows_are_the_documented_order():
    for Sz in (16, 32):
        m = S.window_major_rows(Sz)
        assert sorted(m.reshape(-1).tolist()) == list(range(Sz * Sz))
        for Y, X, dy, dx in ((0, 0, 0, 0), (3, 5, 1, 0), (Sz // 2 - 1, Sz // 2 - 1, 1, 1)):
            assert m[2 * Y + dy, 2 * X + dx] == 4 * (Y * (Sz // 2) + X) + dy * 2 + dx
    Y, X = np.mgrid[0:16, 0:16]
    assert np.array_equal(S.window_major_rows(16), G.pixel_row(Y, X))
    assert np.array_equal(S.pack_nibbles(np.array([1, 4, 0, 3])), np.array([0x41, 0x30], dtype=np.uint8))


def test_expansion_reference_equals_max_pool2d_of_relu():
    U, V, sub, obj = _expand_case()
    mu, mv = _maps(U), _maps(V)
    for i, j in zip(sub, obj):
        z, code = S.expand_reference(U[i].reshape(256, 4, -1), V[j].reshape(256, 4, -1))
        s = U[i].reshape(256, 4, -1) + V[j].reshape(256, 4, -1)
        top = np.sort(s, axis=1)
        assert (top[:, 3] > top[:, 2]).all()                               # tie-free
        val, idx = F.max_pool2d(torch.relu(mu[i] + mv[j])[None], 2, return_indices=True)
        want_code = _codes_from_indices(val, idx, 32)[0].numpy()           # [C, 16, 16]
        assert np.array_equal(z.reshape(16, 16, -1).transpose(2, 0, 1), val[0].numpy())
        assert np.array_equal(code.reshape(16, 16, -1).transpose(2, 0, 1), want_code)
        assert (code == 4).any() and all((code == q).any() for q in range(4))


def test_expansion_reference_on_the_planted_ties_and_zeros():
    for regime in ("exact", "real"):
        U, V = S.expand_operands(np.random.default_rng(2), 3, 16, regime)
        assert np.array_equal(U.astype(np.float16).astype(np.float64), U) and np.array_equal(V.astype(np.float16).astype(np.float64), V)
        s32 = U.astype(np.float32)[:, None] + V.astype(np.float32)[None]
        assert np.array_equal(s32.astype(np.float64), U[:, None] + V[None])          # every sum exact in f32
        for i in range(3):
            for j in range(3):
                z, code = S.expand_reference(U[i].reshape(256, 4, -1), V[j].reshape(256, 4, -1))
                assert (code[:, 0] == 0).all() and (z[:, 0] > 0).all()               # four-way tie: the first
                assert (code[:, 1] == 1).all() and (code[:, 6] == 0).all()           # two-way ties: the first of the two
                assert (code[:, 2:6] == 4).all() and (z[:, 2:6] == 0).all()          # negative, +0 and -0 sums: nothing wins
                assert not np.signbit(z[:, 2:6]).any()
                assert (code[:, 7] == 2).all() or (z[:, 7] == 0).all()
        assert np.signbit(U[..., 4]).all() and np.signbit(V[..., 5]).all()


def test_contraction_reference_equals_autograd_of_the_expansion():
    U, V, sub, obj = _expand_case(seed=3)
    rng = np.random.default_rng(4)
    P, C = len(sub), U.shape[-1]
    dz = rng.standard_normal((P, 16, 16, C))
    codes = np.stack([S.expand_reference(U[i].reshape(256, 4, -1), V[j].reshape(256, 4, -1))[1].reshape(16, 16, C) for i, j in zip(sub, obj)])
    mu, mv = _maps(U).requires_grad_(True), _maps(V).requires_grad_(True)
    loss = 0
    for p in range(P):
        z = F.max_pool2d(torch.relu(mu[sub[p]] + mv[obj[p]])[None], 2)[0]
        loss = loss + (z * torch.from_numpy(dz[p].transpose(2, 0, 1))).sum()
    loss.backward()
    for index, grad in ((sub, mu.grad), (obj, mv.grad)):
        ptr, lst = G.csr(index, 4)
        ref, mag, cnt = S.contract_step_reference(dz, codes, ptr, lst)
        # [n, 16, 16, 4, C] -> [n, C, 32, 32]: slot q = dy 2 + dx of window (Y, X) is pixel (2 Y + dy, 2 X + dx)
        full = ref.reshape(4, 16, 16, 2, 2, C).transpose(0, 5, 1, 3, 2, 4).reshape(4, C, 32, 32)
        assert np.allclose(full, grad.numpy(), rtol=0, atol=1e-12)
        assert (cnt.reshape(-1) == np.bincount(index, minlength=4)).all() and (mag >= np.abs(ref) - 1e-12).all()


def test_contraction_lists_cover_every_arm_of_the_loop():
    ptr, lst = S.contract_lists(np.random.default_rng(5))
    cnt = np.diff(ptr).tolist()
    assert {0, 1, 3, 4, 5, 8, 9, 13} <= set(cnt) and len(cnt) == 12
    assert {c % 4 for c in cnt} == {0, 1, 2, 3} and len(set(lst.tolist())) < len(lst)       # pairs shared between lists
    for o in range(12):
        assert len(set(lst[ptr[o]:ptr[o + 1]].tolist())) == cnt[o]


def test_unpool_reference_equals_autograd_of_pool_of_relu():
    rng = np.random.default_rng(6)
    C = 5
    c = torch.from_numpy(_tie_free(rng, (3, C, 16, 16))).requires_grad_(True)
    val, idx = F.max_pool2d(torch.relu(c), 2, return_indices=True)
    dy = rng.standard_normal((3, C, 8, 8))
    (val * torch.from_numpy(dy)).sum().backward()
    code = _codes_from_indices(val, idx, 16).numpy().transpose(0, 2, 3, 1).reshape(3 * 64, C).astype(np.uint8)
    routed = G.unpool(dy.transpose(0, 2, 3, 1).reshape(3 * 64, C), code)               # [192, 4, C]
    full = routed.reshape(3, 8, 8, 2, 2, C).transpose(0, 5, 1, 3, 2, 4).reshape(3, C, 16, 16)
    assert np.array_equal(full, c.grad.numpy()) and (code == 4).any()
    parts = S.unpool_bias_parts(routed.sum(1), 7)
    assert np.allclose(parts.sum(0), c.grad.numpy().sum((0, 2, 3)), rtol=0, atol=1e-12)


def test_mask_references_equal_where_and_its_autograd():
    bb, ptr, obj_img = S.mask_scene()
    assert np.diff(ptr).tolist() == [4, 0, 3]
    ins = S.box_mask(bb)
    assert ins[0].all() and not ins[1].any() and ins[2].sum() == 1
    assert ins[3][0, 0] and ins[4][31, 31] and ins[5][0, 31] and ins[6][31, 0] and (ins[4] & ins[5]).any()      # every corner, an overlap
    rng = np.random.default_rng(7)
    D, F_ = 8, 32
    a = torch.from_numpy(rng.standard_normal((3, F_, F_, D))).requires_grad_(True)
    cst = torch.from_numpy(rng.standard_normal(D)).requires_grad_(True)
    m = torch.from_numpy(ins)[..., None]
    pad = torch.where(m, a[torch.from_numpy(obj_img).long()], cst.expand(len(bb), F_, F_, D))
    ref = S.mask_forward_reference(a.detach().numpy().reshape(-1, D), obj_img, bb, cst.detach().numpy())
    assert np.array_equal(ref[:, 1:33, 1:33], pad.detach().numpy())
    border = ref.copy()
    border[:, 1:33, 1:33] = 0
    assert (border == 0).all()
    da = rng.standard_normal((len(bb), F_, F_, D))                                       # by (y, x)
    (pad * torch.from_numpy(da)).sum().backward()
    da_rows = np.zeros((len(bb), F_ * F_, D))
    da_rows[:, M32.reshape(-1)] = da.reshape(len(bb), -1, D)                             # window-major, as conv2's data gradient leaves it
    dA, magA, part, magp = S.mask_backward_reference(da_rows, ptr, bb)
    assert np.allclose(dA.reshape(3, F_, F_, D), a.grad.numpy(), rtol=0, atol=1e-12)
    assert np.allclose(part.sum(0), cst.grad.numpy(), rtol=0, atol=1e-11) and part.shape == (3 * 64, D)
    assert (dA[1] == 0).all() and (part[64:128] == 0).all()                               # the image without objects
    out = np.where(ins.reshape(len(bb), -1, 1), 0.0, da.reshape(len(bb), -1, D))
    assert np.allclose(part[5], out[:4, 80:96].sum((0, 1)), rtol=0, atol=1e-12)          # block 5 of image 0: pixels 80 .. 95


def test_sgd_reference_equals_torch_optim_sgd_over_three_steps():
    rng = np.random.default_rng(8)
    lr, mom, wd = 0.05, 0.9, 1e-2
    w0 = rng.standard_normal(33)
    wt = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.SGD([wt], lr=lr, momentum=mom, weight_decay=wd, dampening=0)
    w, buf = w0.copy(), np.zeros(33)
    for step in range(3):
        g = rng.standard_normal(33)
        wt.grad = torch.from_numpy(g.copy())
        opt.step()
        w, buf, mw, mb = S.sgd_reference(w, g, buf, lr, mom, wd, step == 0)
        assert np.allclose(w, wt.detach().numpy(), rtol=0, atol=1e-14)
        assert np.allclose(buf, opt.state[wt]["momentum_buffer"].numpy(), rtol=0, atol=1e-14)
        assert (mw >= np.abs(w) - 1e-14).all() and (mb >= np.abs(buf) - 1e-14).all()


def _head_autograd(case, hier, cs, extra, scale):
    """float64 autograd of the forward formulas on the case's pre-activations: returns everything head_loss_reference takes and gives."""
    n = len(case["conn"])
    pre = torch.from_numpy(case["p"].copy()).requires_grad_(True)
    hidden = torch.relu(pre) * scale
    W = torch.from_numpy(case["W"])
    logits = hidden @ W.T * 8.0                                                   # [n, 64]
    logits.retain_grad()
    T = 1.0 / case["invT"]
    seg = torch.from_numpy(S.SEG)
    tgt = case["tgt"]
    if hier:
        sup = F.log_softmax(logits[:, S.R:S.R + 3], dim=1)
        rel = torch.cat([F.log_softmax(logits[:, :S.R][:, seg == k] / T[k], dim=1) + sup[:, k:k + 1] for k in range(3)], dim=1)
        cn = logits[:, S.R + 3]
    else:
        rel, sup, cn = logits[:, :S.R], torch.zeros(n, 3, dtype=torch.float64), logits[:, S.R]
    y = torch.from_numpy(case["y"])
    loss = torch.from_numpy(case["c"]) * F.binary_cross_entropy_with_logits(cn, y, reduction="none")
    loss = torch.where(torch.from_numpy(case["c"]) != 0, loss, torch.zeros_like(loss))
    rows = []
    for i in range(n):
        li = loss[i]
        t = int(tgt[i])
        if t >= 0 and hier:
            li = li - case["a"][i] * sup[i, S.SEG[t]] - case["b"][i] * rel[i, t]
        if t >= 0 and not hier:
            li = li - case["b"][i] * F.log_softmax(rel[i], dim=0)[t]
        if cs:
            for k in range(3 if hier else 1):
                blk = logits[i, :S.R][seg == k] / T[k] if hier else logits[i, :S.R]
                li = li + case["cs_coef"][i, k] * torch.softmax(blk, dim=0).max()
        rows.append(li)
    per_pair = torch.stack(rows)
    total = per_pair.sum()
    if extra:
        total = total + (hidden * torch.from_numpy(case["dp_extra"])).sum()
    total.backward()
    return rel.detach().numpy(), sup.detach().numpy(), cn.detach().numpy(), hidden.detach().numpy(), per_pair.detach().numpy(), \
        logits.grad.numpy(), pre.grad.numpy()


def _candidates(rel, hier):
    if not hier:
        return rel.max(1, keepdims=True), rel.argmax(1)[:, None]
    off = [0, S.NG, S.NG + S.NP]
    return (np.stack([rel[:, S.SEG == k].max(1) for k in range(3)], 1), np.stack([rel[:, S.SEG == k].argmax(1) + off[k] for k in range(3)], 1))


def test_head_loss_reference_equals_float64_autograd_of_the_forward_formulas():
    for hier in (1, 0):
        for cs in (False, True):
            for extra, scale in ((False, 1.0), (True, 2.0)):
                case = S.head_case(np.random.default_rng(9 + hier), 9, hier)
                assert {int(S.SEG[t]) for t in case["tgt"] if t >= 0} == {0, 1, 2} and (case["tgt"] == -1).any() and (case["c"] == 0).any()
                rel, sup, cn, hidden, loss_t, dl_t, dpre_t = _head_autograd(case, hier, cs, extra, scale)
                cc, cp = _candidates(rel, hier)
                loss, dl, dpre, e_dpre, e_loss, e_dl = S.head_loss_reference(
                    rel, sup, cn, hidden, case["tgt"], case["a"], case["b"], case["c"], case["y"], case["W"] * 8.0, hier, case["invT"], scale,
                    case["dp_extra"] if extra else None, case["cs_coef"] if cs else None, cc, cp)
                assert np.allclose(loss, loss_t, rtol=1e-12, atol=1e-12), (hier, cs)
                assert np.allclose(dl, dl_t, rtol=1e-11, atol=1e-12), (hier, cs)
                assert np.allclose(dpre, dpre_t, rtol=1e-11, atol=1e-12), (hier, cs, extra)
                assert (dpre[case["p"] <= 0] == 0).all() and (case["p"] == 0).any() and (case["p"] < 0).any()
                assert (e_dl >= 0).all() and (e_dpre >= 0).all() and (e_loss >= 0).all() and (dl[:, (S.R + 4 if hier else S.R + 1):] == 0).all()


def test_head_forward_outputs_equal_the_oracle_head():
    from oracle import relhead_oracle as O
    rng = np.random.default_rng(10)
    p = torch.from_numpy(rng.standard_normal((6, 512)))
    W = torch.from_numpy(rng.standard_normal((64, 512)) * 0.1)
    sd = {"fc3_1.weight": W[:S.NG], "fc3_2.weight": W[S.NG:S.NG + S.NP], "fc3_3.weight": W[S.NG + S.NP:S.R], "fc5.weight": W[S.R:S.R + 3]}
    sd.update({k.replace("weight", "bias"): torch.zeros(len(v), dtype=torch.float64) for k, v in list(sd.items())})
    T = (1.0, 1.5, 0.75)
    r1, r2, r3, sup = O.bayes_head(sd, p, T)
    logits = (p @ W.T).numpy()
    rel, sup2 = S.head_forward_outputs(logits[:, :S.R], logits[:, S.R:S.R + 3], T)
    assert np.allclose(rel, torch.cat([r1, r2, r3], 1).numpy(), rtol=0, atol=1e-12) and np.allclose(sup2, sup.numpy(), rtol=0, atol=1e-12)


def test_head_upstream_reference_equals_float64_autograd():
    rng = np.random.default_rng(11)
    for hier in (1, 0):
        for given in ((1, 1, 1), (0, 0, 0), (1, 0, 1), (0, 1, 0)):
            case = S.head_case(rng, 6, hier)
            n = 6
            pre = torch.from_numpy(case["p"].copy()).requires_grad_(True)
            hidden = torch.relu(pre) * 2.0
            logits = hidden @ torch.from_numpy(case["W"]).T * 8.0
            logits.retain_grad()
            T = 1.0 / case["invT"]
            seg = torch.from_numpy(S.SEG)
            if hier:
                sup = F.log_softmax(logits[:, S.R:S.R + 3], dim=1)
                rel = torch.cat([F.log_softmax(logits[:, :S.R][:, seg == k] / T[k], dim=1) + sup[:, k:k + 1] for k in range(3)], dim=1)
                cn = logits[:, S.R + 3]
            else:
                rel, sup, cn = logits[:, :S.R], torch.zeros(n, 3, dtype=torch.float64), logits[:, S.R]
            g_rel = rng.standard_normal((n, S.R))
            g_sup = rng.standard_normal((n, 3)) if given[0] and hier else None
            g_conn = rng.standard_normal(n) if given[1] else None
            g_hid = rng.standard_normal((n, 512)) if given[2] else None
            total = (rel * torch.from_numpy(g_rel)).sum()
            if g_sup is not None:
                total = total + (sup * torch.from_numpy(g_sup)).sum()
            if g_conn is not None:
                total = total + (cn * torch.from_numpy(g_conn)).sum()
            if g_hid is not None:
                total = total + (hidden * torch.from_numpy(g_hid)).sum()
            total.backward()
            dl, dpre, e_dpre, e_dl = S.head_upstream_reference(rel.detach().numpy(), sup.detach().numpy(), hidden.detach().numpy(), g_rel, g_sup,
                                                               g_conn, g_hid, case["W"] * 8.0, hier, case["invT"], 2.0)
            assert np.allclose(dl, logits.grad.numpy(), rtol=1e-11, atol=1e-12), (hier, given)
            assert np.allclose(dpre, pre.grad.numpy(), rtol=1e-11, atol=1e-12), (hier, given)


def test_head_wgrad_reference_is_the_chunked_outer_product():
    rng = np.random.default_rng(12)
    dl, p = rng.standard_normal((130, 64)), rng.standard_normal((130, 512))
    for chunk in (1, 64, 200):
        part, mag = S.head_wgrad_reference(dl, p, chunk)
        assert part.shape[0] == -(-130 // chunk)
        assert np.allclose(part.sum(0)[:, :512], np.einsum("pr,pk->rk", dl, p), rtol=0, atol=1e-11)
        assert np.allclose(part.sum(0)[:, 512], dl.sum(0), rtol=0, atol=1e-12)
        assert np.allclose(part[1 % part.shape[0]][:, :512], dl[chunk * (1 % part.shape[0]):][:chunk].T @ p[chunk * (1 % part.shape[0]):][:chunk], atol=1e-11)


def _np_strided(src, off, dims, strides):
    """numpy's as_strided from element ``off`` (negative strides allowed, which torch.as_strided refuses)."""
    base = src[off:]
    return np.lib.stride_tricks.as_strided(base, shape=dims, strides=[s * src.itemsize for s in strides])


def test_layout_references_equal_as_strided():
    rng = np.random.default_rng(13)
    src = rng.standard_normal(2 * 65536)
    for sa_s, sb_s, ss_i, sa_d, sb_d, ds_j in ((65536, 64, 1024, 65536, 4096, 64), (65536, 4096, 64, 65536, 64, 1024)):
        pos, val = S.transpose_cast_reference(src, 2 * 65536, 2, 3, sa_s, sb_s, ss_i, sa_d, sb_d, ds_j)
        got = np.zeros(2 * 65536)
        got[pos] = val
        want = torch.zeros(2 * 65536, dtype=torch.float64)
        torch.as_strided(want, (2, 3, 64, 64), (sa_d, sb_d, ds_j, 1)).copy_(torch.as_strided(torch.from_numpy(src), (2, 3, 64, 64), (sa_s, sb_s, 1, ss_i)))
        assert np.array_equal(got, want.numpy())
    # a flipped 3 x 3 kernel: stride -1 from offset 8, and a permutation of the leading dimensions
    w = rng.standard_normal(4 * 5 * 9)
    pos, val = S.scatter_reference(w, 7 + 5 * 4 * 9, (5, 4, 9), (9, 45, -1), (36, 9, 1), src_off=8, dst_off=7)
    want = np.ascontiguousarray(w.reshape(4, 5, 3, 3)[:, :, ::-1, ::-1].transpose(1, 0, 2, 3)).reshape(-1)
    assert np.array_equal(pos, 7 + np.arange(180)) and np.array_equal(val, want)
    assert np.array_equal(val, _np_strided(w, 8, (5, 4, 9), (9, 45, -1)).reshape(-1))
    for nd in range(1, 6):
        dims = (2, 3, 4, 5, 6)[:nd]
        n = int(np.prod(dims))
        srcn = rng.standard_normal(n + 3)
        sstr = np.cumprod((1,) + dims[:-1]).tolist()                                    # the source walks the dimensions the other way round
        dstr = (np.cumprod((1,) + dims[::-1][:-1])[::-1] * 2).tolist()                  # destination: row-major with every second element
        pos, val = S.scatter_reference(srcn, 2 * n + 1, dims, sstr, dstr, src_off=3, dst_off=1)
        want = torch.as_strided(torch.from_numpy(srcn), dims, sstr, 3).contiguous().view(-1).numpy()
        assert np.array_equal(val, want) and np.array_equal(pos, 1 + 2 * np.arange(n))
    mat = rng.standard_normal(40 * 30)
    pos, val = S.segment_cast_reference(mat, 4000, 5, 6, 30, 1, [0, 100, 1000], [6, 7, 50], [0, 7, 300])
    for s, (do, ld, so) in enumerate(((0, 6, 0), (100, 7, 7), (1000, 50, 300))):
        want = torch.as_strided(torch.from_numpy(mat), (5, 6), (30, 1), so).numpy()
        k = slice(30 * s, 30 * s + 30)
        assert np.array_equal(val[k].reshape(5, 6), want)
        assert np.array_equal(pos[k].reshape(5, 6), do + np.arange(5)[:, None] * ld + np.arange(6)[None])


def test_reduction_references_equal_np_sum():
    rng = np.random.default_rng(14)
    x = rng.standard_normal((9, 257))
    s, m, n = S.slab_sum_reference(x)
    assert np.allclose(s, np.sum(x, axis=0), rtol=0, atol=1e-13) and n == 9 and (m >= np.abs(s) - 1e-13).all()
    s2, _, n2 = S.slab_sum_reference(x, old=x[0])
    assert np.allclose(s2, np.sum(x, axis=0) + x[0], rtol=0, atol=1e-13) and n2 == 10
    X = rng.standard_normal((9, 16))
    for rb in (1, 3, 12):
        part, mag, r = S.colsum_reference(X, rb)
        assert part.shape == (rb, 16) and np.allclose(part.sum(0), np.sum(X, axis=0), rtol=0, atol=1e-13)
        assert (part[-(-9 // r):] == 0).all()
    part, _, r = S.colsum_reference(X, 3)
    assert r == 3 and np.allclose(part[1], np.sum(X[3:6], axis=0), rtol=0, atol=1e-13)
    ptr, lst = np.array([0, 0, 1, 3, 5]), np.array([2, 0, 2, 1, 1])
    out, mag, n = S.segment_sum_reference(X, ptr, lst)
    assert (out[0] == 0).all() and np.array_equal(out[1], X[2]) and np.allclose(out[2], X[0] + X[2]) and np.allclose(out[3], 2 * X[1])
    f0, f1 = rng.standard_normal((2, 3, 64)), rng.standard_normal((2, 1, 64))
    x = S.pack_image_reference(f0, f1, 8)
    want = torch.cat([torch.from_numpy(f0), torch.from_numpy(f1)], dim=1).permute(0, 2, 1).reshape(128, 4).numpy()
    assert np.array_equal(x[:, :4], want) and (x[:, 4:] == 0).all()
    t, dA = np.array([0.0, 0.25, -0.5, 1.0]), np.array([3.0, 16.0, -7.0, 5.0])
    tt = torch.from_numpy(np.arctanh(np.clip(t, -0.999999, 0.999999))).requires_grad_(True)
    (torch.tanh(tt) * torch.from_numpy(dA)).sum().backward()
    assert np.allclose(S.tanh_bwd_reference(dA, t)[:3], tt.grad.numpy()[:3], rtol=1e-9, atol=0) and S.tanh_bwd_reference(dA, t)[3] == 0


def test_expand_scene_holds_the_cases_the_list_kernel_branches_on():
    sc = S.ExpandScene()
    assert np.diff(sc.img_ptr).tolist() == [70, 0, 17] and sc.P == 200 + 272
    pairs0 = {(int(i), int(j)) for i, j in zip(sc.sub, sc.obj) if i < 70}
    assert len(pairs0) == 200
    assert {0, 7, 8, 63, 64, 69} <= {i for i, _ in pairs0} and {0, 15, 16, 31, 63, 64, 69} <= {j for _, j in pairs0}
    assert 33 not in {i for i, _ in pairs0} and (sc.pid[33] == -1).all()
    assert all(sc.pid[i, i] == -1 for i in range(70)) and all(sc.pid[70 + i, i] == -1 for i in range(17))
    assert (np.sort(sc.pid[sc.pid >= 0]) == np.arange(sc.P)).all()
    tiles_of_chunk1 = {j // 16 for i, j in pairs0 if i >= 64}
    assert tiles_of_chunk1 == {0, 4}                                        # tiles 1 .. 3: the second chunk has nothing live
    lv = sc.chunk_liveness(0)
    assert (lv[1] & ~lv[0]).any() and (lv[0] & ~lv[1]).any() and (~lv[0] & ~lv[1]).any()
    kinds = set(sc.pixrect.tolist())
    assert 0 in kinds and G.FULL_PIXRECT in kinds and S.pack_pixels(15, 16, 15, 16) in kinds and S.pack_pixels(0, 12, 3, 4) in kinds
    assert sc.live.sum((1, 2)).min() == 0 and sc.live.sum((1, 2)).max() == 256 and (sc.live.sum((1, 2)) == 1).any()
    few = [(W, t) for t in range(5) for W in range(256)
           if 0 < sum(sc.live[p, W >> 4, W & 15] for p in range(200) if sc.obj[p] // 16 == t) < 8]
    assert few                                                              # fewer than eight live items: wavefronts with an empty eighth
