"""Self-test of tests/shared_glue_cases.py without a device: the definitional references against independent evaluations in int64 /
float64, the rounding helpers against torch's casts, and the properties the box sets must have."""
import numpy as np
import torch

from tests import shared_glue_cases as G


def test_rne_helpers_equal_the_casts_of_torch_on_10000_values_with_halves():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4000) * 10.0 ** rng.integers(-9, 5, 4000), rng.integers(-65000, 65000, 3000).astype(np.float64),
                        rng.integers(-8192, 8192, 2000) + 0.5, rng.integers(-600, 600, 995) * 2.0 ** -25, [0.0, 65504.0, 65519.0, 2.0 ** -24, 2.0 ** -25]])
    x = np.asarray(x, dtype=np.float32).astype(np.float64)                    # f32 values, as the kernels' accumulators are
    assert len(x) == 10000
    for fmt, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        want = torch.from_numpy(x).float().to(dt)
        got = G.rne(x, fmt)
        ok = torch.isfinite(want).numpy()
        assert ok.all()
        assert np.array_equal(got[ok], want.double().numpy()[ok]), fmt
        wbits = want.view(torch.int16).numpy().view(np.uint16)[ok]
        assert np.array_equal(G.to_bits(got[ok], fmt), wbits & np.where(want.double().numpy()[ok] == 0, 0x7FFF, 0xFFFF))        # -0 counts as +0
        assert np.array_equal(G.from_bits(G.to_bits(got[ok], fmt), fmt), got[ok] + 0.0)
    assert G.rne(np.array([257.0, 258.0, 259.0, 261.0]), "bf16").tolist() == [256.0, 258.0, 260.0, 260.0]      # halves go to even
    assert G.rne(np.array([2049.0, 2051.0, 4098.0, 4102.0]), "f16").tolist() == [2048.0, 2052.0, 4096.0, 4104.0]
    assert G.rounding_cases(np.array([256.0, 257.0, 258.5, 3.0]), "bf16") == (2, 1)
    x32 = rng.standard_normal(1000) * 1e3
    assert np.array_equal(G.rne(x32, "f32"), x32.astype(np.float32).astype(np.float64))


def test_box_sets_hold_every_kind_of_box_and_pair():
    sc = G.base_scene()
    assert sc.n_img == 3 and np.diff(sc.img_ptr).tolist() == [6, 0, 5] and sc.n <= 12
    lin, conv, none = sc.kinds()
    assert lin > 0 and conv > 0 and none > 0, (lin, conv, none)
    ins = sc.inside.sum(1).tolist()
    assert ins[0] == 64 and ins[1] == 1 and ins[2] == 1 and ins[3] == 0 and ins[4] == 0 and ins[5] == 16      # full, corners, empty, reversed, strip
    assert sc.R[10].tolist() == [6, 8, 6, 8]                                                              # the stop beyond the grid is clamped
    assert (sc.R[6] == sc.R[7]).all() and sc.xmask[list(zip(sc.sub, sc.obj)).index((6, 7))].sum() == 9     # identical boxes
    p = list(zip(sc.sub, sc.obj)).index((6, 9))
    assert sc.linear[p] and sc.cnt_all[p] == 6                                                            # windows meet, D16 rectangles do not
    sub = G.base_scene(subset=True)
    pairs = list(zip(sub.sub.tolist(), sub.obj.tolist()))
    assert len(pairs) < sc.P and len(set(pairs)) == len(pairs) - 1                                        # a subset with one duplicate
    f2 = G.Scene(G.FULL2_IMAGES)
    assert f2.cnt_all.max() == 64 and f2.cnt_all.min() == 0
    for s in (G.gsum_groups_scene(), G.gsum_groups_scene(swap=True)):
        assert np.diff(s.img_ptr).tolist() == [0, 1, 8, 9, 17]
    ptr, _ = G.csr(G.gsum_groups_scene().sub, 35)
    assert np.diff(ptr)[18:22].tolist() == [16, 15, 1, 17]
    ptr, _ = G.csr(G.gsum_groups_scene(swap=True).obj, 35)
    assert np.diff(ptr)[18:22].tolist() == [16, 15, 1, 17]
    ls = G.linear_scene()
    assert ls.linear.all() and ls.E_lin == 6 * ls.P
    keys = ls.obj_img[ls.sub[ls.gather_lin >> 6]] * 64 + (ls.gather_lin & 63)
    assert sorted(set(np.bincount(keys, minlength=64 * ls.n_img).tolist())) == [0, 1, 3, 4, 5, 16, 17, 65, 70]
    lo = G.linear_objects_scene()
    assert lo.linear[:71].all() and 0 < lo.linear[71:].sum() < lo.P - 71


def test_fc1_reference_equals_the_inclusion_exclusion_expression_in_int64():
    rng = np.random.default_rng(1)
    for sc in (G.base_scene(), G.base_scene(subset=True), G.Scene(G.FULL2_IMAGES)):
        C = 8
        own = rng.integers(-50, 50, (sc.n2, 64, C))
        bg = rng.integers(-50, 50, (sc.n_img, 64, C))
        T = G.pseudo_rows(sc, own, bg)
        xp = rng.integers(-50, 50, (sc.E_all, C))
        bias = rng.integers(-9, 9, C)
        pre, mag, nx = G.fc1_reference(sc, T.astype(np.float64), xp.astype(np.float64), bias.astype(np.float64))
        assert np.array_equal(pre.astype(np.int64), G.fc1_inclusion_exclusion(sc, T.astype(np.int64), xp.astype(np.int64), bias.astype(np.int64)))
        assert (mag >= np.abs(pre)).all() and nx.tolist() == sc.cnt_all.tolist()
        # the background row is what a pseudo-pair uses outside R_o - and only there
        for ps in range(sc.n2):
            o = ps % sc.n
            assert np.array_equal(T[ps][~sc.inside[o]], bg[sc.obj_img[o]][~sc.inside[o]]) and np.array_equal(T[ps][sc.inside[o]], own[ps][sc.inside[o]])
        own_sum, _ = G.own_rect_reference(sc, T)
        S, _ = G.integral_reference(T)
        assert np.array_equal(own_sum, np.stack([G.rect_sum(S[sc.n + j], sc.R[j]) + 0 * S[0, 0, 0] for j in range(sc.n)]))
        assert not own_sum[3].any() and not own_sum[4].any() or sc.n != 11


def test_gradient_sum_reference_is_the_transpose_of_the_copy_matrix():
    rng = np.random.default_rng(2)
    for sc in (G.base_scene(), G.base_scene(subset=True), G.gsum_groups_scene()):
        dh = rng.integers(-20, 20, (sc.P, 4)).astype(np.float64)
        Gs, A, N, BG, BA, BN = G.gsum_reference(sc, dh)
        M = G.copy_matrix(sc)
        assert np.array_equal(Gs, np.einsum("psw,pc->swc", M, dh))
        assert np.array_equal(N[:, :, 0], M.sum(0))
        # forward / backward adjointness: <assembly(T), dh> = <T, G>, with the background rows folded in
        T = rng.integers(-5, 5, (sc.n2, 64, 4)).astype(np.float64)
        lhs = (np.einsum("psw,swc->pc", M, T) * dh).sum()
        assert lhs == (T * Gs).sum()
        want = np.zeros_like(BG)
        for i in range(sc.n):
            want[sc.obj_img[i]] += np.where(sc.inside[i][:, None], 0.0, Gs[i])
        assert np.array_equal(BG, want)
        assert not (M[:, sc.n:] * ~np.tile(sc.inside, (1, 1))[None]).any()                     # role 1 never copies outside R_o


def test_linear_reference_equals_a_direct_convolution_of_the_combined_map():
    """2-channel toy: three 16 x 16 input maps, z_ij = z_(i,bg) + z_(bg,j) - z_(bg,bg); conv3 (3 x 3, padded) is linear, so the
    combination of the three pre-activations equals the pre-activation of the combined map; then bias, ReLU, 2 x 2 max."""
    rng = np.random.default_rng(3)
    Cin, Cout = 2, 2
    w3 = rng.integers(-3, 4, (Cout, Cin, 3, 3)).astype(np.float64)
    z = rng.integers(-4, 5, (3, 18, 18, Cin)).astype(np.float64)
    z[:, [0, 17]] = 0
    z[:, :, [0, 17]] = 0

    def conv(m):                                              # [18, 18, Cin] -> [64 windows, 4 pixels, Cout]
        out = np.zeros((64, 4, Cout))
        for w in range(64):
            for q in range(4):
                y, x = 2 * (w >> 3) + (q >> 1), 2 * (w & 7) + (q & 1)
                out[w, q] = np.einsum("ocyx,yxc->o", w3, m[y:y + 3, x:x + 3])
        return out

    sc = G.Scene([[G.LIN_A, G.LIN_B]])
    assert sc.linear.all() and sc.P == 2
    a, b, g = conv(z[0]), conv(z[1]), conv(z[2])
    pre_own = np.zeros((4, 64, 4, Cout))
    pre_own[0], pre_own[3] = a, b                                       # (o = 0, bg) and (bg, o = 1): what the pair (0, 1) combines
    pre_bg = g[None]
    ps, w = np.nonzero(sc.obj_entry >= 0)
    raw_own = np.zeros((sc.E_obj, 4, Cout))
    raw_own[sc.obj_entry[ps, w]] = pre_own[ps, w]
    pre, mag, used_own, used_bg = G.linear_pre_reference(sc, raw_own, pre_bg)
    assert used_bg.sum() == 6 and used_own.sum() == 24
    direct = conv(z[0] + z[1] - z[2])
    w = sc.gather_lin[:6] & 63
    assert np.array_equal(pre[:6], direct[w])                              # pair (0, 1): subject 0's (o, bg) + object 1's (bg, o)
    assert (mag >= np.abs(pre)).all()
    bias = np.array([1.0, -2.0])
    v, code = G.pool_reference(pre, bias)
    want = np.maximum(direct[w].max(1) + bias, 0)
    assert np.array_equal(v[:6], want)
    tie = np.array([[[5.0], [7.0], [7.0], [1.0]], [[-3.0], [-3.0], [-3.0], [-3.0]]])
    v, code = G.pool_reference(tie, np.array([0.0]))
    assert v[:, 0].tolist() == [7.0, 0.0] and code[:, 0].tolist() == [1, 4]
    assert G.unpool(np.array([[2.0, 3.0]]), np.array([[1, 4]]))[0].tolist() == [[0, 0], [2, 0], [0, 0], [0, 0]]


def test_patch_and_contraction_references_on_hand_made_cases():
    sc = G.Scene([[G.CORNER_LO, G.FULL]])
    assert sc.cnt_conv.tolist() == [1, 1]
    V = np.arange(16, dtype=np.float64).reshape(1, 16, 1) + 1
    dz, mag, cnt = G.patch_sum_reference(sc, V, np.abs(V), sc.incl_conv, sc.gather_conv, 0, 1)
    # window (0, 0): patch pixel (py, px) is pixel (py - 1, px - 1); row / column 0 of the patch fall off the map
    assert dz[0, :3, :3, 0].tolist() == [[6, 7, 8], [10, 11, 12], [14, 15, 16]] and dz[0].sum() == sum([6, 7, 8, 10, 11, 12, 14, 15, 16])
    assert cnt[0, 0, 0, 0] == 2 and cnt[0, 2, 2, 0] == 1
    assert G.PATCH_ROW20 == [0, 1, 2, 3, 4, 5, 7, 9, 10, 11, 13, 15, 16, 17, 18, 19]
    assert [G.pixel_row(0, 0), G.pixel_row(0, 1), G.pixel_row(1, 0), G.pixel_row(2, 0), G.pixel_row(15, 15)] == [0, 1, 2, 32, 255]
    # contraction: object 0 (corner) as subject: its one real pair and its pseudo-pair, inside the pseudo-pair's pixel rectangle only
    n_pairs = sc.P + sc.n2 + 1
    rng = np.random.default_rng(4)
    dzv = rng.integers(-5, 6, (n_pairs, 16, 16, 2)).astype(np.float64)
    codes = rng.integers(0, 5, (n_pairs, 16, 16, 2))
    pix = np.concatenate([sc.pixrect_conv, sc.pixrect_obj, [G.FULL_PIXRECT]])
    dU, mag, cnt = G.contract_reference(sc, 0, dzv, codes, pix, 1)
    assert not dU[0, 3:].any() and not dU[0, :, 3:].any()                  # the corner's rectangle: pixels 0..2
    k = [int(np.nonzero(sc.sub == 0)[0][0]), sc.P + 0]
    for q in range(4):
        assert np.array_equal(dU[0, 1, 1, q], sum(np.where(codes[p, 1, 1] == q, dzv[p, 1, 1], 0) for p in k))
    want = sum(np.where(codes[p, 9, 9] == 2, dzv[p, 9, 9], 0) for p in (sc.P + 3, sc.P + 4))
    assert np.array_equal(dU[2, 9, 9, 2], want) and cnt[2, 9, 9, 0, 0] == 2   # background as subject: the (bg, o) pseudo-pairs that exist there + its map


def test_row_tables_of_the_two_spaces_are_consistent():
    for sc in (G.base_scene(), G.base_scene(subset=True), G.many_objects_scene()):
        for name, sp in sc.spaces.items():
            used = np.concatenate([sp["prow"], sp["dest"][:sc.E_all]])
            assert used.min() >= 0 and used.max() < sp["rows"]
            for w in range(64):
                rows = np.concatenate([sp["prow"][w::64], sp["dest"][:sc.E_all][(sc.gather_all[:sc.E_all] & 63) == w]])
                assert rows.min() >= sp["goff"][w] and rows.max() < sp["gend"][w] <= sp["goff"][w + 1]
                own = sp["prow"][w::64][np.tile(sc.inside[:, w], 2)] if name == "compact" else sp["prow"][w::64]
                x = sp["dest"][:sc.E_all][(sc.gather_all[:sc.E_all] & 63) == w]
                lead0 = sp["goff"][w] + (sc.n_img if name == "compact" else 0)
                assert np.array_equal(np.concatenate([own, x]), np.arange(lead0, sp["gend"][w]))             # every row named exactly once, in order
            assert np.array_equal(sp["dest"][sc.E_all:], sp["prow"].reshape(-1, 64)[np.tile(sc.inside, (2, 1))])
