"""Definitional float64 / int64 references and case builders for the per-pair step kernels of csrc/kernels_fwd.hip and csrc/kernels_bwd.hip
(tests/test_step_glue_gpu.py runs the kernels, tests/test_step_glue_cases_cpu.py proves this file against independent formulations
without a device).  NumPy only; the number formats, the two regimes and the checking helpers are those of tests/shared_glue_cases.py.

One plain function per operation, written from the documentation of include/sgc_relhead.h: the expansion is max-pool(relu(U_i + V_j))
with the route of the first maximum, the contraction its transpose summed over an object's list, the un-pool the routed gradient, the
mask backward the sum over the objects whose box holds (does not hold) the pixel, SGD the three lines of torch.optim.SGD, the head
backward the derivative of  -a sup[st] - b rel[t] + c BCE(conn, y) + sum kappa max softmax  written out per logit."""
import numpy as np

from tests import shared_glue_cases as G

# ---------------------------------------------------------------------------------------------------------------- layouts
def window_major_rows(S):
    """[S, S] int: row m = 4 (Y (S/2) + X) + dy 2 + dx of pixel (y, x) = (2 Y + dy, 2 X + dx) of an S x S map."""
    y, x = np.mgrid[0:S, 0:S]
    return 4 * ((y >> 1) * (S >> 1) + (x >> 1)) + (y & 1) * 2 + (x & 1)


def pack_pixels(Y0, Y1, X0, X1):
    """A packed pixel rectangle given by its pixels (G.pack_pixrect dilates a WINDOW rectangle and cannot name one pixel)."""
    return Y0 | (Y1 << 5) | (X0 << 10) | (X1 << 15)


def pack_nibbles(codes):
    """[..., C] codes -> [..., C / 2] bytes: channel 2k in the low nibble, 2k + 1 in the high one."""
    codes = np.asarray(codes, dtype=np.uint8)
    return (codes[..., 0::2] | (codes[..., 1::2] << 4)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- 1. expansion
def expand_reference(Ui, Vj):
    """Ui, Vj [256 W, 4 q, C] (the four window-major rows 4 W + q of pixel W = 16 Y + X) -> (z [256, C] float64, code [256, C]):
    z = max(0, max_q(u + v)); code = the first q that attains the maximum, 4 when the maximum is not positive."""
    s = np.asarray(Ui, dtype=np.float64) + np.asarray(Vj, dtype=np.float64)
    m = s.max(axis=1)
    first = np.full(m.shape, 3, dtype=np.int64)
    for q in (2, 1, 0):
        first = np.where(s[:, q] == m, q, first)
    dead = ~(m > 0)
    return np.where(dead, 0.0, m), np.where(dead, 4, first).astype(np.uint8)


PLANT = 8          # channels 0 .. 7 of every window hold the planted cases


def plant_expand_cases(U, V):
    """U, V [n, 1024, C] float64 (window-major rows): channels 0 .. 7 of EVERY row are overwritten so that every pair and window has
    0 a four-way tie of a positive maximum, 1 a two-way tie (q = 1 and q = 3), 2 four negative sums, 3 u = -v (sums +0), 4 u = v = -0.0
    (sums -0), 5 u = +0, v = -0 (sums +0), 6 a two-way tie at q = 0 and q = 2 under a smaller positive, 7 one positive maximum at q = 2."""
    n = U.shape[0]
    q = np.tile(np.arange(4), 256)[None, :]                                  # q of every row
    o = (np.arange(n) % 5)[:, None].astype(np.float64)
    U[:, :, 0], V[:, :, 0] = 1.0 + o, 0.5 + 0 * o + 0 * q
    U[:, :, 1], V[:, :, 1] = np.where(q % 2 == 1, 2.0, -1.0) + 0 * o, 0.25 * (1 + o) + 0 * q
    U[:, :, 2], V[:, :, 2] = -1.0 - o - 0.125 * q, -0.5 - 0.25 * q + 0 * o
    U[:, :, 3], V[:, :, 3] = 1.5, -1.5
    U[:, :, 4], V[:, :, 4] = -0.0, -0.0
    U[:, :, 5], V[:, :, 5] = 0.0, -0.0
    U[:, :, 6], V[:, :, 6] = np.where(q % 2 == 0, 3.0, 1.0) + 0 * o, 0.5 * o + 0 * q
    U[:, :, 7], V[:, :, 7] = np.where(q == 2, 4.0, -4.0) + 0 * o, o - 2.0 + 0 * q
    return U, V


def expand_operands(rng, n, C, regime):
    """f16-representable U, V [n, 1024, C] whose every sum u + v is exact in f32.  EXACT: integers in [-12, 12]; REAL: sign x
    mantissa (11 bits) x 2**e with e in [-6, 3] (magnitudes in [2**-6, 2**4): the lowest bit of any operand is 2**-16, every sum is
    below 2**5 - 21 bits), one value in eight an exact zero.  Then the planted channels."""
    def draw():
        if regime == "exact":
            return rng.integers(-12, 13, (n, 1024, C)).astype(np.float64)
        mant = rng.integers(1024, 2048, (n, 1024, C)).astype(np.float64) / 1024.0
        v = mant * np.exp2(rng.integers(-6, 4, (n, 1024, C))) * rng.choice([-1.0, 1.0], (n, 1024, C))
        return np.where(rng.integers(0, 8, (n, 1024, C)) == 0, 0.0, v)
    return plant_expand_cases(draw(), draw())


SIGN = (PLANT, PLANT + 1)          # two more channels name the objects of a pair: z = subject index / object index, route = index % 4


def expand_scene_operands(rng, n, C, regime, pool=16):
    """U, V [n, 1024, C] float16 for a whole scene: object o takes map o % pool of ``expand_operands`` (a scene of 87 distinct random
    maps costs seconds to draw and adds nothing), and the two SIGN channels make every object's map its own: channel 8 of U_o is o at
    q = o % 4 and -1 elsewhere with V = 0, channel 9 of V_o likewise with U = 0 - a kernel that reads another object's rows shows there."""
    Up, Vp = expand_operands(rng, pool, C, regime)
    idx = np.arange(n) % pool
    U, V = Up.astype(np.float16)[idx], Vp.astype(np.float16)[idx]
    q = np.tile(np.arange(4), 256)[None, :]
    o = np.arange(n)[:, None]
    own = np.where(q == o % 4, o, -1).astype(np.float16)
    U[:, :, SIGN[0]], V[:, :, SIGN[0]] = own, 0
    U[:, :, SIGN[1]], V[:, :, SIGN[1]] = 0, own
    return U, V


class ExpandScene:
    """Three images of 70, 0 and 17 objects.  Image 0: about 200 ordered pairs - subjects 0, 7, 8, 63 with the objects 0, 5, 15, 16,
    31, 40, 47, 48, 63, 64, 69; subjects 64 and 69 (the second 64-subject chunk) with objects of the tiles 0 and 4 only (its other
    tiles: nothing live); random pairs of the other subjects; subject 33 has none; the diagonal is -1.  Image 2: every ordered pair.
    Pixel rectangles: full only for objects of the tiles 1 .. 3 of image 0 (where the second chunk has nothing); for the objects of
    tiles 0 and 4 the first chunk's rectangles lie in Y < 12 and the second chunk's in Y >= 4, so that for (pixels with Y >= 12, tile 0)
    only the second chunk is live and for (Y < 4, tile 0) only the first; single pixels, strips and 0 (none) everywhere."""
    SIZES = (70, 0, 17)
    MAX_N = 70

    def __init__(self, seed=31):
        rng = np.random.default_rng(seed)
        self.img_ptr = np.concatenate([[0], np.cumsum(self.SIZES)]).astype(np.int32)
        self.n = int(self.img_ptr[-1])
        pairs = []
        for i in (0, 7, 8, 63):
            pairs += [(i, j) for j in (0, 5, 15, 16, 31, 40, 47, 48, 63, 64, 69) if j != i]
        for i in (64, 69):
            pairs += [(i, j) for j in (0, 5, 15, 64, 66, 69) if j != i]
        seen = set(pairs)
        while len(pairs) < 200:
            i, j = int(rng.integers(1, 63)), int(rng.integers(0, 70))
            if i in (7, 8, 33) or i == j or (i, j) in seen:
                continue
            seen.add((i, j))
            pairs.append((i, j))
        order = rng.permutation(len(pairs))                                   # pair indices in no particular order
        pairs = [pairs[k] for k in order]
        o2 = int(self.img_ptr[2])
        pairs += [(o2 + i, o2 + j) for i in range(17) for j in range(17) if i != j]
        self.sub = np.array([p[0] for p in pairs], dtype=np.int32)
        self.obj = np.array([p[1] for p in pairs], dtype=np.int32)
        self.P = len(pairs)
        self.pid = np.full((self.n, self.MAX_N), -1, dtype=np.int32)         # [subject object][object index inside the image]
        img0 = np.searchsorted(self.img_ptr, self.sub, side="right") - 1
        self.pid[self.sub, self.obj - self.img_ptr[img0]] = np.arange(self.P)
        low = [G.pack_pixrect(0, 3, 0, 4), G.pack_pixrect(2, 6, 1, 5), pack_pixels(0, 12, 3, 4), pack_pixels(5, 6, 9, 10), 0,
               pack_pixels(0, 1, 0, 16), G.pack_pixrect(7, 8, 0, 1)]        # all inside Y < 12 (pack_pixrect(.., y0, y1) stops at 2 y1 + 1)
        high = [pack_pixels(4, 16, 0, 16), pack_pixels(15, 16, 15, 16), pack_pixels(12, 16, 7, 8), 0, G.pack_pixrect(3, 5, 6, 8)]
        anyr = low + high + [G.FULL_PIXRECT, G.pack_pixrect(3, 4, 0, 8)]
        rect = np.zeros(self.P, dtype=np.int32)
        for p, (i, j) in enumerate(pairs):
            if i >= o2:
                rect[p] = anyr[p % len(anyr)]
            elif 16 <= j < 64:
                rect[p] = G.FULL_PIXRECT if p % 3 == 0 else anyr[p % len(anyr)]
            else:
                rect[p] = (high if i >= 64 else low)[p % (len(high) if i >= 64 else len(low))]
        self.pixrect = rect
        self.live = np.stack([G.pixrect_mask(int(r)) for r in rect])          # [P, 16, 16]

    def chunk_liveness(self, tile):
        """[2, 16, 16] bool: some pair of image 0 with the subject in chunk c and the object in ``tile`` needs the pixel."""
        out = np.zeros((2, 16, 16), dtype=bool)
        for p in range(self.P):
            if self.sub[p] < 70 and self.obj[p] // 16 == tile:
                out[self.sub[p] // 64] |= self.live[p]
        return out


# ---------------------------------------------------------------------------------------------------------------- 2. contraction
def contract_lists(rng, n_obj=12, counts=(0, 1, 3, 4, 5, 8, 9, 13, 4, 0, 2, 7), n_pairs=16):
    """ptr / list of an object -> pairs CSR with the given list lengths; the pairs are drawn from one pool, so lists share them."""
    assert len(counts) == n_obj
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    lst = np.concatenate([rng.permutation(n_pairs)[:c] for c in counts]).astype(np.int32)
    return ptr, lst


def contract_step_reference(dz, codes, ptr, lst):
    """dU [n_obj, 16, 16, 4, C]: for pixel W = (Y, X) and slot q the sum, IN LIST ORDER, over the object's pairs of dz[p][Y][X] where
    the pair's route at W equals q.  dz, codes [P, 16, 16, C] by (Y, X).  Also the sums of |terms| and the list lengths."""
    n = len(ptr) - 1
    C = dz.shape[-1]
    dU, mag = np.zeros((n, 16, 16, 4, C)), np.zeros((n, 16, 16, 4, C))
    for o in range(n):
        for p in lst[ptr[o]:ptr[o + 1]]:
            r = G.unpool(dz[p], codes[p])
            dU[o] += r
            mag[o] += np.abs(r)
    return dU, mag, np.diff(ptr).astype(np.float64).reshape(n, 1, 1, 1, 1)


# ---------------------------------------------------------------------------------------------------------------- 3. un-pool
def unpool_bias_parts(routed, n_parts):
    """What block b of sgc_unpool_relu_bwd sums: the windows w = b 2 + s + k 2 n_parts; here only their float64 total per part
    (the test compares the SUM over parts with the column sum; the split into parts is not documented)."""
    n_win = routed.shape[0]
    parts = np.zeros((n_parts, routed.shape[-1]))
    for b in range(n_parts):
        idx = np.concatenate([np.arange(2 * b + s, n_win, 2 * n_parts) for s in (0, 1)])
        parts[b] = routed[idx].sum(0)
    return parts


# ---------------------------------------------------------------------------------------------------------------- 4. masks
# (x0, x1, y0, y1).  Image 0: the full map, an empty box (x0 == x1), one pixel, the top-left corner (all inside the full map: overlaps);
# image 1: no object; image 2: bottom-right and top-right corners that overlap in x 26..31, y 25..29, and the bottom-left corner
MASK_IMAGES = [[[0, 32, 0, 32], [10, 10, 4, 9], [5, 6, 7, 8], [0, 3, 0, 2]], [], [[20, 32, 25, 32], [26, 32, 0, 30], [0, 4, 28, 32]]]


def mask_scene():
    images = MASK_IMAGES
    bb = np.array([b for im in images for b in im], dtype=np.int32).reshape(-1, 4)
    ptr = np.concatenate([[0], np.cumsum([len(i) for i in images])]).astype(np.int32)
    return bb, ptr, np.repeat(np.arange(len(images)), np.diff(ptr)).astype(np.int32)


def box_mask(bb, F=32):
    """[n, F, F] bool (y, x): x0 <= x < x1 and y0 <= y < y1 (slice semantics)."""
    y, x = np.mgrid[0:F, 0:F]
    bb = np.asarray(bb).reshape(-1, 4, 1, 1)
    return (x[None] >= bb[:, 0]) & (x[None] < bb[:, 1]) & (y[None] >= bb[:, 2]) & (y[None] < bb[:, 3])


def mask_forward_reference(a_img, obj_img, bb, cst, F=32):
    """a_pad [n, F + 2, F + 2, D]: zero border; inside the box the image map (pixel-major rows y F + x), outside the constant."""
    n, D = len(bb), a_img.shape[-1]
    out = np.zeros((n, F + 2, F + 2, D), dtype=a_img.dtype)
    ins = box_mask(bb, F)
    maps = a_img.reshape(-1, F, F, D)
    for o in range(n):
        out[o, 1:F + 1, 1:F + 1] = np.where(ins[o][:, :, None], maps[obj_img[o]], cst[None, None, :])
    return out


def mask_backward_reference(da, img_ptr, bb, F=32):
    """da [n, F F, D] with WINDOW-MAJOR rows.  dA [n_img, F F, D] (pixel-major) = the sum in object order over the image's objects
    whose box holds the pixel; part [n_img * F F / 16, D]: part (img, block) = the sum over the block's 16 pixels, in pixel order, of
    the sums in object order over the objects whose box does NOT hold the pixel.  With the sums of |terms| and the term counts."""
    n_img, D = len(img_ptr) - 1, da.shape[-1]
    m = window_major_rows(F).reshape(-1)
    ins = box_mask(bb, F).reshape(len(bb), -1)
    dA, magA = np.zeros((n_img, F * F, D)), np.zeros((n_img, F * F, D))
    out, mago = np.zeros((n_img, F * F, D)), np.zeros((n_img, F * F, D))
    for b in range(n_img):
        for o in range(img_ptr[b], img_ptr[b + 1]):
            g = da[o][m]                                                       # pixel-major
            dA[b] += np.where(ins[o][:, None], g, 0.0)
            magA[b] += np.where(ins[o][:, None], np.abs(g), 0.0)
            out[b] += np.where(ins[o][:, None], 0.0, g)
            mago[b] += np.where(ins[o][:, None], 0.0, np.abs(g))
    part = np.zeros((n_img, F * F // 16, D))
    for k in range(16):
        part += out.reshape(n_img, -1, 16, D)[:, :, k]
    return dA, magA, part.reshape(-1, D), mago.reshape(n_img, -1, 16, D).sum(2).reshape(-1, D)


# ---------------------------------------------------------------------------------------------------------------- 5. element-wise
def tanh_bwd_reference(dA, t):
    """dpre = dA (1 - t^2)."""
    return dA * (1.0 - t * t)


def pack_image_reference(f0, f1, XC):
    """f0 [n_img, C0, HW], f1 [n_img, C1, HW] or None -> [n_img * HW, XC]: channels of f0, then of f1, then zeros."""
    parts = [f0] + ([f1] if f1 is not None else [])
    x = np.concatenate(parts, axis=1)
    n_img, C, HW = x.shape
    out = np.zeros((n_img, HW, XC))
    out[:, :, :C] = x.transpose(0, 2, 1)
    return out.reshape(n_img * HW, XC)


# ---------------------------------------------------------------------------------------------------------------- 6. reductions
def slab_sum_reference(x, old=None):
    """x [slabs, n] -> sum over slabs (+ old), the sum of |terms| and the number of additions."""
    s, m = x.sum(0), np.abs(x).sum(0)
    if old is not None:
        s, m = s + old, m + np.abs(old)
    return s, m, x.shape[0] + (old is not None)


def colsum_reference(X, row_blocks):
    """part [row_blocks, cols]: block b sums the rows [b r, min((b + 1) r, rows)) with r = ceil(rows / row_blocks); empty blocks: zeros."""
    rows, cols = X.shape
    r = -(-rows // row_blocks)
    part, mag = np.zeros((row_blocks, cols)), np.zeros((row_blocks, cols))
    for b in range(row_blocks):
        blk = X[b * r:min((b + 1) * r, rows)] if b * r < rows else X[:0]
        part[b], mag[b] = blk.sum(0), np.abs(blk).sum(0)
    return part, mag, r


def segment_sum_reference(X, ptr, lst):
    out, mag = np.zeros((len(ptr) - 1, X.shape[1])), np.zeros((len(ptr) - 1, X.shape[1]))
    for s in range(len(ptr) - 1):
        for r in lst[ptr[s]:ptr[s + 1]]:
            out[s] += X[r]
            mag[s] += np.abs(X[r])
    return out, mag, np.maximum(np.diff(ptr), 1).astype(np.float64)[:, None]


# ---------------------------------------------------------------------------------------------------------------- 7. layout casts
def scatter_reference(src, dst_size, dims, src_strides, dst_strides, src_off=0, dst_off=0):
    """(positions, values): dst[dst_off + sum i_k dst_strides[k]] = src[src_off + sum i_k src_strides[k]] over the index space dims."""
    idx = np.indices(dims).reshape(len(dims), -1).astype(np.int64)
    s = src_off + sum(idx[k] * int(src_strides[k]) for k in range(len(dims)))
    d = dst_off + sum(idx[k] * int(dst_strides[k]) for k in range(len(dims)))
    assert s.min() >= 0 and s.max() < src.size and d.min() >= 0 and d.max() < dst_size and len(np.unique(d)) == d.size
    return d, np.asarray(src, dtype=np.float64).reshape(-1)[s]


def transpose_cast_reference(src, dst_size, na, nb, sa_s, sb_s, ss_i, sa_d, sb_d, ds_j):
    """dst[a sa_d + b sb_d + j ds_j + i] = src[a sa_s + b sb_s + i ss_i + j], i, j < 64: index space (a, b, j, i)."""
    return scatter_reference(src, dst_size, (na, nb, 64, 64), (sa_s, sb_s, 1, ss_i), (sa_d, sb_d, ds_j, 1))


def segment_cast_reference(src, dst_size, rows, cols, s_row, s_col, dst_off, dst_ld, src_off):
    pos, val = [], []
    for s in range(len(dst_off)):
        d, v = scatter_reference(src, dst_size, (rows, cols), (s_row, s_col), (int(dst_ld[s]), 1), int(src_off[s]), int(dst_off[s]))
        pos.append(d), val.append(v)
    pos = np.concatenate(pos)
    assert len(np.unique(pos)) == pos.size
    return pos, np.concatenate(val)


CAST_FMT = {0: "f16", 1: "bf16", 2: "f32"}


# ---------------------------------------------------------------------------------------------------------------- 8. SGD
def sgd_reference(w, g, buf, lr, momentum, wd, first):
    """torch.optim.SGD with dampening 0, no Nesterov: g' = g + wd w; buf = g' (first step) or momentum buf + g'; w = w - lr buf.
    Returns (w, buf, sum |terms| of w, sum |terms| of buf).  Roundings on the way: buf 4 (two products, two sums), w 2 more."""
    gg = g + wd * w
    b = gg if first else momentum * buf + gg
    mb = np.abs(g) + np.abs(wd * w) + (0.0 if first else np.abs(momentum * buf))
    return w - lr * b, b, np.abs(w) + np.abs(lr) * mb, mb


N_SGD_W, N_SGD_BUF = 6, 4


# ---------------------------------------------------------------------------------------------------------------- 9. head backward
NG, NP, NS = 15, 11, 24
R = NG + NP + NS
SEG = np.array([0] * NG + [1] * NP + [2] * NS)
U32 = 2.0 ** -24


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def inv_T(T):
    """1 / T as the entry point forms it: in f32."""
    return np.array([float(np.float32(1.0) / np.float32(t)) for t in T])


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def head_forward_outputs(l, s, T):
    """logits l [n, R], s [n, 3] -> (rel [n, R] = log_softmax(l_k / T_k) + sup_k, sup [n, 3] = log_softmax(s)) in float64."""
    def lsm(x):
        x = x - x.max(1, keepdims=True)
        return x - np.log(np.exp(x).sum(1, keepdims=True))
    sup = lsm(s)
    rel = np.concatenate([lsm(l[:, SEG == k] / T[k]) + sup[:, k:k + 1] for k in range(3)], axis=1)
    return rel, sup


def head_loss_reference(rel, sup, conn, p, tgt, a, b, c, y, W, hier, invT, drop_scale, dp_extra=None, cs_coef=None, cand_conf=None,
                        cand_pred=None):
    """The documented loss  -a sup[st] - b rel[t] + c BCE(conn, y) (+ sum_k kappa_k max softmax_k)  per pair and its derivative
    with respect to the 64 packed logits (rows 0 .. R-1 relations, then hier: three super rows and the connectivity row; flat: the
    connectivity row), from the forward's OUTPUTS: softmax(l_k / T_k) = exp(rel - sup_k), softmax(s) = exp(sup); flat: rel are the
    raw logits.  dpre = (p > 0) drop_scale (dl W + dp_extra).  Returns loss, dl, dpre and the error budgets ``e_*``: the absolute
    error that N roundings of 2**-24 on every term, one ulp (2 x 2**-24) per expf / logf / log1pf / division and the rounding of
    every exponent's argument (|x| 2**-24 e^x) allow - see HEAD_ROUNDINGS."""
    n = len(conn)
    dl, e_dl = np.zeros((n, 64)), np.zeros((n, 64))
    loss, e_loss = np.zeros(n), np.zeros(n)
    N = HEAD_ROUNDINGS["hier" if hier else "flat"]
    for i in range(n):
        t = int(tgt[i])
        sig = 1.0 / (1.0 + np.exp(-conn[i]))
        row_c = R + 3 if hier else R
        dl[i, row_c] = c[i] * (sig - y[i])
        e_dl[i, row_c] = N * U32 * abs(c[i]) * (sig + abs(y[i]))
        if c[i] != 0:
            sp = softplus(-conn[i]) if y[i] > 0.5 else softplus(conn[i])
            loss[i] += c[i] * sp
            e_loss[i] += N * U32 * abs(c[i]) * (abs(conn[i]) + np.log(2.0) + 1.0)
        if hier:
            if t >= 0:
                st = SEG[t]
                k = np.nonzero(SEG == st)[0]
                x = rel[i, k] - sup[i, st]
                e = np.exp(x)
                hot = (k == t).astype(np.float64)
                dl[i, k] = b[i] * invT[st] * (e - hot)
                e_dl[i, k] += abs(b[i]) * invT[st] * U32 * (N * (e + hot) + np.abs(x) * e)
                es = np.exp(sup[i])
                hs = (np.arange(3) == st).astype(np.float64)
                dl[i, R:R + 3] = (a[i] + b[i]) * (es - hs)
                e_dl[i, R:R + 3] += (abs(a[i]) + abs(b[i])) * U32 * (N * (es + hs) + np.abs(sup[i]) * es)
                loss[i] += -a[i] * sup[i, st] - b[i] * rel[i, t]
                e_loss[i] += N * U32 * (abs(a[i] * sup[i, st]) + abs(b[i] * rel[i, t]))
            if cs_coef is not None:
                for s2 in range(3):
                    kap = cs_coef[i, s2]
                    if kap == 0:
                        continue
                    k = np.nonzero(SEG == s2)[0]
                    xp = cand_conf[i, s2] - sup[i, s2]
                    pmax = np.exp(xp)
                    x = rel[i, k] - sup[i, s2]
                    e = np.exp(x)
                    hot = (k == cand_pred[i, s2]).astype(np.float64)
                    dl[i, k] += kap * invT[s2] * pmax * (hot - e)
                    e_dl[i, k] += abs(kap) * invT[s2] * pmax * U32 * (N * (hot + e) + np.abs(x) * e + np.abs(xp) * (hot + e))
                    loss[i] += kap * pmax
                    e_loss[i] += abs(kap) * pmax * U32 * (N + abs(xp))
        else:
            x = rel[i]
            m = x.max()
            e = np.exp(x - m)
            ssum = e.sum()
            if t >= 0:
                hot = (np.arange(R) == t).astype(np.float64)
                dl[i, :R] = b[i] * (e / ssum - hot)
                e_dl[i, :R] += abs(b[i]) * U32 * (N * (e / ssum + hot) + np.abs(x - m) * e / ssum + (np.abs(x - m) * e).sum() / ssum * e / ssum)
                loss[i] += -b[i] * (x[t] - m - np.log(ssum))
                e_loss[i] += abs(b[i]) * U32 * (N * (abs(x[t]) + abs(m) + abs(np.log(ssum)) + 1.0) + (np.abs(x - m) * e).sum() / ssum)
            if cs_coef is not None and cs_coef[i, 0] != 0:
                kap = cs_coef[i, 0]
                hot = (np.arange(R) == cand_pred[i, 0]).astype(np.float64)
                pmax = 1.0 / ssum
                dl[i, :R] += kap * pmax * (hot - e / ssum)
                arg = (np.abs(x - m) * e).sum() / ssum
                e_dl[i, :R] += abs(kap) * pmax * U32 * (N * (hot + e / ssum) + np.abs(x - m) * e / ssum + 2 * arg * (hot + e / ssum))
                loss[i] += kap * pmax
                e_loss[i] += abs(kap) * pmax * U32 * (N + arg)
    return (loss, dl) + head_dpre(dl, e_dl, p, W, drop_scale, dp_extra) + (e_loss, e_dl)


def head_dpre(dl, e_dl, p, W, drop_scale, extra):
    """dpre [n, 512] = (p > 0) drop_scale (sum_r dl_r W[r] + extra) and its budget: the budgets of dl through |W|, 66 roundings (64 fused
    multiply-adds, the extra term, the scale) on the sum of |terms|; the bf16 rounding of the result is added by the caller."""
    x = 0.0 if extra is None else extra
    keep = p > 0
    g = dl @ W + x
    mag = np.abs(dl) @ np.abs(W) + np.abs(x)
    return np.where(keep, drop_scale * g, 0.0), np.where(keep, drop_scale * (e_dl @ np.abs(W) + 66 * U32 * mag), 0.0)


HEAD_ROUNDINGS = {
    # hier, a relation row of the target's block with the penalty on it:  expf 2, - [r == t] 1, b / T 1, x 1 (5);  penalty: expf of the
    # maximum 2, expf of the row 2, [r == pred] - e 1, kappa / T 1, x pmax 1, x 1 (8);  their sum 1: 14.  A super row: a + b 1, expf 2, - 1,
    # x 1 (5).  The connectivity row: expf 2, 1 + 1, the division 2, - y 1, x c 1 (7).  The loss: two products and a sum (3), the softplus
    # (expf 2, log1pf 2, max + 1, x c 1, + 1: 7), three penalty terms (expf 2, x 1, + 1 each).  16 covers every path.
    "hier": 16,
    # flat: the maximum is exact; expf 2, the sum of 50 terms over the wavefront's six exchange steps 6, the division 2, - 1, x b 1 (12); the
    # penalty the same again with 1 / s (2), x kappa 1, x 1, + 1 (17); the loss: x - m - logf(s) 2 + 2 + 6, x b 1, + 1.  32 covers every path.
    "flat": 32,
}


def head_upstream_reference(rel, sup, p, g_rel, g_sup, g_conn, g_hidden, W, hier, invT, drop_scale):
    """dL/d(packed logits) for upstream gradients of rel (log-probs; flat: the logits themselves), sup and the connectivity logit:
    rel_r = log_softmax(l / T)_r + sup_k, sup = log_softmax(s):  d l_r = (G_r - softmax_r sum_block G) / T_k;
    d s_j = Gs_j - softmax(s)_j sum Gs with Gs_k = g_sup_k + sum_block_k G."""
    n = len(rel)
    dl, e_dl = np.zeros((n, 64)), np.zeros((n, 64))
    gs_in = np.zeros((n, 3)) if g_sup is None else g_sup
    gc = np.zeros(n) if g_conn is None else g_conn
    N = 16                                                           # block sums: 6 exchange steps; expf 2; x, -, x: 3; Gs and its total: 3
    if hier:
        for k in range(3):
            idx = np.nonzero(SEG == k)[0]
            tot = g_rel[:, idx].sum(1, keepdims=True)
            atot = np.abs(g_rel[:, idx]).sum(1, keepdims=True)
            x = rel[:, idx] - sup[:, k:k + 1]
            e = np.exp(x)
            dl[:, idx] = invT[k] * (g_rel[:, idx] - e * tot)
            e_dl[:, idx] = invT[k] * U32 * (N * (np.abs(g_rel[:, idx]) + e * atot) + np.abs(x) * e * atot)
        Gs = gs_in + np.stack([g_rel[:, SEG == k].sum(1) for k in range(3)], axis=1)
        aGs = np.abs(gs_in) + np.stack([np.abs(g_rel[:, SEG == k]).sum(1) for k in range(3)], axis=1)
        es = np.exp(sup)
        dl[:, R:R + 3] = Gs - es * Gs.sum(1, keepdims=True)
        e_dl[:, R:R + 3] = U32 * (N * (aGs + es * aGs.sum(1, keepdims=True)) + np.abs(sup) * es * aGs.sum(1, keepdims=True))
        dl[:, R + 3] = gc
    else:
        dl[:, :R] = g_rel
        dl[:, R] = gc
    return (dl,) + head_dpre(dl, e_dl, p, W, drop_scale, g_hidden) + (e_dl,)


def head_wgrad_reference(dl, p, chunk):
    """part [ceil(n / chunk), 64, 513]: columns 0 .. 511 = sum over the chunk's pairs of dl[pair][r] p[pair][k], column 512 = sum dl."""
    n = len(dl)
    nb = -(-n // chunk)
    part, mag = np.zeros((nb, 64, 513)), np.zeros((nb, 64, 513))
    for b in range(nb):
        d, q = dl[b * chunk:(b + 1) * chunk], p[b * chunk:(b + 1) * chunk]
        part[b, :, :512], part[b, :, 512] = d.T @ q, d.sum(0)
        mag[b, :, :512], mag[b, :, 512] = np.abs(d).T @ np.abs(q), np.abs(d).sum(0)
    return part, mag


def head_case(rng, n, hier, regime_scale=1.0):
    """Seeded logits and coefficients of n pairs with the planted rows: targets in each of the three blocks and -1, coef_c 0, conn_y 0
    and 1, hidden values that are 0 and negative.  Everything the kernel reads is f32-representable."""
    l = rng.standard_normal((n, R)) * 2.0
    s = rng.standard_normal((n, 3))
    T = (1.0, 1.5, 0.75) if hier else (1.0, 1.0, 1.0)
    invT = inv_T(T)
    if hier:
        rel, sup = head_forward_outputs(l, s, 1.0 / invT)
    else:
        rel, sup = l, np.zeros((n, 3))
    assert n >= 5
    tgt = rng.integers(-1, R, n)
    tgt[:5] = [3, NG + 2, NG + NP + 7, -1, R - 1]
    c = rng.uniform(0.1, 2.0, n)
    c[1] = 0.0
    y = (rng.uniform(size=n) < 0.5).astype(np.float64)
    y[:5] = [1, 0, 1, 0, 1]
    p = rng.standard_normal((n, 512))
    p[:, 0::7] = 0.0
    p[:, 3::11] = -np.abs(p[:, 3::11]) - 0.5
    case = dict(rel=f32(rel), sup=f32(sup), conn=f32(rng.standard_normal(n) * 2), p=f32(p), tgt=tgt.astype(np.int32),
                a=f32(rng.uniform(0.2, 1.5, n)), b=f32(rng.uniform(0.2, 3.0, n)), c=f32(c), y=y, W=f32(rng.standard_normal((64, 512)) * 0.1),
                T=T, invT=invT, dp_extra=f32(rng.standard_normal((n, 512)) * 0.05))
    nseg = 3 if hier else 1
    kap = rng.uniform(0.1, 1.0, (n, nseg))
    kap[rng.uniform(size=(n, nseg)) < 0.4] = 0.0
    case["cs_coef"] = f32(kap)
    if hier:                                                     # the forward's candidates: per block the maximum log-prob and its first arg-max
        cc = np.stack([case["rel"][:, SEG == k].max(1) for k in range(3)], axis=1)
        off = np.array([0, NG, NG + NP])
        cp = np.stack([case["rel"][:, SEG == k].argmax(1) + off[k] for k in range(3)], axis=1)
    else:
        cc, cp = case["rel"].max(1, keepdims=True), case["rel"].argmax(1)[:, None]
    case["cand_conf"], case["cand_pred"] = cc, cp.astype(np.int32)
    return case
