"""Box sets, definitional float64 / int64 references and checking helpers for the non-GEMM kernels of csrc/kernels_shared.hip
(tests/test_shared_glue_gpu.py runs the kernels, tests/test_shared_glue_cases_cpu.py tests this file without a device).  NumPy only.

The references are DEFINITIONS, not restatements of the kernels' formulas: fc1 of a pair is the float64 sum of the 64 product rows its
windows use (``fc1_reference``), not the inclusion-exclusion over prefix tables the device evaluates (``fc1_inclusion_exclusion`` - kept
only so that the CPU self-test can compare the two in int64); a gradient sum is the sum over the pairs whose window was a copy of the
object's row; dz of a pixel is the sum of the patch pixels that cover it; dU is the sum over the object's pairs whose dz exists there
and whose route equals the slot; a linear pair's window is pre_(i,bg) + pre_(bg,j) - pre_(bg,bg), then bias, ReLU, 2x2 max.
Rectangles come from ``pairs.object_window_rects`` / ``pairs.object_d16_rects`` (pinned against the device's plan by
tests/test_shared_kernels_gpu.py::test_window_plan_and_pixel_rectangles).

Two regimes.  EXACT: small-integer operands; ``assert_exact`` holds per output element (sum of |terms| < 2**24), so every f32 partial
sum in any order is the exact one and the output must equal, bit for bit, the exact sum rounded ONCE, to nearest even, to the output
type (``rne``: the reference rounds itself).  REAL: seeded reals, per element |got - ref| <= u_out |ref| + n 2**-24 sum |terms|
(``real_bound``), u_bf16 = 2**-8, u_f16 = 2**-11, n the number of f32 additions behind the element - derived, never fitted."""
import numpy as np

from scene_graph_commonsense_amd.pairs import object_d16_rects, object_window_rects

WY, WX = np.divmod(np.arange(64), 8)
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 2.0 ** -24}
_FMT = {"bf16": (7, -126), "f16": (10, -14), "f32": (23, -126)}          # explicit mantissa bits, exponent of the smallest normal
PATCH_SLOTS = 20
FULL_PIXRECT = (16 << 5) | (16 << 15)

# ---------------------------------------------------------------------------------------------------------------- box sets
# 32-grid, slice semantics (x0, x1, y0, y1) as normalise_boxes emits them
FULL, CORNER_HI, CORNER_LO, EMPTY, REVERSED = [0, 32, 0, 32], [31, 32, 31, 32], [0, 1, 0, 1], [10, 10, 4, 9], [9, 3, 5, 8]
STRIP, BEYOND, IDENT, OVERLAP = [3, 4, 0, 32], [30, 40, 28, 36], [2, 6, 2, 6], [4, 10, 4, 10]
LIN_A, LIN_B = IDENT, [10, 14, 2, 6]          # window rectangles meet (x windows 0..3 and 1..5), D16 rectangles 0..4 and 4..8 do not
BASE_IMAGES = [[FULL, CORNER_HI, CORNER_LO, EMPTY, REVERSED, STRIP], [], [IDENT, IDENT, OVERLAP, LIN_B, BEYOND]]
FULL2_IMAGES = [[FULL, FULL, CORNER_LO, CORNER_HI]]          # a pair with 64 X entries and a pair with none


def rect_mask(r):
    """[n, 4] window rectangles -> [n, 64] bool: window w = 8 wy + wx inside the rectangle."""
    r = np.asarray(r).reshape(-1, 4)
    return (WX[None] >= r[:, 0:1]) & (WX[None] < r[:, 1:2]) & (WY[None] >= r[:, 2:3]) & (WY[None] < r[:, 3:4])


def pack_pixrect(x0, x1, y0, y1):
    """Pixels of the 16-grid within one pixel of a window rectangle: Y0 | Y1 << 5 | X0 << 10 | X1 << 15, 0 for an empty one."""
    if x1 <= x0 or y1 <= y0:
        return 0
    return max(2 * y0 - 1, 0) | (min(2 * y1 + 1, 16) << 5) | (max(2 * x0 - 1, 0) << 10) | (min(2 * x1 + 1, 16) << 15)


def pixrect_mask(r):
    """packed pixel rectangle -> [16, 16] bool (Y, X)."""
    Y, X = np.mgrid[0:16, 0:16]
    return (Y >= (r & 31)) & (Y < ((r >> 5) & 31)) & (X >= ((r >> 10) & 31)) & (X < ((r >> 15) & 31))


def csr(index, n):
    """ptr / list of pair ids grouped by object id, stable (what engine_core.csr_by builds)."""
    index = np.asarray(index)
    order = np.argsort(index, kind="stable").astype(np.int32)
    return np.searchsorted(index[order], np.arange(n + 1)).astype(np.int32), order


def all_pairs(img_ptr):
    s, o = [], []
    for b in range(len(img_ptr) - 1):
        for i in range(img_ptr[b], img_ptr[b + 1]):
            for j in range(img_ptr[b], img_ptr[b + 1]):
                if i != j:
                    s.append(i), o.append(j)
    return np.array(s, dtype=np.int32), np.array(o, dtype=np.int32)


def shuffled_subset(sub, obj, seed):
    """A shuffled subset (two thirds) of a pair list with one pair duplicated."""
    rng = np.random.default_rng(seed)
    k = rng.permutation(len(sub))[:max(2, 2 * len(sub) // 3)]
    k = np.concatenate([k, k[:1]])
    return sub[k].copy(), obj[k].copy()


class Scene:
    """Boxes of a few images, a pair list and every table of the shared-window plan, computed on the host from the definitions:
    the three window lists (all X windows / the pairs that convolve / the linear pairs, the first two with the pseudo-pairs' windows
    R_o behind them), and the window-major row space in its full and compact forms."""

    def __init__(self, images, pairs=None, pad=8, extra=0):
        self.n_img = len(images)
        self.img_ptr = np.concatenate([[0], np.cumsum([len(b) for b in images])]).astype(np.int32)
        self.bb = np.array([b for im in images for b in im], dtype=np.int32).reshape(-1, 4)
        self.n = n = len(self.bb)
        self.n2 = 2 * n
        self.obj_img = np.repeat(np.arange(self.n_img), np.diff(self.img_ptr)).astype(np.int32)
        self.R, self.D = object_window_rects(self.bb), object_d16_rects(self.bb)
        self.inside = rect_mask(self.R)                                     # [n, 64]
        self.sub, self.obj = all_pairs(self.img_ptr) if pairs is None else (np.asarray(pairs[0], np.int32), np.asarray(pairs[1], np.int32))
        self.P = P = len(self.sub)
        R, D = self.R, self.D
        self.X = np.zeros((P, 4), dtype=np.int64)
        self.linear = np.zeros(P, dtype=bool)
        for p, (i, j) in enumerate(zip(self.sub, self.obj)):
            x = [max(R[i, 0], R[j, 0]), min(R[i, 1], R[j, 1]), max(R[i, 2], R[j, 2]), min(R[i, 3], R[j, 3])]
            if x[1] <= x[0] or x[3] <= x[2]:
                continue
            self.X[p] = x
            meet = max(D[i, 0], D[j, 0]) < min(D[i, 1], D[j, 1]) and max(D[i, 2], D[j, 2]) < min(D[i, 3], D[j, 3])
            self.linear[p] = not meet
        self.xmask = rect_mask(self.X)                                       # [P, 64]
        self.cnt_all = self.xmask.sum(1).astype(np.int32)
        self.cnt_lin = np.where(self.linear, self.cnt_all, 0).astype(np.int32)
        self.cnt_conv = (self.cnt_all - self.cnt_lin).astype(np.int32)
        self.pixrect_conv = np.array([0 if self.linear[p] else pack_pixrect(*self.X[p]) for p in range(P)], dtype=np.int32)
        self.cnt_obj = np.tile(self.inside.sum(1), 2).astype(np.int32)      # [n2]
        self.pixrect_obj = np.tile(np.array([pack_pixrect(*r) for r in R], dtype=np.int32).reshape(-1), 2)
        codes = lambda sel: [p * 64 + w for p in range(P) if sel[p] for w in np.nonzero(self.xmask[p])[0]]
        ocodes = [(P + ps) * 64 + w for ps in range(self.n2) for w in np.nonzero(self.inside[ps % n])[0]] if n else []
        self.E_all, self.E_obj = int(self.cnt_all.sum()), len(ocodes)
        self.E_lin, self.E_conv = int(self.cnt_lin.sum()), int(self.cnt_conv.sum())
        self.gather_all = np.array(codes(np.ones(P, bool)) + ocodes, dtype=np.int32)
        self.gather_conv = np.array(codes(~self.linear) + ocodes, dtype=np.int32)
        self.gather_lin = np.array(codes(self.linear), dtype=np.int32)
        self.obj_entry = np.full((self.n2, 64), -1, dtype=np.int64)          # (ps, w) -> index among the pseudo-pairs' entries
        for k, c in enumerate(ocodes):
            self.obj_entry[(c >> 6) - P, c & 63] = k
        self.incl_all = np.cumsum(np.concatenate([self.cnt_all, self.cnt_obj])).astype(np.int32)
        self.incl_conv = np.cumsum(np.concatenate([self.cnt_conv, self.cnt_obj])).astype(np.int32)
        self.incl_lin = np.cumsum(np.concatenate([self.cnt_lin, 0 * self.cnt_obj])).astype(np.int32)
        # ---- window-major row spaces: counts of X entries / of objects per window, groups padded to a multiple of ``pad`` (+ extra)
        xw = self.gather_all[:self.E_all] & 63
        self.counts = np.bincount(xw, minlength=64).astype(np.int64)
        self.objs = self.inside.sum(0).astype(np.int64)
        rank = np.zeros(self.E_all, dtype=np.int64)                          # rank of an X entry among its window's entries, list order
        seen = np.zeros(64, dtype=np.int64)
        for e, w in enumerate(xw):
            rank[e] = seen[w]
            seen[w] += 1
        self.spaces = {}
        for name, lead in (("full", np.full(64, self.n2, dtype=np.int64)), ("compact", self.n_img + 2 * self.objs)):
            size = (lead + self.counts + extra + pad - 1) // pad * pad
            goff = np.concatenate([[0], np.cumsum(size)]).astype(np.int32)
            xbase = (goff[:64] + lead).astype(np.int32)
            gend = (xbase + self.counts).astype(np.int32)
            prow = np.zeros(self.n2 * 64, dtype=np.int32)
            for w in range(64):
                k = 0
                for ps in range(self.n2):
                    o = ps % n
                    if name == "full":
                        prow[ps * 64 + w] = goff[w] + ps
                    elif self.inside[o, w]:
                        prow[ps * 64 + w] = goff[w] + self.n_img + k
                        k += 1
                    else:
                        prow[ps * 64 + w] = goff[w] + self.obj_img[o]
            dest = np.zeros(len(self.gather_all), dtype=np.int32)
            dest[:self.E_all] = xbase[xw] + rank
            oc = self.gather_all[self.E_all:]
            dest[self.E_all:] = prow[((oc >> 6) - P) * 64 + (oc & 63)]
            # the conv list's rows: the same (pair, window) of the list of all windows
            pos = {int(c): k for k, c in enumerate(self.gather_all)}
            dest_conv = np.array([dest[pos[int(c)]] for c in self.gather_conv], dtype=np.int32)
            self.spaces[name] = dict(lead=lead, goff=goff, xbase=xbase, gend=gend, prow=prow, dest=dest, dest_conv=dest_conv, rows=int(goff[64]))

    def kinds(self):
        """number of (linear, X non-empty and not linear, X empty) pairs."""
        return int(self.linear.sum()), int(((self.cnt_all > 0) & ~self.linear).sum()), int((self.cnt_all == 0).sum())

    def first_all(self, k):
        return int(self.incl_all[k - 1]) if k else 0


def base_scene(subset=False):
    sc = Scene(BASE_IMAGES)
    if subset:
        sc = Scene(BASE_IMAGES, pairs=shuffled_subset(sc.sub, sc.obj, 7))
    return sc


def many_objects_scene(n=130, seed=11):
    """One image of ``n`` objects (2 n pseudo-pairs > 256: the second pass of compact_rows_kernel's loop), no pairs."""
    rng = np.random.default_rng(seed)
    x0, y0 = rng.integers(0, 30, n), rng.integers(0, 30, n)
    bb = np.stack([x0, x0 + rng.integers(1, 12, n), y0, y0 + rng.integers(1, 12, n)], axis=1)
    return Scene([bb.tolist()], pairs=(np.zeros(0, np.int32), np.zeros(0, np.int32)))


def small_boxes(rng, n, span=6):
    x0, y0 = rng.integers(0, 30, n), rng.integers(0, 30, n)
    return np.stack([x0, x0 + rng.integers(1, span, n), y0, y0 + rng.integers(1, span, n)], axis=1).tolist()


def gsum_groups_scene(swap=False, seed=13):
    """Images of 0, 1, 8, 9 and 17 objects (0, 1, 1, 2, 3 role-0 groups); in the last one object k = 0..3 is the subject of exactly
    16, 15, 1 and 17 pairs (the tail of a 16-pair step and both half-waves; 17 through one duplicated pair).  ``swap``: the same
    list with subject and object exchanged, so that the counts are those of role 1."""
    rng = np.random.default_rng(seed)
    images = [[], small_boxes(rng, 1, 20), small_boxes(rng, 8, 20), small_boxes(rng, 9, 20), small_boxes(rng, 17, 20)]
    images[4][0], images[4][5] = FULL, EMPTY
    ptr = np.concatenate([[0], np.cumsum([len(b) for b in images])])
    s, o = all_pairs(ptr[:5])                                                     # every ordered pair of the images of 8 and 9 objects
    s, o = list(s), list(o)
    a = int(ptr[4])
    for k, cnt in ((0, 16), (1, 15), (2, 1), (3, 17)):
        others = [a + t for t in range(17) if t != k]
        for t in range(cnt):
            s.append(a + k)
            o.append(others[t % 16])
    return Scene(images, pairs=(o, s) if swap else (s, o))


def gsum_many_partners_scene(n=514, seed=17):
    """One image of 514 objects; object 0 is the subject of 513 pairs and the object of 513 (more than GSUM_MAXP = 512)."""
    rng = np.random.default_rng(seed)
    boxes = small_boxes(rng, n, 4)
    boxes[0] = [6, 22, 8, 20]
    k = np.arange(1, n)
    return Scene([boxes], pairs=(np.concatenate([0 * k, k]), np.concatenate([k, 0 * k])))


def contract_scene():
    """One image of 72 objects: S1 = object 0 (full image) with the 70 partners 2..71, which all cover pixel (0, 0) (more than 64
    candidates: the second 64-chunk), S2 = object 1 (full image) with the 9 nested boxes 2..10 only (0 .. 9 candidates over the
    pixels: every arm of the request / route schedule); pairs in both directions."""
    size = {1: 1, 2: 3, 3: 7, 4: 11, 5: 15}                               # box stop -> a window rectangle 1 .. 5 wide
    nested = [[0, size[(k + 3) // 2], 0, size[(k + 2) // 2]] for k in range(9)]      # (1,1), (2,1), (2,2), (3,2) .. (5,5): strictly nested
    images = [[FULL, FULL] + nested + [[0, 20 + (k % 7), 0, 18 + (k % 5)] for k in range(61)]]
    s = [0] * 70 + [1] * 9
    o = list(range(2, 72)) + list(range(2, 11))
    return Scene(images, pairs=(s + o, o + s))


def linear_scene(counts=(1, 3, 4, 5, 16, 17, 65, 70)):
    """Image b: one box LIN_A and counts[b] copies of LIN_B, the pairs (A, B_k) - all linear, six X windows each, so every
    (image, window) segment of the background side has 0 or counts[b] entries; a last image without objects."""
    images = [[LIN_A] + [LIN_B] * c for c in counts] + [[]]
    ptr = np.concatenate([[0], np.cumsum([len(b) for b in images])])
    s, o = [], []
    for b, c in enumerate(counts):
        a = int(ptr[b])
        s += [a] * c
        o += [a + 1 + k for k in range(c)]
    return Scene(images, pairs=(s, o))


def linear_objects_scene():
    """For the per-object side: A with 70 linear partners (second ballot chunk), a B touched by 1 pair, by 2 (a duplicated pair), and
    the base set's boxes (entries no linear pair touches, pairs that are not linear)."""
    images = [[LIN_A] + [LIN_B] * 70, BASE_IMAGES[2], BASE_IMAGES[0]]
    s, o = [0] * 70 + [0], list(range(1, 71)) + [1]
    s2, o2 = all_pairs(np.array([71, 76, 82]))
    return Scene(images, pairs=(s + list(s2), o + list(o2)))


# ---------------------------------------------------------------------------------------------------------------- number formats
def rne(x, fmt):
    """float64 -> the nearest value of ``fmt`` (ties to even, subnormals, saturating f16 as the kernels' store does), as float64."""
    x = np.asarray(x, dtype=np.float64)
    mant, emin = _FMT[fmt]
    _, e = np.frexp(x)                                                # |x| = m 2**e, m in [0.5, 1)
    ulp = np.ldexp(1.0, np.maximum(e - 1, emin) - mant)
    y = np.rint(x / ulp) * ulp                                        # np.rint: half to even
    if fmt == "f16":
        y = np.clip(y, -65504.0, 65504.0)
    return y


def to_bits(x, fmt):
    """values representable in ``fmt`` (float64) -> their bit patterns (uint16 / uint32), -0 as +0."""
    x = np.asarray(x, dtype=np.float64) + 0.0
    if fmt == "f16":
        b = x.astype(np.float16).view(np.uint16)
        return np.where(b == 0x8000, 0, b).astype(np.uint16)
    f = x.astype(np.float32).view(np.uint32)
    f = np.where(f == 0x80000000, 0, f).astype(np.uint32)
    return f if fmt == "f32" else (f >> 16).astype(np.uint16)


def from_bits(b, fmt):
    b = np.asarray(b)
    if fmt == "f16":
        return b.astype(np.uint16).view(np.float16).astype(np.float64)
    if fmt == "bf16":
        return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def assert_exact(mag, what):
    """EXACT regime: per output element the sum of |terms| is below 2**24, so every f32 partial sum is exact in any order."""
    m = float(np.max(mag)) if np.size(mag) else 0.0
    assert m < 2.0 ** 24, "%s: sum of |terms| = %g is not below 2**24" % (what, m)


def rounding_cases(ref, fmt):
    """(values the format cannot hold, exact halves among them) in a float64 reference."""
    ref = np.asarray(ref, dtype=np.float64)
    mant, emin = _FMT[fmt]
    _, e = np.frexp(ref)
    q = ref / np.ldexp(1.0, np.maximum(e - 1, emin) - mant)           # in units of the format's step at that magnitude
    lost = q != np.rint(q)
    return int(lost.sum()), int((lost & (q - np.floor(q) == 0.5)).sum())


def check_bits(got_bits, ref, fmt, what):
    """EXACT: the output's bits against the float64 reference rounded once (RNE) to ``fmt``; -0 counts as +0."""
    got = np.asarray(got_bits)
    zero = {"f16": 0x8000, "bf16": 0x8000, "f32": 0x80000000}[fmt]
    got = np.where(got == zero, 0, got)
    exp = to_bits(rne(ref, fmt), fmt).reshape(got.shape)
    bad = got != exp
    if bad.any():
        k = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, expected %r (exact %r)"
                             % (what, int(bad.sum()), bad.size, k, float(from_bits(got[k], fmt)), float(from_bits(exp[k], fmt)),
                                float(np.asarray(ref).reshape(got.shape)[k])))


def real_bound(ref, mag, n, fmt, scale=1.0):
    """u_out |ref| + scale n 2**-24 sum |terms| (+ half a subnormal step of the format)."""
    mant, emin = _FMT[fmt]
    return U[fmt] * np.abs(ref) + scale * n * 2.0 ** -24 * mag + 2.0 ** (emin - mant - 1)


def check_real(got, ref, bound, what, quiet=False):
    """REAL: |got - ref| <= bound for every element; returns (and prints) the worst ratio."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref.reshape(got.shape))
    err = np.where(np.isnan(err), np.inf, err)
    ratio = err / np.broadcast_to(bound, ref.shape).reshape(got.shape)
    worst = float(ratio.max()) if ratio.size else 0.0
    if not quiet:
        print("SHARED-GLUE real regime %-66s worst got/bound = %.4f" % (what, worst))
    assert worst <= 1.0, "%s: worst err / bound = %g" % (what, worst)
    return worst


def values(rng, shape, regime, lo=-8, hi=8, channels_last=True):
    """EXACT: integers; channel c (last axis) draws from [lo, hi] for c % 4 != 1 and from [-2, 2] for c % 4 == 1 (exact zeros and
    ties).  REAL: standard normals scaled by (hi - lo) / 4."""
    if regime == "real":
        return rng.standard_normal(shape) * ((hi - lo) / 4.0)
    v = rng.integers(lo, hi + 1, shape).astype(np.float64)
    small = rng.integers(-2, 3, shape).astype(np.float64)
    c = np.arange(shape[-1]) % 4 == 1
    return np.where(c, small, v)


# ---------------------------------------------------------------------------------------------------------------- fc1 forward
def pseudo_rows(sc, own, bg):
    """T[ps][w]: the product row pseudo-pair ps uses at window w - its own row inside R_o, the background row of its image outside.
    own [n2, 64, C] (read only inside R_o), bg [n_img, 64, C]."""
    ins = np.tile(sc.inside, (2, 1))[:, :, None]
    img = np.tile(sc.obj_img, 2)
    return np.where(ins, own, bg[img])


def fc1_reference(sc, T, xprod, bias):
    """pre [P, C] = bias + the float64 sum of the 64 rows pair p's windows use: subject i's pseudo row outside R_j, object j's role-1
    pseudo row inside R_j and outside R_i, the pair's own X entry otherwise.  Also mag [P, C] = |b| + 5 sum |T_i| + 8 sum |T'_j| +
    sum |X products| (the terms behind the device's prefix tables) and the number of X entries per pair."""
    n, P = sc.n, sc.P
    pre = np.zeros((P, T.shape[-1]))
    mag = np.zeros_like(pre)
    for p, (i, j) in enumerate(zip(sc.sub, sc.obj)):
        e0 = sc.first_all(p)
        k = 0
        acc = bias.astype(np.float64).copy()
        for w in range(64):
            if not sc.inside[j, w]:
                acc += T[i, w]
            elif not sc.inside[i, w]:
                acc += T[n + j, w]
            else:
                acc += xprod[e0 + k]
                k += 1
        assert k == sc.cnt_all[p]
        pre[p] = acc
        mag[p] = np.abs(bias) + 5 * np.abs(T[i]).sum(0) + 8 * np.abs(T[n + j]).sum(0) + np.abs(xprod[e0:e0 + k]).sum(0)
    return pre, mag, sc.cnt_all.astype(np.float64)


def fc1_activation(pre, keep=None):
    """ReLU, then dropout with the kept values doubled (scale = 2)."""
    h = np.maximum(pre, 0.0)
    return h if keep is None else np.where(keep, 2.0 * h, 0.0)


def integral_reference(T):
    """S [n2, 9, 9, C]: inclusive 2-D prefix sums of T [n2, 64, C] over the 8 x 8 window grid, zero border; and the sums of |T|."""
    n2, _, C = T.shape
    S = np.zeros((n2, 9, 9, C), dtype=T.dtype)
    S[:, 1:, 1:] = T.reshape(n2, 8, 8, C).cumsum(1).cumsum(2)
    A = np.zeros((n2, 9, 9, C))
    A[:, 1:, 1:] = np.abs(T).reshape(n2, 8, 8, C).cumsum(1).cumsum(2)
    return S, A


def rect_sum(S, r):
    x0, x1, y0, y1 = (int(v) for v in r)
    if x1 <= x0:
        return 0 * S[0, 0]
    return S[y1, x1] - S[y0, x1] - S[y1, x0] + S[y0, x0]


def fc1_inclusion_exclusion(sc, T, xprod, bias):
    """The device's expression b + S_i[all] - S_i[R_j] + S'_j[R_j] - S'_j[X_p] + sum X products, evaluated in the dtype of T."""
    S, _ = integral_reference(T)
    out = []
    for p, (i, j) in enumerate(zip(sc.sub, sc.obj)):
        e0 = sc.first_all(p)
        Si, Sj = S[i], S[sc.n + j]
        out.append(bias + Si[8, 8] - rect_sum(Si, sc.R[j]) + rect_sum(Sj, sc.R[j]) - rect_sum(Sj, sc.X[p]) + xprod[e0:e0 + sc.cnt_all[p]].sum(0))
    return np.stack(out) if out else np.zeros((0, T.shape[-1]), dtype=T.dtype)


def own_rect_reference(sc, T):
    """[n, C]: the sum of object j's role-1 rows over its own rectangle (exact 0 for an empty one), and the sum of their magnitudes."""
    m = sc.inside[:, :, None]
    return (T[sc.n:] * m).sum(1), (np.abs(T[sc.n:]) * m).sum(1)


# ---------------------------------------------------------------------------------------------------------------- fc1 backward sums
def copy_matrix(sc):
    """M [P, n2, 64] 0/1: window w of pair p was a copy of pseudo-pair ps's row (the assembly's copy matrix)."""
    M = np.zeros((sc.P, sc.n2, 64), dtype=np.int64)
    for p, (i, j) in enumerate(zip(sc.sub, sc.obj)):
        M[p, i] = ~sc.inside[j]
        M[p, sc.n + j] = sc.inside[j] & ~sc.inside[i]
    return M


def gsum_reference(sc, dh, only_inside=False):
    """G [n2, 64, C]: the sum of dh over the pairs whose window w was a copy of (role, o)'s row; BG [n_img, 64, C]: the sum over the
    subjects i of image b with w outside R_i of G[(0, i)][w]; with the sums of magnitudes and the numbers of terms of both.
    ``only_inside``: G, A, N hold only the (ps, w) with w inside R_o, in row-major order ([k, C]: what the compact space stores)."""
    n, C = sc.n, dh.shape[1]
    ins = np.tile(sc.inside, (2, 1))
    idx = np.arange(sc.n2 * 64).reshape(sc.n2, 64)
    rows = sc.n2 * 64
    if only_inside:
        idx = np.full((sc.n2, 64), -1)
        idx[ins] = np.arange(int(ins.sum()))
        rows = int(ins.sum())
    G, A, N = np.zeros((rows, C)), np.zeros((rows, C)), np.zeros((rows, 1))
    BG, BA, BN = np.zeros((sc.n_img, 64, C)), np.zeros((sc.n_img, 64, C)), np.zeros((sc.n_img, 64, 1))
    ad = np.abs(dh)
    for p, (i, j) in enumerate(zip(sc.sub, sc.obj)):
        mi, mj = ~sc.inside[j], sc.inside[j] & ~sc.inside[i]
        for ps, m in ((i, mi), (n + j, mj)):
            k = idx[ps][m]
            k = k[k >= 0]
            G[k] += dh[p]
            A[k] += ad[p]
            N[k] += 1
        out = mi & ~sc.inside[i]                                  # a copy of subject i's row that was itself the background row
        BG[sc.obj_img[i]][out] += dh[p]
        BA[sc.obj_img[i]][out] += ad[p]
        BN[sc.obj_img[i]][out] += 1
    BN += np.diff(sc.img_ptr).reshape(-1, 1, 1)                   # one more addition per subject of the image
    if not only_inside:
        G, A, N = G.reshape(sc.n2, 64, C), A.reshape(sc.n2, 64, C), N.reshape(sc.n2, 64, 1)
    return G, A, N, BG, BA, BN


# ---------------------------------------------------------------------------------------------------------------- linear pairs
def pool_reference(pre, bias):
    """pre [..., 4, C] -> (value [..., C] float64, code [..., C]): + bias, ReLU, max over the 4 pixels; the smallest pixel index wins
    a tie; a maximum the ReLU kills gives value 0 and code 4."""
    code = np.argmax(pre, axis=-2)                                   # np.argmax: first occurrence
    v = np.take_along_axis(pre, code[..., None, :], axis=-2)[..., 0, :] + bias
    dead = ~(v > 0)
    return np.where(dead, 0.0, v), np.where(dead, 4, code).astype(np.uint8)


def linear_pre_reference(sc, raw_own, raw_bg):
    """[E_lin, 4, C]: pre_(i,bg)[w] + pre_(bg,j)[w] - pre_(bg,bg)[w] for every listed window of the linear pairs, with the sum of
    magnitudes.  raw_own [E_obj, 4, C]: the pre-activations of the pseudo-pairs' own windows in list order (``Scene.obj_entry``
    [n2, 64] names the entry of (ps, w)), raw_bg [n_img, 64, 4, C].  Also the entries of both that some listed window names."""
    p, w = sc.gather_lin >> 6, sc.gather_lin & 63
    i, j = sc.sub[p], sc.obj[p]
    ei, ej = sc.obj_entry[i, w], sc.obj_entry[sc.n + j, w]
    assert (ei >= 0).all() and (ej >= 0).all()
    a, b, g = raw_own[ei], raw_own[ej], raw_bg[sc.obj_img[i], w]
    used_own = np.zeros(len(raw_own), bool)
    used_own[ei], used_own[ej] = True, True
    used_bg = np.zeros(raw_bg.shape[:2], bool)
    used_bg[sc.obj_img[i], w] = True
    return a + b - g, np.abs(a) + np.abs(b) + np.abs(g), used_own, used_bg


def unpool(dy, code):
    """[..., C] gradient and codes -> [..., 4, C]: the gradient at the routed pixel, zero elsewhere (code 4: nowhere)."""
    q = np.arange(4).reshape((1,) * (dy.ndim - 1) + (4, 1))
    return np.where(code[..., None, :] == q, dy[..., None, :], 0.0)


# ---------------------------------------------------------------------------------------------------------------- conv3 data-gradient tail
PATCH_ROW20 = [pp + (pp > 5) + (pp > 6) + (pp > 9) + (pp > 10) for pp in range(16)]
PATCH_CENTRE = [pp in (5, 6, 9, 10) for pp in range(16)]


def patch_sum_reference(sc, V, A, incl, gather, first_pair, n_list):
    """dz [n_list pairs, 16, 16, C] (Y, X) = the sum of the patch pixels that cover the pixel: patch pixel (py, px) of the listed
    window (wy, wx) is pixel (2 wy - 1 + py, 2 wx - 1 + px).  V / A [entries, 16, C]: values / magnitudes per (entry, patch pixel).
    Pairs first_pair .. first_pair + n_list - 1 of the list (incl, gather); returns (dz, mag, number of terms)."""
    C = V.shape[-1]
    dz, mag, cnt = np.zeros((n_list, 16, 16, C)), np.zeros((n_list, 16, 16, C)), np.zeros((n_list, 16, 16, 1))
    for k in range(n_list):
        pair = first_pair + k
        e0 = int(incl[pair - 1]) if pair else 0
        for e in range(e0, int(incl[pair])):
            assert gather[e] >> 6 == pair
            wy, wx = divmod(int(gather[e]) & 63, 8)
            for pp in range(16):
                Y, Xp = 2 * wy - 1 + pp // 4, 2 * wx - 1 + pp % 4
                if 0 <= Y < 16 and 0 <= Xp < 16:
                    dz[k, Y, Xp] += V[e, pp]
                    mag[k, Y, Xp] += A[e, pp]
                    cnt[k, Y, Xp] += 2 if PATCH_CENTRE[pp] else 1
    return dz, mag, cnt


def pixel_row(Y, X):
    """row of pixel (Y, X) inside a pair's [256] window-major pixel rows."""
    return 4 * ((Y >> 1) * 8 + (X >> 1)) + (Y & 1) * 2 + (X & 1)


def contract_reference(sc, role, dz, codes, pixrect, bg_maps):
    """dU [n + n_img, 16, 16, 4, C]: for object o the sum over its pairs (the real pairs of its list and its pseudo-pair) whose dz
    exists at the pixel (pixel rectangle) and whose route equals q; for the background object of image b the pseudo-pairs of the
    other role of that image's objects (+ its all-background map).  dz [pairs, 16, 16, C], codes [pairs, 16, 16, C] by (Y, X)."""
    n, P, C = sc.n, sc.P, dz.shape[-1]
    ptr, lst = csr(sc.obj if role else sc.sub, n)
    masks = np.stack([pixrect_mask(int(r)) for r in pixrect])
    dU, mag, cnt = np.zeros((n + sc.n_img, 16, 16, 4, C)), np.zeros((n + sc.n_img, 16, 16, 1, C)), np.zeros((n + sc.n_img, 16, 16, 1, 1))

    def add(o, k, m):
        v = np.where(m[:, :, None], dz[k], 0.0)
        dU[o] += unpool(v, codes[k])
        mag[o][:, :, 0] += np.abs(v)
        cnt[o][:, :, 0, 0] += m

    for o in range(n):
        ps = P + (n + o if role else o)
        cell = masks[ps]                                              # outside the pseudo-pair's rectangle nothing contributes
        for k in lst[ptr[o]:ptr[o + 1]]:
            add(o, int(k), masks[k] & cell)
        add(o, ps, cell)
    for b in range(sc.n_img):
        for i in range(sc.img_ptr[b], sc.img_ptr[b + 1]):
            k = P + (i if role else n + i)
            add(n + b, k, masks[k])
        if bg_maps:
            add(n + b, P + 2 * n + b, np.ones((16, 16), bool))
    return dU, mag, cnt
