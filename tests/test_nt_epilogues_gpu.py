"""Every fused epilogue of the dense NT GEMM family (csrc/gemm_nt.h, csrc/gemm_nt_pp.h) through the shipped C ABI, on every block
the launchers choose, against the float64 references of tests/nt_epilogue_cases.py.

EXACT regime: small-integer operands for which ``assert_exact`` holds, so the f32 accumulators equal the float64 result and every output
is compared bit for bit (values rounded once with torch's round-to-nearest-even casts).  REAL regime: seeded reals, per-element bound
``u |ref| + acc_bound`` (u = 2**-11 f16, 2**-8 bf16, 2**-23 f32), routing codes checked without exclusions against the same bound; the
worst err / bound of each test is printed.  Outputs are pre-filled with 0xFF bytes (NaN in every float type, no routing code): whatever
the kernel does not own must keep them.

Which block a shape reaches follows from the launchers' size rule (launch_gemm_nt: a 256x256 block from M * N >= 256**3 with
N % 256 == 0 - the halo block for 3x3 convolutions on whole 16x16 maps, the ping-pong block for plain rows, the two-stage block for
the other convolutions - else the 128x128 block; the listed-window and grouped launchers always take the ping-pong block)."""
import ctypes

import pytest
import torch

from tests import nt_epilogue_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
U16, UBF, U32 = 2.0 ** -11, 2.0 ** -8, 2.0 ** -23
REGIMES = ["exact", "real"]


@pytest.fixture(scope="module")
def cases():
    """The shared operands and float64 references (built once per regime, kept on the device), released when the module ends."""
    built = {}

    def get(builder, regime):
        if (builder, regime) not in built:
            built[(builder, regime)] = builder(regime)
        return built[(builder, regime)]

    yield get
    built.clear()
    torch.cuda.empty_cache()


def _lib():
    from scene_graph_commonsense_amd import _lib
    return _lib.load(), _lib


def _filled(shape, dtype):
    """A tensor of 0xFF bytes: NaN for f16 / bf16 / f32, 255 for the routing bytes."""
    n = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}[dtype]
    t = torch.full(shape, -1 if n != torch.uint8 else 255, dtype=n, device=DEV)
    return t.view(dtype)


def _bits(t):
    return t if t.dtype == torch.uint8 else t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _is_fill(t):
    return _bits(t) == (255 if t.dtype == torch.uint8 else -1)


def _assert_untouched(t, what):
    bad = int((~_is_fill(t)).sum())
    assert bad == 0, "%s: %d elements outside the kernel's rows / columns were written" % (what, bad)


def _assert_bits(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, what
    if not torch.equal(_bits(got), _bits(exp)):
        d = _bits(got) != _bits(exp)
        i = d.nonzero()[0].tolist()
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, expected %r"
                             % (what, int(d.sum()), d.numel(), i, got[tuple(i)].item(), exp[tuple(i)].item()))


def _assert_close(got, ref, u, accb, what, extra=0.0):
    """|got - ref| <= u |ref| + acc_bound (+ extra), element by element; prints the worst err / bound."""
    ref = ref.to(got.device)
    err = (got.double() - ref).abs()
    bound = u * ref.abs() + accb.to(got.device) + extra
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("NT-EPILOGUE real regime %-58s worst err/bound = %.4f" % (what, worst))
    assert worst <= 1.0, "%s: worst err / bound = %g" % (what, worst)


def _assert_codes(code, pre, bias, accb, what):
    """Routing bytes of the real regime, no exclusions: T = the window's largest acc_bound, m = its float64 maximum; a code c < 4 needs
    pre[c] >= m - 2T and m + bias > -T; code 4 needs m + bias <= T."""
    p4 = pre.view(-1, 4, pre.shape[1])
    T = accb.view(-1, 4, accb.shape[1]).max(1).values
    m = p4.max(1).values
    mb = m + (bias.double() if bias is not None else 0.0)
    c = code.long()
    assert bool((c <= 4).all()), what + ": a routing byte above 4"
    chosen = p4.gather(1, c.clamp(max=3).unsqueeze(1)).squeeze(1)
    ok = torch.where(c < 4, (chosen >= m - 2 * T) & (mb > -T), mb <= T)
    assert bool(ok.all()), "%s: %d routing bytes outside the bound" % (what, int((~ok).sum()))


def _real(shape, seed, kind="normal", scale=1.0, sparsity=0.0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g) if kind == "normal" else torch.rand(shape, generator=g)
    if sparsity:
        t = t * (torch.rand(shape, generator=g) >= sparsity)
    return t * scale


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).to(DEV)


def _big_bias(n, seed, lo=120, step=8, big=2400):
    """Integer bias: small everywhere, + ``big`` on every ``step``-th column so that outputs above 2048 (not exact in f16) occur."""
    b = C.exact_operands((n,), range(-lo, lo + 1), 1.0, 1.0, seed)
    b[::step] += big
    return b


# ------------------------------------------------------------------------------------------------------------ conv3 (+ pooling)
def _conv3_case(regime):
    """64 pairs' maps z_pad [64][18][18][512] f16, w3r [1024][9*512] f16, b3; float64 pre-activations of all rows and the magnitude sums."""
    n = 64
    if regime == "exact":
        z = C.exact_operands((n, 16, 16, 512), (1, 2, 3), 0.15, 1.0, 101)
        w = C.exact_operands((1024, 9 * 512), (-3, -2, -1, 1, 2, 3), 0.5, 1.0, 102)
        b = _big_bias(1024, 103)
    else:
        z = _real((n, 16, 16, 512), 111, "uniform", 1.0, 0.5)
        w = _real((1024, 9 * 512), 112, "normal", 0.02)
        b = _real((1024,), 113, "normal", 0.5)
    zp = torch.zeros(n, 18, 18, 512, dtype=torch.float16, device=DEV)
    zp[:, 1:17, 1:17] = z.half().to(DEV)
    w = w.half().to(DEV)
    b = b.float().to(DEV)
    pre = C.conv3x3_rows(zp, w, 4)
    mag = C.conv3x3_rows(zp.abs(), w.abs(), 4)
    if regime == "exact":
        C.assert_exact(zp, w, b.view(1, -1), mag=mag)
        val, code = C.pool_ref(pre, b)
        p4 = pre.view(-1, 4, 1024)
        m = p4.max(1).values
        assert bool(((p4 == m.unsqueeze(1)).sum(1) > 1)[code < 4].any()), "no tie among the pixels of a live window"
        assert bool(((m + b.double()) == 0).any()), "no pre-activation of exactly 0"
        assert bool((val > 2048).any()) and bool(((val > 2048) & (val % 2 == 1)).any()), "no value above 2048 that f16 has to round"
    return dict(z=zp, w=w, b=b, pre=pre, accb=C.acc_bound(None, None, 9 * 512, mag=mag))


def _check_pool_outputs(regime, case, rows, y, ybf, am, what, pre=None, accb=None):
    """y / ybf / am hold the pooled rows ``rows`` (indices into the case's window rows, or None with explicit pre / accb)."""
    pre = case["pre"].view(-1, 4, 1024)[rows].reshape(-1, 1024) if pre is None else pre
    val, code = C.pool_ref(pre, case["b"])
    if regime == "exact":
        if y is not None: _assert_bits(y, val.half(), what + " y")
        if ybf is not None: _assert_bits(ybf, val.bfloat16(), what + " y_bf16")
        if am is not None: _assert_bits(am, code, what + " argmax")
    else:
        accb = case["accb"].view(-1, 4, 1024)[rows].reshape(-1, 1024) if accb is None else accb
        T = accb.view(-1, 4, 1024).max(1).values
        if y is not None: _assert_close(y, val, U16, T, what + " y")
        if ybf is not None: _assert_close(ybf, val, UBF, T, what + " y_bf16")
        if am is not None: _assert_codes(am, pre, case["b"], accb, what + " argmax")


@pytest.mark.parametrize("n_pairs", [64, 63])     # 64: M * N = 256**3, whole maps -> halo block, nt_epilogue_pool16<.., HALO>; 63: 128x128 block
@pytest.mark.parametrize("regime", REGIMES)
def test_conv3_relu_pool(cases, regime, n_pairs):
    lib, L = _lib()
    c = cases(_conv3_case, regime)
    R, G = n_pairs * 64, 64                         # G guard rows behind every output

    def run(n, with_am=True, with_bf=True):
        y, ybf, am = _filled((n * 64 + G, 1024), torch.float16), _filled((n * 64 + G, 1024), torch.bfloat16), _filled((n * 64 + G, 1024), torch.uint8)
        assert lib.sgc_conv3_relu_pool(L.ptr(c["z"]), L.ptr(c["w"]), L.ptr(c["b"]), L.ptr(y), L.ptr(am) if with_am else None,
                                       L.ptr(ybf) if with_bf else None, n, L.stream_ptr()) == 0
        torch.cuda.synchronize()
        return y, ybf, am

    y, ybf, am = run(n_pairs)
    rows = torch.arange(R, device=DEV)
    _check_pool_outputs(regime, c, rows, y[:R], ybf[:R], am[:R], "conv3_relu_pool %d pairs" % n_pairs)
    for t in (y, ybf, am):
        _assert_untouched(t[R:], "conv3_relu_pool guard rows")
    # an absent output changes nothing else
    y2, ybf2, am2 = run(n_pairs, with_am=False)
    assert torch.equal(_bits(y2), _bits(y)) and torch.equal(_bits(ybf2), _bits(ybf))
    _assert_untouched(am2, "argmax = NULL")
    y3, ybf3, am3 = run(n_pairs, with_bf=False)
    assert torch.equal(_bits(y3), _bits(y)) and torch.equal(am3, am)
    _assert_untouched(ybf3, "y_bf16 = NULL")
    if regime == "exact" and n_pairs == 63:         # the two blocks agree bit for bit on the rows they share
        y64, ybf64, am64 = run(64)
        assert torch.equal(_bits(y64[:R]), _bits(y[:R])) and torch.equal(_bits(ybf64[:R]), _bits(ybf[:R])) and torch.equal(am64[:R], am[:R])


@pytest.mark.parametrize("n_pairs", [64, 63])
@pytest.mark.parametrize("regime", REGIMES)
def test_conv3_relu_pool_wm(cases, regime, n_pairs):
    """Window-major rows: y / bf16 of (pair ps, window w) at goff[w] + ps, with padding between the groups; routing bytes stay pair-major."""
    lib, L = _lib()
    c = cases(_conv3_case, regime)
    goff = torch.arange(64) * (n_pairs + 5) + 3
    total = int(goff[-1]) + n_pairs + 7
    y, ybf, am = _filled((total, 1024), torch.float16), _filled((total, 1024), torch.bfloat16), _filled((n_pairs * 64 + 64, 1024), torch.uint8)
    assert lib.sgc_conv3_relu_pool_wm(L.ptr(c["z"]), L.ptr(c["w"]), L.ptr(c["b"]), L.ptr(_i32(goff)), L.ptr(y), L.ptr(am), L.ptr(ybf),
                                      n_pairs, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    prow = torch.arange(n_pairs * 64)
    dst = (goff[prow % 64] + prow // 64).to(DEV)
    _check_pool_outputs(regime, c, prow.to(DEV), y[dst], ybf[dst], am[:n_pairs * 64], "conv3_relu_pool_wm %d pairs" % n_pairs)
    keep = torch.ones(total, dtype=torch.bool, device=DEV)
    keep[dst] = False
    _assert_untouched(y[keep], "ywm padding rows")
    _assert_untouched(ybf[keep], "ywm_bf16 padding rows")
    _assert_untouched(am[n_pairs * 64:], "argmax guard rows")


def _window_list(n_windows, n_listed, seed):
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(n_windows, generator=g)
    return perm[:n_listed].sort().values, int(perm[n_listed])          # the sorted list, and one window that is not on it


@pytest.mark.parametrize("regime", REGIMES)
def test_conv3_relu_pool_windows_family(cases, regime):
    """Listed windows on the ping-pong gather block (nt_epilogue_pool16<.., GATHER>): 203 of the 384 windows of 6 maps, bound 320 - tiles
    0-2 full, tile 3 ragged (812 rows), tile 4 wholly beyond the list; raw_first = 70 falls inside tile 1."""
    lib, L = _lib()
    c = cases(_conv3_case, regime)
    n_maps, n, bound, raw_first = 6, 203, 320, 70
    lst, spare = _window_list(n_maps * 64, n, 7)
    gather = torch.full((bound,), spare, dtype=torch.int64)           # entries behind the list name a valid window that is not listed
    gather[:n] = lst
    gd, nd = _i32(gather), _i32([n])
    rows = lst.to(DEV)
    W = n_maps * 64

    def outs(nrows):
        return _filled((nrows, 1024), torch.float16), _filled((nrows, 1024), torch.bfloat16), _filled((W, 1024), torch.uint8)

    def check_rows(y, ybf, am, dst, what):
        _check_pool_outputs(regime, c, rows, y[dst], ybf[dst], am[rows], what)
        for t, d in ((y, dst), (ybf, dst), (am, rows)):
            keep = torch.ones(t.shape[0], dtype=torch.bool, device=DEV)
            keep[d] = False
            _assert_untouched(t[keep], what + ": unlisted rows")

    # results at rows gather[e]
    y, ybf, am = outs(W)
    assert lib.sgc_conv3_relu_pool_windows(L.ptr(c["z"]), L.ptr(c["w"]), L.ptr(c["b"]), L.ptr(gd), L.ptr(nd), bound, L.ptr(y), L.ptr(am),
                                           L.ptr(ybf), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    check_rows(y, ybf, am, rows, "conv3_relu_pool_windows")
    if regime == "exact":                              # the same windows from the whole-map launch on those maps (128x128 block)
        yd, ybd, amd = outs(W)
        assert lib.sgc_conv3_relu_pool(L.ptr(c["z"]), L.ptr(c["w"]), L.ptr(c["b"]), L.ptr(yd), L.ptr(amd), L.ptr(ybd), n_maps, L.stream_ptr()) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(yd[rows]), _bits(y[rows])) and torch.equal(_bits(ybd[rows]), _bits(ybf[rows])) and torch.equal(amd[rows], am[rows])
    # y / bf16 at dest[e], routing bytes at gather[e]
    g = torch.Generator().manual_seed(8)
    dest = torch.randperm(512, generator=g)[:bound]
    dd = _i32(dest)
    dst = dest[:n].to(DEV)
    y, ybf, am = outs(512)
    assert lib.sgc_conv3_relu_pool_windows_wm(L.ptr(c["z"]), L.ptr(c["w"]), L.ptr(c["b"]), L.ptr(gd), L.ptr(nd), L.ptr(dd), bound, L.ptr(y),
                                              L.ptr(am), L.ptr(ybf), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    check_rows(y, ybf, am, dst, "conv3_relu_pool_windows_wm")
    # ... and the accumulators of the entries >= raw_first
    y, ybf, am = outs(512)
    raw = _filled(((bound - raw_first) * 4, 1024), torch.float32)
    assert lib.sgc_conv3_relu_pool_windows_wm_raw(L.ptr(c["z"]), L.ptr(c["w"]), L.ptr(c["b"]), L.ptr(gd), L.ptr(nd), L.ptr(dd), bound, L.ptr(y),
                                                  L.ptr(am), L.ptr(ybf), L.ptr(raw), raw_first, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    check_rows(y, ybf, am, dst, "conv3_relu_pool_windows_wm_raw")
    nraw = (n - raw_first) * 4
    pre = c["pre"].view(-1, 4, 1024)[rows[raw_first:]].reshape(-1, 1024)
    if regime == "exact":
        _assert_bits(raw[:nraw], pre.float(), "windows_wm_raw raw rows")
    else:
        _assert_close(raw[:nraw], pre, U32, c["accb"].view(-1, 4, 1024)[rows[raw_first:]].reshape(-1, 1024), "windows_wm_raw raw rows")
    _assert_untouched(raw[nraw:], "raw rows behind the list")
    # an empty list writes nothing
    y, ybf, am = outs(512)
    raw = _filled(((bound - raw_first) * 4, 1024), torch.float32)
    zero = _i32([0])
    assert lib.sgc_conv3_relu_pool_windows_wm_raw(L.ptr(c["z"]), L.ptr(c["w"]), L.ptr(c["b"]), L.ptr(gd), L.ptr(zero), L.ptr(dd), bound, L.ptr(y),
                                                  L.ptr(am), L.ptr(ybf), L.ptr(raw), raw_first, L.stream_ptr()) == 0
    assert lib.sgc_conv3_relu_pool_windows(L.ptr(c["z"]), L.ptr(c["w"]), L.ptr(c["b"]), L.ptr(gd), L.ptr(zero), bound, L.ptr(y), L.ptr(am),
                                           L.ptr(ybf), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    for t in (y, ybf, am, raw):
        _assert_untouched(t, "gather_n = 0")


@pytest.mark.parametrize("regime", REGIMES)
def test_conv3_windows_raw(cases, regime):
    """f32 accumulators of the listed windows, rows 4e + q (ping-pong gather block, generic f32 store)."""
    lib, L = _lib()
    c = cases(_conv3_case, regime)
    n, bound = 203, 320
    lst, spare = _window_list(6 * 64, n, 7)
    gather = torch.full((bound,), spare, dtype=torch.int64)
    gather[:n] = lst
    raw = _filled((bound * 4, 1024), torch.float32)
    assert lib.sgc_conv3_windows_raw(L.ptr(c["z"]), L.ptr(c["w"]), L.ptr(_i32(gather)), L.ptr(_i32([n])), bound, L.ptr(raw), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    rows = lst.to(DEV)
    pre = c["pre"].view(-1, 4, 1024)[rows].reshape(-1, 1024)
    if regime == "exact":
        _assert_bits(raw[:4 * n], pre.float(), "conv3_windows_raw")
    else:
        _assert_close(raw[:4 * n], pre, U32, c["accb"].view(-1, 4, 1024)[rows].reshape(-1, 1024), "conv3_windows_raw")
    _assert_untouched(raw[4 * n:], "conv3_windows_raw rows behind the list")
    raw = _filled((bound * 4, 1024), torch.float32)
    assert lib.sgc_conv3_windows_raw(L.ptr(c["z"]), L.ptr(c["w"]), L.ptr(_i32(gather)), L.ptr(_i32([0])), bound, L.ptr(raw), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    _assert_untouched(raw, "conv3_windows_raw, gather_n = 0")


def test_conv3_windows_distant_list_entries():
    """One 64-entry tile whose windows come from maps 0, 1, 3300, 6500 and 6599 of 6600: the last ones lie more than 2**31 bytes behind the
    tile's first map (a conv3 map is 331 776 bytes), beyond what one buffer descriptor with a 32-bit offset reaches - such a tile is
    computed again by the far-tile pass, which addresses every list entry through its own map (gemm_nt_pp_far_kernel, csrc/gemm_nt_pp.h);
    the second tile of the list is not far and stays the first kernel's.  Exact regime, every output bit for bit; runs once."""
    lib, L = _lib()
    n_maps = 6600
    maps = [0, 1, 3300, 6500, 6599]
    zp = torch.zeros(n_maps, 18, 18, 512, dtype=torch.float16, device=DEV)
    for i, mp in enumerate(maps):
        zp[mp, 1:17, 1:17] = C.exact_operands((16, 16, 512), (1, 2, 3), 0.15, 1.0, 300 + i).half().to(DEV)
    w = C.exact_operands((1024, 9 * 512), (-3, -2, -1, 1, 2, 3), 0.5, 1.0, 102).half().to(DEV)
    b = _big_bias(1024, 103).float().to(DEV)
    # 13 + 13 + 13 + 13 + 18 = 70 entries: tile 0 = entries 0..63 holds windows of all five maps (odd counts: the two entries of one load
    # instruction come from different maps), tile 1 the last 6 windows of map 6599
    g = torch.Generator().manual_seed(9)
    lst = torch.cat([mp * 64 + torch.randperm(64, generator=g)[:(18 if mp == 6599 else 13)].sort().values for mp in maps])
    n, bound = int(lst.numel()), 128
    assert n == 70 and bool((lst[1:] > lst[:-1]).all()) and int(lst[63]) // 64 == 6599
    assert (int(lst[63]) // 64 - int(lst[0]) // 64) * 18 * 18 * 512 * 2 > 2 ** 31
    gather = torch.full((bound,), 5, dtype=torch.int64)
    gather[:n] = lst
    pre = C.conv3x3_rows(zp, w, 4, windows=lst)
    C.assert_exact(None, w, b.view(1, -1), mag=C.conv3x3_rows(zp.abs(), w.abs(), 4, windows=lst))
    assert bool((pre.view(n, 4, 1024)[40:64].abs().sum((1, 2)) > 0).all())           # the far maps' windows are not zero rows
    val, code = C.pool_ref(pre, b)
    W = n_maps * 64
    y, ybf, am = _filled((W, 1024), torch.float16), _filled((W, 1024), torch.bfloat16), _filled((W, 1024), torch.uint8)
    assert lib.sgc_conv3_relu_pool_windows(L.ptr(zp), L.ptr(w), L.ptr(b), L.ptr(_i32(gather)), L.ptr(_i32([n])), bound, L.ptr(y), L.ptr(am),
                                           L.ptr(ybf), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    rows = lst.to(DEV)
    _assert_bits(y[rows], val.half(), "distant entries y")
    _assert_bits(ybf[rows], val.bfloat16(), "distant entries y_bf16")
    _assert_bits(am[rows], code, "distant entries argmax")
    for t in (y, ybf, am):
        _bits(t)[rows] = 255 if t.dtype == torch.uint8 else -1
        _assert_untouched(t, "distant entries: unlisted rows")


# ------------------------------------------------------------------------------------------------------------ conv2
def _conv2_case(regime):
    n = 32
    if regime == "exact":
        a = C.exact_operands((n, 32, 32, 128), (-3, -2, -1, 1, 2, 3), 0.5, 1.0, 201)
        w = C.exact_operands((512, 9 * 128), (-3, -2, -1, 1, 2, 3, 40), 0.5, 1.0, 202)
        b = _big_bias(512, 203)
    else:
        a = torch.tanh(_real((n, 32, 32, 128), 211))
        w = _real((512, 9 * 128), 212, "normal", 0.03)
        b = _real((512,), 213, "normal", 0.5)
    ap = torch.zeros(n, 34, 34, 128, dtype=torch.float16, device=DEV)
    ap[:, 1:33, 1:33] = a.half().to(DEV)
    w, b = w.half().to(DEV), b.float().to(DEV)
    pre = C.conv3x3_rows(ap, w, 5)
    mag = C.conv3x3_rows(ap.abs(), w.abs(), 5)
    if regime == "exact":
        C.assert_exact(ap, w, b.view(1, -1), mag=mag)
        for v in (pre, pre + b.double()):            # without and with bias: an exact 0 and an odd value above 2048 (f16 has to round)
            assert bool((v == 0).any()) and bool(((v.abs() > 2048) & (v % 2 == 1)).any())
    return dict(a=ap, w=w, b=b, pre=pre, accb=C.acc_bound(None, None, 9 * 128, mag=mag))


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("n_obj", [32, 31])       # 32: M * N = 256**3 on 32x32 maps -> the two-stage 256x256 block, nt_epilogue_store16; 31: 128x128
@pytest.mark.parametrize("regime", REGIMES)
def test_conv2_object(cases, regime, n_obj, with_bias):
    lib, L = _lib()
    c = cases(_conv2_case, regime)
    R = n_obj * 1024
    out = _filled((R + 256, 512), torch.float16)
    assert lib.sgc_conv2_object(L.ptr(c["a"]), L.ptr(c["w"]), L.ptr(c["b"]) if with_bias else None, L.ptr(out), n_obj, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    ref = c["pre"][:R] + (c["b"].double() if with_bias else 0.0)
    what = "conv2_object %d objects%s" % (n_obj, "" if with_bias else ", no bias")
    if regime == "exact":
        _assert_bits(out[:R], ref.half(), what)
    else:
        _assert_close(out[:R], ref, U16, c["accb"][:R], what)
    _assert_untouched(out[R:], what + ": guard rows")


@pytest.mark.parametrize("regime", REGIMES)
def test_conv2_object_regions(cases, regime):
    """150 of the 768 2x2 windows of three 32x32 maps, bound 256 (ping-pong gather block, generic 16-bit store): rows 4 gather[e] + q."""
    lib, L = _lib()
    c = cases(_conv2_case, regime)
    n, bound = 150, 256
    lst, spare = _window_list(3 * 256, n, 17)
    gather = torch.full((bound,), spare, dtype=torch.int64)
    gather[:n] = lst
    uv = _filled((3 * 1024, 512), torch.float16)
    assert lib.sgc_conv2_object_regions(L.ptr(c["a"]), L.ptr(c["w"]), L.ptr(c["b"]), L.ptr(_i32(gather)), L.ptr(_i32([n])), bound, L.ptr(uv),
                                        L.stream_ptr()) == 0
    torch.cuda.synchronize()
    rows = (lst.repeat_interleave(4) * 4 + torch.arange(4).repeat(n)).to(DEV)
    ref = c["pre"][rows] + c["b"].double()
    if regime == "exact":
        _assert_bits(uv[rows], ref.half(), "conv2_object_regions")
    else:
        _assert_close(uv[rows], ref, U16, c["accb"][rows], "conv2_object_regions")
    keep = torch.ones(3 * 1024, dtype=torch.bool, device=DEV)
    keep[rows] = False
    _assert_untouched(uv[keep], "conv2_object_regions: unlisted rows")


@pytest.mark.parametrize("regime", REGIMES)
def test_conv2_dgrad_regions(regime):
    """bf16 data gradient of conv2 on listed cells, N = 128 (128x128 gather block, generic store): rows 4 gather[e] + q of da."""
    lib, L = _lib()
    n_obj, n, bound = 3, 150, 256
    if regime == "exact":
        d = C.exact_operands((n_obj, 32, 32, 512), (-3, -2, -1, 1, 2, 3), 0.2, 1.0, 221)
        w = C.exact_operands((128, 9 * 512), (-2, -1, 1, 2), 0.5, 1.0, 222)
    else:
        d = _real((n_obj, 32, 32, 512), 231, "normal", 0.5)
        w = _real((128, 9 * 512), 232, "normal", 0.03)
    dp = torch.zeros(n_obj, 34, 34, 512, dtype=torch.bfloat16, device=DEV)
    dp[:, 1:33, 1:33] = d.bfloat16().to(DEV)
    w = w.bfloat16().to(DEV)
    lst, spare = _window_list(n_obj * 256, n, 18)
    gather = torch.full((bound,), spare, dtype=torch.int64)
    gather[:n] = lst
    da = _filled((n_obj * 1024, 128), torch.bfloat16)
    assert lib.sgc_conv2_dgrad_regions(L.ptr(dp), L.ptr(w), L.ptr(_i32(gather)), L.ptr(_i32([n])), bound, L.ptr(da), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    ref = C.conv3x3_rows(dp, w, 5, windows=lst)
    mag = C.conv3x3_rows(dp.abs(), w.abs(), 5, windows=lst)
    rows = (lst.repeat_interleave(4) * 4 + torch.arange(4).repeat(n)).to(DEV)
    if regime == "exact":
        C.assert_exact(dp, w, None, mag=mag)
        assert bool((ref == 0).any()) and bool((ref.bfloat16().double() != ref).any())           # a value that bf16 has to round
        _assert_bits(da[rows], ref.bfloat16(), "conv2_dgrad_regions")
    else:
        _assert_close(da[rows], ref, UBF, C.acc_bound(None, None, 9 * 512, mag=mag), "conv2_dgrad_regions")
    keep = torch.ones(n_obj * 1024, dtype=torch.bool, device=DEV)
    keep[rows] = False
    _assert_untouched(da[keep], "conv2_dgrad_regions: unlisted rows")


# ------------------------------------------------------------------------------------------------------------ conv1
def _ordered_f16(t):
    """f16 bit patterns on a scale where neighbouring values differ by one."""
    b = t.view(torch.int16).int()
    return torch.where(b < 0, -(b & 0x7FFF), b)


@pytest.mark.parametrize("XC", [64, 192])
@pytest.mark.parametrize("regime", REGIMES)
def test_conv1_tanh(regime, XC):
    """bias + tanh on the 128x128 block, 300 rows (ragged last tile).  Exact regime: pre-activations that are multiples of 1/8 within
    +-3 - the accumulator is exact, the f16 result may differ from the correctly rounded tanh by one ulp (tanhf)."""
    lib, L = _lib()
    M = 300
    if regime == "exact":
        x = torch.zeros(M, XC, dtype=torch.float64)
        g = torch.Generator().manual_seed(41 + XC)
        for k in range(2):                                  # two non-zeros per row (they may fall on one column)
            x[torch.arange(M), torch.randint(0, XC, (M,), generator=g)] += C.exact_operands((M,), (-1, 1, 2), 1.0, 1.0, 42 + k + XC)
        x = x.clamp(-2, 2)
        w = C.exact_operands((128, XC), range(-4, 5), 1.0, 0.125, 44 + XC)
        b = C.exact_operands((128,), range(-8, 9), 1.0, 0.125, 45 + XC)
    else:
        x, w, b = _real((M, XC), 51 + XC), _real((128, XC), 52 + XC, "normal", 0.1), _real((128,), 53 + XC, "normal", 0.3)
    x, w, b = x.half().to(DEV), w.half().to(DEV), b.float().to(DEV)
    out = _filled((M + 128, 128), torch.float16)
    assert lib.sgc_conv1_tanh(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(out), M, XC, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    pre = x.double() @ w.double().t() + b.double()
    if regime == "exact":
        C.assert_exact(x, w, b.view(1, -1), 1.0, 0.125)
        assert float(pre.abs().max()) <= 3.0 and bool((pre == 0).any()) and bool((pre * 8 == (pre * 8).round()).all())
        exp = torch.tanh(pre).half()
        d = (_ordered_f16(out[:M]) - _ordered_f16(exp)).abs()
        assert int(d.max()) <= 1, "conv1_tanh: %d f16 ulps from tanh of the exact pre-activation" % int(d.max())
        assert torch.equal(_bits(out[:M])[pre == 0], torch.zeros_like(_bits(out[:M])[pre == 0]))
    else:
        _assert_close(out[:M], torch.tanh(pre), U16, C.acc_bound(x, w, XC), "conv1_tanh XC=%d" % XC, extra=4 * 2.0 ** -24)
    _assert_untouched(out[M:], "conv1_tanh guard rows")


# ------------------------------------------------------------------------------------------------------------ fc1 / fc2 forward
def _keep_mask(seed, rows, cols):
    from scene_graph_commonsense_amd.synthetic import dropout_keep_mask
    return torch.from_numpy(dropout_keep_mask(seed, rows, cols)).to(DEV)


def _check_dropout(run, base, P, N, dtype, what, ref=None, u=None, accb=None):
    """run(seed) -> output with dropout; the keep mask is the host replica's, dropped elements are +0, kept ones 2 x the no-dropout
    values bit for bit.  Doubling commutes with rounding only while the no-dropout output is a NORMAL number of its type (an f16 value
    below 2**-14 was rounded on the subnormal grid before the test doubles it, and one rounded to 0 says nothing about twice its f32
    value), so in the real regime (``ref``: float64 no-dropout reference) the kept elements whose no-dropout output is subnormal or
    zero are held to the regime's own bound around 2 ref instead: |got - 2 ref| <= u |2 ref| + 2 acc_bound.  The exact regime has no
    such values but 0 itself and compares every bit."""
    tiny = {torch.float16: 2.0 ** -14, torch.float32: 2.0 ** -126}[dtype]
    for seed in (3, 1234567):
        got = run(seed)
        keep = _keep_mask(seed, P, N)
        assert 0.4 < float(keep.float().mean()) < 0.6
        exp = torch.where(keep, (base.float() * 2).to(dtype), torch.zeros((), dtype=dtype, device=DEV))
        if ref is None:
            _assert_bits(got, exp, "%s, dropout seed %d" % (what, seed))
            continue
        sub = keep & (base.float().abs() < tiny)
        _assert_bits(torch.where(sub, exp, got), exp, "%s, dropout seed %d" % (what, seed))
        _assert_close(got[sub], 2 * ref[sub], u, 2 * accb[sub], "%s, dropout seed %d, doubled subnormals" % (what, seed))


@pytest.mark.parametrize("P", [4096 + 37, 300])     # 4133 x 4096 >= 256**3: ping-pong block, generic bias / ReLU epilogue, ragged last tile; 300: 128x128
@pytest.mark.parametrize("regime", REGIMES)
def test_fc1_relu(regime, P):
    lib, L = _lib()
    K = 192
    if regime == "exact":
        y = C.exact_operands((P, K), (1, 2, 3), 0.3, 1.0, 61)
        w = C.exact_operands((4096, K), (-3, -2, -1, 1, 2, 3), 1.0, 1.0, 62)
        b = _big_bias(4096, 63, lo=60)
    else:
        y, w, b = _real((P, K), 71, "uniform", 1.0, 0.5), _real((4096, K), 72, "normal", 0.05), _real((4096,), 73, "normal", 0.3)
    y, w, b = y.half().to(DEV), w.half().to(DEV), b.float().to(DEV)

    def run(drop, seed=0):
        h = _filled((P + 64, 4096), torch.float16)
        assert lib.sgc_fc1_relu(L.ptr(y), L.ptr(w), L.ptr(b), L.ptr(h), P, K, drop, seed, L.stream_ptr()) == 0
        torch.cuda.synchronize()
        _assert_untouched(h[P:], "fc1_relu guard rows")
        return h[:P]

    h = run(0)
    pre = y.double() @ w.double().t() + b.double()
    what = "fc1_relu %d pairs" % P
    if regime == "exact":
        C.assert_exact(y, w, b.view(1, -1))
        assert bool((pre == 0).any()) and bool(((pre > 2048) & (pre % 2 == 1)).any())
        _assert_bits(h, pre.clamp(min=0).half(), what)
    else:
        _assert_close(h, pre.clamp(min=0), U16, C.acc_bound(y, w, K), what)
    if regime == "exact":
        _check_dropout(lambda s: run(1, s), h, P, 4096, torch.float16, what)
    else:
        _check_dropout(lambda s: run(1, s), h, P, 4096, torch.float16, what, pre.clamp(min=0), U16, C.acc_bound(y, w, K))


def _fc2_case(regime):
    P, n_obj = 16384 + 5, 37
    if regime == "exact":
        h = C.exact_operands((P, 4096), (1, 2, 3), 0.1, 1.0, 81)
        w = C.exact_operands((512, 4096), (-3, -2, -1, 1, 2, 3), 0.5, 1.0, 82)
        b = C.exact_operands((512,), range(-50, 51), 1.0, 1.0, 83)
        ls, lo = C.exact_operands((n_obj, 512), range(-40, 41), 1.0, 1.0, 84), C.exact_operands((n_obj, 512), range(-40, 41), 1.0, 1.0, 85)
    else:
        h, w = _real((P, 4096), 91, "uniform", 1.0, 0.5), _real((512, 4096), 92, "normal", 0.02)
        b, ls, lo = _real((512,), 93, "normal", 0.3), _real((n_obj, 512), 94, "normal", 0.5), _real((n_obj, 512), 95, "normal", 0.5)
    g = torch.Generator().manual_seed(86)
    si, oi = torch.randint(0, n_obj, (P,), generator=g), torch.randint(0, n_obj, (P,), generator=g)
    si[[0, 299, P - 1]] = n_obj - 1                       # the last label row, also in the first and the last pair
    oi[[1, 298, P - 2]] = n_obj - 1
    h, w = h.half().to(DEV), w.half().to(DEV)
    b, ls, lo = b.float().to(DEV), ls.float().to(DEV), lo.float().to(DEV)
    si, oi = si.to(DEV), oi.to(DEV)
    add = b.double() + ls.double()[si] + lo.double()[oi]
    pre = h.double() @ w.double().t() + add
    mag = h.double().abs() @ w.double().abs().t()
    if regime == "exact":
        C.assert_exact(h, w, add, mag=mag)
        assert bool((pre == 0).any()) and bool((pre < 0).any())
    return dict(h=h, w=w, b=b, ls=ls, lo=lo, si=si.int(), oi=oi.int(), pre=pre, accb=C.acc_bound(None, None, 4096, mag=mag))


@pytest.mark.parametrize("P", [16384 + 5, 300])      # from 16384 pairs its own switch to the ping-pong block (generic fc2 epilogue); 300: 128x128
@pytest.mark.parametrize("regime", REGIMES)
def test_fc2_labels_relu(cases, regime, P):
    lib, L = _lib()
    c = cases(_fc2_case, regime)

    def run(drop, seed=0):
        out = _filled((P + 64, 512), torch.float32)
        assert lib.sgc_fc2_labels_relu(L.ptr(c["h"]), L.ptr(c["w"]), L.ptr(c["b"]), L.ptr(c["ls"]), L.ptr(c["lo"]), L.ptr(c["si"]), L.ptr(c["oi"]),
                                       L.ptr(out), P, drop, seed, L.stream_ptr()) == 0
        torch.cuda.synchronize()
        _assert_untouched(out[P:], "fc2_labels_relu guard rows")
        return out[:P]

    out = run(0)
    ref = c["pre"][:P].clamp(min=0)
    what = "fc2_labels_relu %d pairs" % P
    if regime == "exact":
        _assert_bits(out, ref.float(), what)
    else:
        _assert_close(out, ref, U32, c["accb"][:P], what)
    if regime == "exact":
        _check_dropout(lambda s: run(1, s), out, P, 512, torch.float32, what)
    else:
        _check_dropout(lambda s: run(1, s), out, P, 512, torch.float32, what, ref, U32, c["accb"][:P])


# ------------------------------------------------------------------------------------------------------------ fc2 data gradient
@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("P", [4096 + 37, 300])      # 4133: ping-pong block, nt_epilogue_store16<.., MASK>; 300: 128x128, generic mask epilogue
@pytest.mark.parametrize("regime", REGIMES)
def test_fc2_dgrad(regime, P, scale):
    lib, L = _lib()
    if regime == "exact":
        d = C.exact_operands((P, 512), (-3, -2, -1, 1, 2, 3), 0.5, 1.0, 121)
        w = C.exact_operands((4096, 512), (-3, -2, -1, 1, 2, 3), 1.0, 1.0, 122)
    else:
        d, w = _real((P, 512), 131, "normal", 0.5), _real((4096, 512), 132, "normal", 0.05)
    d, w = d.bfloat16().to(DEV), w.bfloat16().to(DEV)
    # the mask operand: +0, -0, the smallest positive f16 (passes), negatives, ordinary positives
    pats = torch.tensor([0x0000, -0x8000, 0x0001, -0x4400, -0x7FFF, 0x3C00, 0x4100, 0x0400], dtype=torch.int16)
    g = torch.Generator().manual_seed(123)
    h1 = pats[torch.randint(0, len(pats), (P, 4096), generator=g)].to(DEV).view(torch.float16)
    passes = torch.tensor([False, False, True, False, False, True, True, True])
    assert torch.equal((pats.view(torch.float16).float() > 0), passes)
    out = _filled((P + 64, 4096), torch.bfloat16)
    assert lib.sgc_fc2_dgrad(L.ptr(d), L.ptr(w), L.ptr(h1), L.ptr(out), P, ctypes.c_float(scale), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    live = h1.float() > 0
    assert bool((_bits(h1)[live] == 1).any()) and bool((_bits(h1)[~live] == -0x8000).any())
    ref = torch.where(live, d.double() @ w.double().t() * scale, torch.zeros((), dtype=torch.float64, device=DEV))
    what = "fc2_dgrad %d pairs, scale %g" % (P, scale)
    if regime == "exact":
        C.assert_exact(d, w, None)
        assert bool((ref.bfloat16().double() != ref).any())                          # a value that bf16 has to round
        assert bool(((ref == 0) & live).any())                                           # an exact 0 that the mask lets pass
        _assert_bits(out[:P], ref.bfloat16(), what)
    else:
        _assert_close(out[:P], ref, UBF, C.acc_bound(d, w, 512) * scale, what)
    assert bool((_bits(out[:P])[~live] == 0).all()), what + ": a masked output is not +0"
    _assert_untouched(out[P:], what + ": guard rows")


# ------------------------------------------------------------------------------------------------------------ fc1 over window-major rows
TILE_GROUP = [63, 0, 17]


def _grouped_ref(a, wg):
    """Per 256-row tile t: a[t] * (group TILE_GROUP[t] of the weight)^T in float64, and the magnitude sums."""
    ref, mag = [], []
    for t, blk in enumerate(wg):
        at = a[256 * t:256 * (t + 1)].double()
        ref.append(at @ blk.double().t())
        mag.append(at.abs() @ blk.double().abs().t())
    return torch.cat(ref), torch.cat(mag)


def _fc1w_case(regime):
    """ywm [768][1024] f16 and w1p [4096][65536] f16 (zeros, only the three groups' 1024 columns filled), created on the device."""
    if regime == "exact":
        a = C.exact_operands((768, 1024), (1, 2, 3), 0.3, 1.0, 141, device=DEV)
        blocks = [C.exact_operands((4096, 1024), (-30, -3, -2, -1, 1, 2, 3, 30), 1.0, 1.0, 142 + t, device=DEV) for t in range(3)]
    else:
        g = torch.Generator(device=DEV).manual_seed(151)
        a = torch.rand((768, 1024), generator=g, device=DEV) * (torch.rand((768, 1024), generator=g, device=DEV) < 0.5)
        blocks = [torch.randn((4096, 1024), generator=g, device=DEV) * 0.03 for t in range(3)]
    a = a.half()
    blocks = [b.half() for b in blocks]
    w1p = torch.zeros(4096, 65536, dtype=torch.float16, device=DEV)
    for t, grp in enumerate(TILE_GROUP):
        w1p[:, grp * 1024:(grp + 1) * 1024] = blocks[t]
    ref, mag = _grouped_ref(a, blocks)
    if regime == "exact":
        C.assert_exact(a, blocks[0], None, mag=mag)
        assert bool((ref == 0).any()) and bool(((ref.abs() > 2048) & (ref % 2 == 1)).any())
    return dict(a=a, w=w1p, ref=ref, accb=C.acc_bound(None, None, 1024, mag=mag))


@pytest.mark.parametrize("regime", REGIMES)
def test_fc1_windows_gemm(cases, regime):
    """Grouped ping-pong block with the transposed f32 tile (nt_epilogue_f32t): three tiles, each against its own 1024-column group."""
    lib, L = _lib()
    c = cases(_fc1w_case, regime)
    pitch = lib.sgc_fc1_products_pitch()
    assert pitch > 4096
    owm = _filled((768 + 256, pitch), torch.float32)
    assert lib.sgc_fc1_windows_gemm(L.ptr(c["a"]), L.ptr(c["w"]), L.ptr(_i32(TILE_GROUP)), L.ptr(owm), 768, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    if regime == "exact":
        _assert_bits(owm[:768, :4096].contiguous(), c["ref"].float(), "fc1_windows_gemm")
    else:
        _assert_close(owm[:768, :4096], c["ref"], U32, c["accb"], "fc1_windows_gemm")
    _assert_untouched(owm[:768, 4096:], "fc1_windows_gemm: columns behind 4095")
    _assert_untouched(owm[768:], "fc1_windows_gemm: guard rows")


@pytest.mark.parametrize("regime", REGIMES)
def test_fc1_windows_gemm_x16(cases, regime):
    """The same with the rows from goff[group] + n_pseudo on as f16 X rows: first X row 100 inside tile 0 (group 63), 256 = the start of
    tile 1 (group 0), 768 = none in tile 2 (group 17).  f32 rows go to owm only, X rows to oxh only."""
    lib, L = _lib()
    c = cases(_fc1w_case, regime)
    pitch = lib.sgc_fc1_products_pitch()
    n_pseudo = 40
    goff = torch.full((65,), 10 ** 6, dtype=torch.int64)
    goff[63], goff[0], goff[17] = 60, 216, 728
    owm, oxh = _filled((768 + 256, pitch), torch.float32), _filled((768 + 256, 4096), torch.float16)
    assert lib.sgc_fc1_windows_gemm_x16(L.ptr(c["a"]), L.ptr(c["w"]), L.ptr(_i32(TILE_GROUP)), L.ptr(_i32(goff)), n_pseudo, L.ptr(owm), L.ptr(oxh),
                                        768, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    xrow = torch.zeros(768, dtype=torch.bool, device=DEV)
    xrow[100:256] = True
    xrow[256:512] = True
    ref, accb = c["ref"], c["accb"]
    if regime == "exact":
        _assert_bits(owm[:768, :4096][~xrow], ref[~xrow].float(), "fc1_windows_gemm_x16 f32 rows")
        _assert_bits(oxh[:768][xrow], ref[xrow].half(), "fc1_windows_gemm_x16 X rows")
    else:
        _assert_close(owm[:768, :4096][~xrow], ref[~xrow], U32, accb[~xrow], "fc1_windows_gemm_x16 f32 rows")
        _assert_close(oxh[:768][xrow], ref[xrow], U16, accb[xrow], "fc1_windows_gemm_x16 X rows")
    _assert_untouched(owm[:768][xrow], "x16: f32 buffer at the X rows")
    _assert_untouched(oxh[:768][~xrow], "x16: f16 buffer at the per-object rows")
    _assert_untouched(owm[:768, 4096:], "x16: columns behind 4095")
    _assert_untouched(owm[768:], "x16: owm guard rows")
    _assert_untouched(oxh[768:], "x16: oxh guard rows")


@pytest.mark.parametrize("regime", REGIMES)
def test_fc1_windows_dgrad(regime):
    """Grouped ping-pong block, bf16 output through nt_epilogue_store16: gwm [768][4096] x rows g * 1024 .. of w1pT [65536][4096]."""
    lib, L = _lib()
    if regime == "exact":
        a = C.exact_operands((768, 4096), (-3, -2, -1, 1, 2, 3), 0.3, 1.0, 161, device=DEV)
        blocks = [C.exact_operands((1024, 4096), (-3, -2, -1, 1, 2, 3), 1.0, 1.0, 162 + t, device=DEV) for t in range(3)]
    else:
        g = torch.Generator(device=DEV).manual_seed(171)
        a = torch.randn((768, 4096), generator=g, device=DEV) * 0.5
        blocks = [torch.randn((1024, 4096), generator=g, device=DEV) * 0.03 for t in range(3)]
    a = a.bfloat16()
    blocks = [b.bfloat16() for b in blocks]
    wT = torch.zeros(65536, 4096, dtype=torch.bfloat16, device=DEV)
    for t, grp in enumerate(TILE_GROUP):
        wT[grp * 1024:(grp + 1) * 1024] = blocks[t]
    out = _filled((768 + 256, 1024), torch.bfloat16)
    assert lib.sgc_fc1_windows_dgrad(L.ptr(a), L.ptr(wT), L.ptr(_i32(TILE_GROUP)), L.ptr(out), 768, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    ref, mag = _grouped_ref(a, blocks)
    if regime == "exact":
        C.assert_exact(a, blocks[0], None, mag=mag)
        assert bool((ref == 0).any()) and bool((ref.bfloat16().double() != ref).any())
        _assert_bits(out[:768], ref.bfloat16(), "fc1_windows_dgrad")
    else:
        _assert_close(out[:768], ref, UBF, C.acc_bound(None, None, 4096, mag=mag), "fc1_windows_dgrad")
    _assert_untouched(out[768:], "fc1_windows_dgrad: guard rows")
