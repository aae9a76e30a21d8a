"""Every block of the TN GEMM family - the weight gradients (csrc/gemm_tn.h, csrc/gemm_tn_pp_tile.h, csrc/gemm_tn_sp.h) - through the shipped
C ABI, against the float64 references of tests/tn_cases.py.

EXACT regime: small-integer operands for which ``assert_exact`` holds, so every f32 partial sum equals the float64 one: the float64 sum of
the written slabs, cast to f32, is compared bit for bit with the reference.  REAL regime (small shapes only): seeded reals, per element
``|sum of slabs - ref| <= 2**-24 |ref| + acc_bound(K)`` with K the number of contraction rows; no element excluded, the worst err / bound
of each test is printed.  In both: the slab buffer holds one slab more than is written and is pre-filled with 0xFF bytes - every element
of slabs [0, *n_slabs) must be written, everything behind them must keep the fill (that also catches the columns past N = 1152 that the
last tile computes and must not store), and *n_slabs must be the launchers' count (tn_cases.expected_slabs).  Operands the contract says
are not read hold NaN: the ring of the ACONV operands dy3_pad / dU_pad, rows of dy3x / zpatch behind ``rows``, the pitch padding.

Which block and walk a shape reaches (launch_gemm_tn: the 256x256 ping-pong block from M % 256 == 0, tileable N and M * N >= 262144,
else the 128x128 block; the ping-pong schedule has code of its own for 0, 1, 2 and >= 3 K tiles per block and its tail alternates parity):

  sgc_dbg_gemm_tn   128 x 384, pitches M + 8 / N + 8      128x128; K tiles 1 | 3+2 | 2+2+1 (4 asked, 3 written) | 5 x 1 (9 asked)
                    256 x 768 | 256 x 1024                 196608: 128x128, 2 x 6 tiles | 262144: first ping-pong shape; K tiles 1, 2, 3, 5
                    2048 x 256 | 4096 x 2560               ping-pong, xcd_patch walk: 8 x 1 tiles | 16 x 10 tiles (edge patches)
  sgc_dbg_conv_tn   (1, lgS 4, Cin 128, M 128)             128x128, BMODE_CONV, ACONV = 0
                    (2, lgS 5, Cin 128, M 256)             ping-pong, per-lane taps, N = 1152: half-empty last tile
  sgc_conv1_wgrad   128 x 384, 1024 rows                   128x128; 16 x 1 and 6+6+4 K tiles
  sgc_fc2_wgrad     512 x 4096                             ping-pong, super-tile walk 2 x 16; K tiles 1 | 5 x 1 (32 asked) | 3+2
  sgc_fc1_wgrad     4096 x 512 | 4096 x 2560               ping-pong, xcd_patch walk, one split
  sgc_conv2_wgrad   512 x 1152, lgS 5                      ping-pong, BMODE_CONV, ACONV = 1; 16 and 48 K tiles, auto and 5 splits
  sgc_conv3_wgrad   1024 x 4608, lgS 4                     ping-pong, BMODE_CONV, ACONV = 1, xcd_map = 1; K tiles 4 | 8 | 7+7+6
  sgc_windows_wgrad / _patch / _gather                     ping-pong 4 x 18 tiles, BMODE_PLAIN / PATCH / GATHER; K tiles 1, 3, 5 and 1, 2+1, 3+2
  sgc_fc1_windows_wgrad / _rows                            ping-pong, grouped form (goff), 64 groups of 0, 1, 2, 3, 5 K tiles; _rows: AROWS
  sgc_conv3_wgrad_sparse                                   gemm_tn_sp_kernel<0>, walk j / 9; K tiles 4 | 8 | 7+7+6; 512 pairs: xcd_map == 2
  sgc_windows_wgrad_patch_sparse / _gather_sparse          gemm_tn_sp_kernel<1> / <2>; K tiles 1, 1+1, 3, 3+2;
                                                           splits = -1: 2047 K tiles (auto, 7 slabs) | 32 x 64 | 31 x 65 + 38 (xcd_map == 2)

gemm_tn_kernel<.., BMODE_CONV, ACONV = 1, ..> on the 128x128 block is compiled but no shipped entry point reaches it (conv2 and conv3
always tile for the ping-pong block)."""
import ctypes

import pytest
import torch

from tests import nt_epilogue_cases as C
from tests import tn_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
REGIMES = ["exact", "real"]
F16, BF16 = 0, 1
DT = {F16: torch.float16, BF16: torch.bfloat16}
NAN = float("nan")


@pytest.fixture(scope="module")
def cases():
    """Shared operands and float64 references: built once per key, kept on the device, released when the module ends."""
    built = {}

    def get(key, builder):
        if key not in built:
            built[key] = builder()
        return built[key]

    yield get
    built.clear()
    torch.cuda.empty_cache()


def _lib():
    from scene_graph_commonsense_amd import _lib
    return _lib.load(), _lib


def _filled(shape, dtype=torch.float32):
    """A tensor of 0xFF bytes (a NaN no kernel computes in every float type)."""
    n = {2: torch.int16, 4: torch.int32, 1: torch.uint8}[torch.empty((), dtype=dtype).element_size()]
    return torch.full(shape, 255 if n == torch.uint8 else -1, dtype=n, device=DEV).view(dtype)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def _is_fill(t):
    return _bits(t) == (255 if t.element_size() == 1 else -1)


def _assert_untouched(t, what):
    bad = int((~_is_fill(t)).sum())
    assert bad == 0, "%s: %d elements behind the kernel's output were written" % (what, bad)


def _assert_written(t, what):
    bad = int(_is_fill(t).sum())
    assert bad == 0, "%s: %d elements of the output still hold the fill pattern" % (what, bad)


def _assert_bits(got, exp, what):
    """Bit equality of two f32 tensors.  Both sides pass through ``+ 0.0`` first: a float64 BLAS may return -0 for a sum of -0 products,
    an accumulator that starts at +0 never does; nothing else changes."""
    got, exp = got + 0.0, exp.to(got.device) + 0.0
    assert got.shape == exp.shape and got.dtype == exp.dtype, what
    if not torch.equal(_bits(got), _bits(exp)):
        d = _bits(got) != _bits(exp)
        i = d.nonzero()[0].tolist()
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, expected %r"
                             % (what, int(d.sum()), d.numel(), i, got[tuple(i)].item(), exp[tuple(i)].item()))


def _assert_close(got, ref, accb, what, quiet=False):
    """|got - ref| <= 2**-24 |ref| + acc_bound, element by element (got: float64); returns and prints the worst err / bound."""
    ref = ref.to(got.device)
    err = (got - ref).abs()
    bound = 2.0 ** -24 * ref.abs() + accb.to(got.device)
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    worst = float(ratio.max())
    if not quiet:
        print("TN-BLOCKS real regime %-58s worst err/bound = %.4f" % (what, worst))
    assert worst <= 1.0, "%s: worst err / bound = %g" % (what, worst)
    return worst


def _check(regime, total, ref, mag, K, what):
    """total: float64 sum of the written slabs (or the one f32 output as float64)."""
    if regime == "exact":
        _assert_bits(total.float(), ref.float(), what)
    else:
        _assert_close(total, ref, C.acc_bound(None, None, K, mag=mag), what)


def _slabs(call, M, N, nk, splits, tiles, what, sparse=False):
    """Runs ``call(slab pointer, n_slabs pointer)`` on a filled buffer of one slab more than the launcher writes; checks the count, that
    every written slab is written whole and that the rest keeps the fill; returns the float64 sum of the written slabs and the slabs."""
    lib, L = _lib()
    exp = T.expected_slabs(nk, splits, tiles, sparse)
    buf = _filled((exp + 1, M, N))
    ns = ctypes.c_int(-1)
    assert call(L.ptr(buf), ctypes.byref(ns)) == 0, what
    torch.cuda.synchronize()
    assert ns.value == exp, "%s: %d slabs reported, %d expected" % (what, ns.value, exp)
    _assert_written(buf[:exp], what)
    _assert_untouched(buf[exp:], what)
    return buf[:exp].double().sum(0), buf[:exp]


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).to(DEV).contiguous()


def _guarded(t, extra_rows, fill=NAN):
    """``t`` [rows][...] as the head of a buffer with ``extra_rows`` rows of ``fill`` behind it (rows the kernel must not read)."""
    buf = torch.full((t.shape[0] + extra_rows,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
    buf[:t.shape[0]] = t
    return buf


# ------------------------------------------------------------------------------------------------------------ plain products
def _pp(M, N):
    return M % 256 == 0 and N % 256 == 0 and M * N >= 262144


def _plain(regime, elem, M, N, K, splits, seed, pad):
    lib, L = _lib()
    A, B = T.plain_case(regime, K, M, N, DT[elem], seed, DEV)
    mag = T.tn_ref(A.abs(), B.abs())
    if regime == "exact":
        C.assert_exact(A, B, mag=mag)
    Ab = torch.full((K, M + pad), NAN, dtype=DT[elem], device=DEV)
    Bb = torch.full((K, N + pad), NAN, dtype=DT[elem], device=DEV)
    Ab[:, :M], Bb[:, :N] = A, B
    what = "dbg_gemm_tn %s %dx%dx%d splits %d" % ("f16" if elem == F16 else "bf16", M, N, K, splits)
    tiles = (M // 256) * (N // 256) if _pp(M, N) else (M // 128) * (N // 128)
    total, _ = _slabs(lambda c, ns: lib.sgc_dbg_gemm_tn(elem, L.ptr(Ab), L.ptr(Bb), c, M, N, K, ctypes.c_long(M + pad), ctypes.c_long(N + pad),
                                                       splits, ns, L.stream_ptr()), M, N, K // 64, splits, tiles, what)
    _check(regime, total, T.tn_ref(A, B), mag, K, what)


@pytest.mark.parametrize("M,N,K,splits", T.PLAIN_STRIDED)
@pytest.mark.parametrize("elem", [F16, BF16])
@pytest.mark.parametrize("regime", REGIMES)
def test_plain_128_block_strided_operands_and_split_counts(regime, elem, M, N, K, splits):
    _plain(regime, elem, M, N, K, splits, 100 + K + splits, 8)


@pytest.mark.parametrize("M,N,K,splits", T.PLAIN_SIZE_RULE)
@pytest.mark.parametrize("elem", [F16, BF16])
@pytest.mark.parametrize("regime", REGIMES)
def test_plain_both_sides_of_the_size_rule(regime, elem, M, N, K, splits):
    _plain(regime, elem, M, N, K, splits, 120 + K, 0)


@pytest.mark.parametrize("M,N,K,splits", T.PLAIN_WALK)
@pytest.mark.parametrize("elem", [F16, BF16])
def test_plain_ping_pong_xcd_patch_walk(elem, M, N, K, splits):
    _plain("exact", elem, M, N, K, splits, 140, 0)


@pytest.mark.parametrize("n_img,lgS,Cin,M,splits", T.CONV_DBG)
@pytest.mark.parametrize("elem", [F16, BF16])
@pytest.mark.parametrize("regime", REGIMES)
def test_conv_rows_operand(regime, elem, n_img, lgS, Cin, M, splits):
    """ACONV = 0: the gradient as window-major rows, the input as padded maps."""
    lib, L = _lib()
    dy_pad, x_pad = T.conv_case(regime, n_img, lgS, Cin, M, 150 + lgS, DEV)
    dy_pad, x_pad = dy_pad.to(DT[elem]), x_pad.to(DT[elem])
    rows = T.centre_rows(dy_pad, lgS)
    mag = T.conv_wgrad_ref(dy_pad.abs(), x_pad.abs(), lgS)
    if regime == "exact":
        C.assert_exact(rows, x_pad, mag=mag)
    K, N = rows.shape[0], 9 * Cin
    pp = M % 256 == 0 and M * N >= 262144
    tiles = (M // 256) * ((N + 255) // 256) if pp else (M // 128) * (N // 128)
    what = "dbg_conv_tn %s (%d, %d, %d, %d)" % ("f16" if elem == F16 else "bf16", n_img, lgS, Cin, M)
    total, _ = _slabs(lambda c, ns: lib.sgc_dbg_conv_tn(elem, L.ptr(rows), L.ptr(x_pad), c, M, n_img, lgS, Cin, splits, ns, L.stream_ptr()),
                      M, N, K // 64, splits, tiles, what)
    _check(regime, total, T.conv_wgrad_ref(dy_pad, x_pad, lgS), mag, K, what)


@pytest.mark.parametrize("XC,n_rows,splits", T.CONV1)
@pytest.mark.parametrize("regime", REGIMES)
def test_conv1_wgrad(regime, XC, n_rows, splits):
    lib, L = _lib()
    A, B = T.plain_case(regime, n_rows, 128, XC, torch.bfloat16, 200, DEV)
    mag = T.tn_ref(A.abs(), B.abs())
    if regime == "exact":
        C.assert_exact(A, B, mag=mag)
    what = "conv1_wgrad XC %d rows %d splits %d" % (XC, n_rows, splits)
    total, _ = _slabs(lambda c, ns: lib.sgc_conv1_wgrad(L.ptr(A), L.ptr(B), c, n_rows, XC, splits, ns, L.stream_ptr()),
                      128, XC, n_rows // 64, splits, XC // 128, what)
    _check(regime, total, T.tn_ref(A, B), mag, n_rows, what)


@pytest.mark.parametrize("n_rows,splits", T.FC2)
@pytest.mark.parametrize("regime", REGIMES)
def test_fc2_wgrad(regime, n_rows, splits):
    lib, L = _lib()
    A, B = T.plain_case(regime, n_rows, 512, 4096, torch.bfloat16, 210, DEV)
    mag = T.tn_ref(A.abs(), B.abs())
    if regime == "exact":
        C.assert_exact(A, B, mag=mag)
    what = "fc2_wgrad rows %d splits %d" % (n_rows, splits)
    total, _ = _slabs(lambda c, ns: lib.sgc_fc2_wgrad(L.ptr(A), L.ptr(B), c, n_rows, splits, ns, L.stream_ptr()),
                      512, 4096, n_rows // 64, splits, 32, what)
    _check(regime, total, T.tn_ref(A, B), mag, n_rows, what)


@pytest.mark.parametrize("n_rows,cols", T.FC1)
@pytest.mark.parametrize("regime", REGIMES)
def test_fc1_wgrad(regime, n_rows, cols):
    lib, L = _lib()
    A, B = T.plain_case(regime, n_rows, 4096, cols, torch.bfloat16, 220, DEV)
    mag = T.tn_ref(A.abs(), B.abs())
    if regime == "exact":
        C.assert_exact(A, B, mag=mag)
    what = "fc1_wgrad rows %d columns %d" % (n_rows, cols)
    dw = _filled((4096 + 8, cols))
    assert lib.sgc_fc1_wgrad(L.ptr(A), L.ptr(B), L.ptr(dw), n_rows, cols, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    _assert_written(dw[:4096], what)
    _assert_untouched(dw[4096:], what)
    _check(regime, dw[:4096].double(), T.tn_ref(A, B), mag, n_rows, what)


# ------------------------------------------------------------------------------------------------------------ convolutions, ACONV = 1
@pytest.mark.parametrize("n_obj,splits", T.CONV2)
@pytest.mark.parametrize("regime", REGIMES)
def test_conv2_wgrad(cases, regime, n_obj, splits):
    lib, L = _lib()

    def build():
        dU, a = T.conv_case(regime, n_obj, 5, 128, 512, 310, DEV)
        return dU, a, T.conv_wgrad_ref(dU, a, 5), T.conv_wgrad_ref(dU.abs(), a.abs(), 5)

    dU, a, ref, mag = cases(("conv2", regime, n_obj), build)
    assert bool(torch.isnan(dU[:, 0].float()).all()) and bool(torch.isnan(dU[:, :, 33].float()).all())
    if regime == "exact":
        C.assert_exact(dU[:, 1:-1, 1:-1], a, mag=mag)
    what = "conv2_wgrad %d objects splits %d" % (n_obj, splits)
    total, _ = _slabs(lambda c, ns: lib.sgc_conv2_wgrad(L.ptr(dU), L.ptr(a), c, n_obj, splits, ns, L.stream_ptr()),
                      512, 1152, n_obj * 16, splits, 10, what)
    _check(regime, total, ref, mag, n_obj * 1024, what)


def _conv3(cases, regime, n_pairs):
    def build():
        c = T.conv3_pairs_case(regime, n_pairs, 320 + n_pairs, DEV)
        c["ref"] = T.list_wgrad_ref(c["dy"], c["code"], c["gather"], c["dest"], c["z"])
        c["mag"] = T.list_mag(c)
        return c

    c = cases(("conv3", regime, n_pairs), build)
    if regime == "exact":
        C.assert_exact(c["dy"], c["z"], mag=c["mag"])
    return c


@pytest.mark.parametrize("n_pairs,splits", T.CONV3)
@pytest.mark.parametrize("regime", REGIMES)
def test_conv3_wgrad(cases, regime, n_pairs, splits):
    lib, L = _lib()
    c = _conv3(cases, regime, n_pairs)
    dy3 = T.unpooled_pad(c)                                                      # NaN ring
    what = "conv3_wgrad %d pairs splits %d" % (n_pairs, splits)
    total, _ = _slabs(lambda s, ns: lib.sgc_conv3_wgrad(L.ptr(dy3), L.ptr(c["z"]), s, n_pairs, splits, ns, L.stream_ptr()),
                      T.M3, T.N3, n_pairs * 4, splits, 72, what)
    _check(regime, total, c["ref"], c["mag"], n_pairs * 256, what)


def _packs(n_tiles, fill=False):
    if fill:
        return _filled((n_tiles * 65536,), torch.uint8), _filled((n_tiles * 8192,), torch.uint8)
    return torch.empty(n_tiles * 65536, dtype=torch.uint8, device=DEV), torch.empty(n_tiles * 8192, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("n_pairs,splits", T.CONV3)
@pytest.mark.parametrize("regime", REGIMES)
def test_conv3_wgrad_sparse(cases, regime, n_pairs, splits):
    lib, L = _lib()
    c = _conv3(cases, regime, n_pairs)
    ac, ic = _packs(n_pairs * 4)
    what = "conv3_wgrad_sparse %d pairs splits %d" % (n_pairs, splits)
    total, sl = _slabs(lambda s, ns: lib.sgc_conv3_wgrad_sparse(L.ptr(c["dy"]), L.ptr(c["code"]), L.ptr(c["z"]), L.ptr(ac), L.ptr(ic), s,
                                                                n_pairs, splits, ns, L.stream_ptr()),
                       T.M3, T.N3, n_pairs * 4, splits, 72, what, sparse=True)
    _check(regime, total, c["ref"], c["mag"], n_pairs * 256, what)
    # the operand packed by the fused un-pool pass, dy = NULL: the same bits
    ac2, ic2 = _packs(n_pairs * 4)
    bpart = torch.zeros(768, 1024, device=DEV)
    nparts = ctypes.c_int(0)
    assert lib.sgc_unpool_relu_bwd_pack(L.ptr(c["dy"]), L.ptr(c["code"]), None, L.ptr(bpart), ctypes.byref(nparts), L.ptr(ac2), L.ptr(ic2),
                                        n_pairs, L.stream_ptr()) == 0
    _, sl2 = _slabs(lambda s, ns: lib.sgc_conv3_wgrad_sparse(None, None, L.ptr(c["z"]), L.ptr(ac2), L.ptr(ic2), s, n_pairs, splits, ns,
                                                             L.stream_ptr()),
                    T.M3, T.N3, n_pairs * 4, splits, 72, what + " (packed operand)", sparse=True)
    assert torch.equal(ac2, ac) and torch.equal(ic2, ic)
    assert torch.equal(_bits(sl2), _bits(sl))


# ------------------------------------------------------------------------------------------------------------ window lists, dense blocks
def _list(cases, regime, E, f16=False):
    def build():
        if f16 and regime == "exact":
            c = T.list_case(regime, E, 500 + E, DEV, z_dtype=torch.float16, z_values=T.F16_TIES + (257, 300, 1025, 1999))
        else:
            c = T.list_case(regime, E, 400 + E, DEV, z_dtype=torch.float16 if f16 else torch.bfloat16)
        c["zb"] = c["z"].to(torch.bfloat16)                                      # the operand the products see
        c["ref"] = T.list_wgrad_ref(c["dy"], c["code"], c["gather"], c["dest"], c["z"])
        c["mag"] = T.list_wgrad_ref(c["dy"].abs(), c["code"], c["gather"], c["dest"], c["zb"].abs())
        c["n"] = _i32([E])
        return c

    c = cases(("list", regime, E, f16), build)
    if regime == "exact":
        C.assert_exact(c["dy"], c["zb"], mag=c["mag"])
    return c


def _im2patch(c, E, f16, guard=16):
    """zpatch [E + guard][16][512] bf16 by the step's own copy kernel, NaN behind the E entries; checked against the listed patches."""
    lib, L = _lib()
    zp = torch.full((E + guard, 16, T.CIN3), NAN, dtype=torch.bfloat16, device=DEV)
    fn = lib.sgc_windows_im2patch_f16 if f16 else lib.sgc_windows_im2patch
    assert fn(L.ptr(c["z"]), L.ptr(c["gather"]), L.ptr(c["n"]), E, L.ptr(zp), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    want = T.list_patches(c["gather"][:E], c["z"]).to(torch.bfloat16).reshape(E, 16, T.CIN3)
    assert torch.equal(_bits(zp[:E]), _bits(want)) and bool(torch.isnan(zp[E:].float()).all())
    return zp


@pytest.mark.parametrize("rows", T.LIST_ROWS)
@pytest.mark.parametrize("form", ["plain", "patch", "gather"])
@pytest.mark.parametrize("regime", REGIMES)
def test_windows_wgrad_dense_forms(cases, regime, form, rows):
    lib, L = _lib()
    E = rows // 4
    c = _list(cases, regime, E)
    dy3x = _guarded(T.unpool_rows(c["dy"][c["dest"].long()], c["code"][c["gather"].long()]), 64)      # NaN rows behind ``rows``
    if form == "plain":
        zcol = _guarded(T.zcol_rows(c["gather"], c["z"]), 64)
        call = lambda s, ns, sp: lib.sgc_windows_wgrad(L.ptr(dy3x), L.ptr(zcol), s, rows, sp, ns, L.stream_ptr())
    elif form == "patch":
        zp = _im2patch(c, E, False)
        call = lambda s, ns, sp: lib.sgc_windows_wgrad_patch(L.ptr(dy3x), L.ptr(zp), s, rows, sp, ns, L.stream_ptr())
    else:
        call = lambda s, ns, sp: lib.sgc_windows_wgrad_gather(L.ptr(dy3x), L.ptr(c["z"]), L.ptr(c["gather"]), s, rows, sp, ns, L.stream_ptr())
    for splits in (0, 2):
        what = "windows_wgrad %s rows %d splits %d" % (form, rows, splits)
        total, _ = _slabs(lambda s, ns: call(s, ns, splits), T.M3, T.N3, rows // 64, splits, 72, what)
        _check(regime, total, c["ref"], c["mag"], rows, what)


@pytest.mark.parametrize("entry", ["plain", "rows"])
@pytest.mark.parametrize("regime", REGIMES)
def test_fc1_windows_wgrad_grouped(cases, regime, entry):
    """Both grouped entries against the float64 product of every group; the empty groups (first, last and every fifth) come out as zeros."""
    lib, L = _lib()
    c = cases(("grouped", regime), lambda: T.grouped_case(regime, 600, DEV))
    dw = _filled((4096 + 1, 65536))
    if entry == "plain":
        st = lib.sgc_fc1_windows_wgrad(L.ptr(c["gwm"]), L.ptr(c["ywm"]), L.ptr(c["goff"]), L.ptr(dw), c["rows"], L.stream_ptr())
    else:
        st = lib.sgc_fc1_windows_wgrad_rows(L.ptr(c["gsrc"]), L.ptr(c["rowsrc"]), c["gsrc"].shape[0], L.ptr(c["ywm"]), L.ptr(c["goff"]), L.ptr(dw),
                                            c["rows"], L.stream_ptr())
    assert st == 0
    torch.cuda.synchronize()
    what = "fc1_windows_wgrad%s" % ("_rows" if entry == "rows" else "")
    _assert_written(dw[:4096], what)
    _assert_untouched(dw[4096:], what)
    sizes, worst = T.group_sizes(), 0.0
    for g, ref in T.grouped_ref(c["gwm"], c["ywm"], c["goff"]):
        got = dw[:4096, g * 1024:(g + 1) * 1024]
        if sizes[g] == 0:
            assert not bool(_bits(got).any()), "%s: empty group %d is not exact zeros" % (what, g)
            continue
        g0 = int(c["goff"][g])
        A, B = c["gwm"][g0:g0 + sizes[g]], c["ywm"][g0:g0 + sizes[g]]
        mag = T.tn_ref(A.abs(), B.abs())
        if regime == "exact":
            C.assert_exact(A, B, mag=mag)
            _assert_bits(got.contiguous(), ref.float(), "%s group %d" % (what, g))
        else:
            worst = max(worst, _assert_close(got.double(), ref, C.acc_bound(None, None, sizes[g], mag=mag), "%s group %d" % (what, g), quiet=True))
    if regime == "real":
        print("TN-BLOCKS real regime %-58s worst err/bound = %.4f" % (what + " (all groups)", worst))


# ------------------------------------------------------------------------------------------------------------ window lists, sparse block
def _sparse_call(name, c, E, z_or_patch, ac, ic, splits):
    lib, L = _lib()
    fn = getattr(lib, name)
    return lambda s, ns: fn(L.ptr(c["dy"]), L.ptr(c["code"]), L.ptr(c["gather"]), L.ptr(c["dest"]), E, L.ptr(z_or_patch), L.ptr(ac), L.ptr(ic),
                            s, splits, ns, L.stream_ptr())


@pytest.mark.parametrize("n_entries,splits", T.SPARSE_ENTRIES)
@pytest.mark.parametrize("regime", REGIMES)
def test_windows_wgrad_patch_sparse(cases, regime, n_entries, splits):
    E = n_entries
    c = _list(cases, regime, E)
    assert all(bool((c["code"][c["gather"].long()] == q).any()) for q in range(5)) and bool((c["code"][c["gather"].long()] > 4).any())
    zp = _im2patch(c, E, False)
    ac, ic = _packs(E // 16)
    what = "windows_wgrad_patch_sparse %d entries splits %d" % (E, splits)
    total, _ = _slabs(_sparse_call("sgc_windows_wgrad_patch_sparse", c, E, zp, ac, ic, splits), T.M3, T.N3, E // 16, splits, 72, what, sparse=True)
    _check(regime, total, c["ref"], c["mag"], 4 * E, what)


def test_windows_wgrad_sparse_refuses_a_list_that_is_no_multiple_of_16():
    lib, L = _lib()
    c = T.list_case("exact", 32, 432, DEV)
    zp = torch.zeros(32, 16, T.CIN3, dtype=torch.bfloat16, device=DEV)
    for name, second in (("sgc_windows_wgrad_patch_sparse", zp), ("sgc_windows_wgrad_gather_sparse", c["z"].half())):
        ac, ic = _packs(2, fill=True)
        sl = _filled((2, T.M3, T.N3))
        ns = ctypes.c_int(-1)
        assert _sparse_call(name, c, 24, second, ac, ic, 1)(L.ptr(sl), ctypes.byref(ns)) == 1          # SGC_ERR_ARG
        torch.cuda.synchronize()
        for t in (sl, ac, ic):
            _assert_untouched(t, name + " with 24 entries")


@pytest.mark.parametrize("n_entries,splits", T.SPARSE_ENTRIES)
@pytest.mark.parametrize("regime", REGIMES)
def test_windows_wgrad_gather_sparse(cases, regime, n_entries, splits):
    """f16 maps, converted in registers.  EXACT: the maps hold integers of [257, 2047] that bf16 cannot hold, ties included; the reference
    rounds them with torch.  And the documented contract: the same bits as sgc_windows_im2patch_f16 + sgc_windows_wgrad_patch_sparse."""
    E = n_entries
    c = _list(cases, regime, E, f16=True)
    if regime == "exact":
        assert not torch.equal(c["zb"].float(), c["z"].float())
    ac, ic = _packs(E // 16)
    what = "windows_wgrad_gather_sparse %d entries splits %d" % (E, splits)
    total, sl = _slabs(_sparse_call("sgc_windows_wgrad_gather_sparse", c, E, c["z"], ac, ic, splits), T.M3, T.N3, E // 16, splits, 72, what,
                       sparse=True)
    _check(regime, total, c["ref"], c["mag"], 4 * E, what)
    zp = _im2patch(c, E, True)
    ac2, ic2 = _packs(E // 16)
    _, sl2 = _slabs(_sparse_call("sgc_windows_wgrad_patch_sparse", c, E, zp, ac2, ic2, splits), T.M3, T.N3, E // 16, splits, 72,
                    what + " (patch copy)", sparse=True)
    assert torch.equal(ac2, ac) and torch.equal(ic2, ic) and torch.equal(_bits(sl2), _bits(sl))


# ------------------------------------------------------------------------------------------------------------ long K: splits = -1 (EXACT only)
def _long(cases):
    def build():
        n = max(T.LONG_ENTRIES)
        c = T.long_list_case(n, 700, DEV)
        T.long_exact(c, n)
        c["n"] = _i32([n])
        refs, acc, e0 = {}, 0.0, 0
        for e1 in T.LONG_ENTRIES:                                                # integer sums: the prefixes add up exactly
            acc = acc + T.list_wgrad_ref(c["dy"], c["code"], c["gather"][e0:e1], c["dest"][e0:e1], c["z"])
            refs[e1], e0 = acc.float(), e1
        c["refs"] = refs
        c["zpatch"] = _im2patch(c, n, True)
        return c

    return cases("long", build)


@pytest.mark.parametrize("n_entries", T.LONG_ENTRIES)
@pytest.mark.parametrize("entry", ["patch", "gather"])
def test_windows_wgrad_sparse_k_ranges_per_xcd(cases, entry, n_entries):
    """splits = -1 on both sides of the threshold of 2048 K tiles: 2047 (as splits = 0), 32 x 64 and 31 x 65 + 38 K tiles."""
    c = _long(cases)
    E = n_entries
    ac, ic = _packs(E // 16)
    name, second = ("sgc_windows_wgrad_patch_sparse", c["zpatch"]) if entry == "patch" else ("sgc_windows_wgrad_gather_sparse", c["z"])
    what = "%s %d entries splits -1" % (name, E)
    total, _ = _slabs(_sparse_call(name, c, E, second, ac, ic, -1), T.M3, T.N3, E // 16, -1, 72, what, sparse=True)
    _assert_bits(total.float(), c["refs"][E], what)


def test_conv3_wgrad_sparse_k_ranges_per_xcd():
    lib, L = _lib()
    P = T.LONG_PAIRS
    c = T.conv3_pairs_case("exact", P, 800, DEV)
    T.long_exact(c, P * 64)
    ref = T.list_wgrad_ref(c["dy"], c["code"], c["gather"], c["dest"], c["z"]).float()
    ac, ic = _packs(P * 4)
    what = "conv3_wgrad_sparse %d pairs splits -1" % P
    total, _ = _slabs(lambda s, ns: lib.sgc_conv3_wgrad_sparse(L.ptr(c["dy"]), L.ptr(c["code"]), L.ptr(c["z"]), L.ptr(ac), L.ptr(ic), s, P, -1, ns,
                                                               L.stream_ptr()), T.M3, T.N3, P * 4, -1, 72, what, sparse=True)
    _assert_bits(total.float(), ref, what)


# ------------------------------------------------------------------------------------------------------------ distant operands (EXACT only)
FAR_MAPS = 6480                      # maps of 18 * 18 * 512 two-byte values: map 6473 ends beyond 2 GiB, the listed far windows lie in 6474 .. 6479


def _far_maps(dtype, seed):
    """~2.2 GB of zero maps with integers in maps 0 .. 2 and 6474 .. 6479; a list of 48 entries: 16 near, 16 whose gradient is zero, 16 far."""
    z = torch.zeros(FAR_MAPS, 18, 18, T.CIN3, dtype=dtype, device=DEV)
    assert z.numel() * 2 > 2 ** 31 and 6474 * 18 * 18 * T.CIN3 * 2 > 2 ** 31
    near, far = [0, 1, 2], list(range(6474, 6480))
    live = torch.tensor(near + far, device=DEV)
    z[live, 1:17, 1:17] = C.exact_operands((9, 16, 16, T.CIN3), (1, 2, 3), 0.5, 1.0, seed).to(dtype).to(DEV)
    g = torch.Generator().manual_seed(seed + 1)
    w = torch.randint(0, 64, (48,), generator=g)
    w[32:36] = torch.tensor([0, 7, 56, 63])
    maps = torch.cat([torch.tensor(near)[torch.randint(0, 3, (16,), generator=g)], torch.zeros(16, dtype=torch.int64),
                      torch.tensor(far)[torch.randint(0, 6, (16,), generator=g)]])
    maps[47] = 6479
    w[47] = 63                                                                   # the last window of the last map
    return z, (maps * 64 + w).to(torch.int32).to(DEV)


def test_windows_wgrad_gather_with_windows_beyond_2_gib():
    lib, L = _lib()
    z, gather = _far_maps(torch.bfloat16, 900)
    dy3x = C.exact_operands((192, T.M3), (-3, -2, -1, 1, 2, 3), 0.5, 1.0, 902).to(torch.bfloat16).to(DEV)
    dy3x[64:128] = 0
    zcol = T.zcol_rows(gather, z)
    mag = T.tn_ref(dy3x.abs(), zcol.abs())
    C.assert_exact(dy3x, zcol, mag=mag)
    ref = T.tn_ref(dy3x, zcol)
    far_only = T.tn_ref(dy3x[128:], zcol[128:])
    assert bool(far_only.any())
    dy3x = _guarded(dy3x, 64)
    what = "windows_wgrad_gather, windows beyond 2 GiB"
    total, _ = _slabs(lambda s, ns: lib.sgc_windows_wgrad_gather(L.ptr(dy3x), L.ptr(z), L.ptr(gather), s, 192, 1, ns, L.stream_ptr()),
                      T.M3, T.N3, 3, 1, 72, what)
    _assert_bits(total.float(), ref.float(), what)


def test_windows_wgrad_gather_sparse_with_windows_beyond_2_gib():
    z, gather = _far_maps(torch.float16, 910)
    dy = C.exact_operands((40, T.M3), (-3, -2, -1, 1, 2, 3), 0.5, 1.0, 912).to(torch.bfloat16).to(DEV)
    dy[39] = 0                                                                   # the zero gradient row of the 16 middle entries
    g = torch.Generator().manual_seed(913)
    dest = torch.randint(0, 39, (48,), generator=g, dtype=torch.int32)
    dest[16:32] = 39
    code = torch.zeros(FAR_MAPS * 64, T.M3, dtype=torch.uint8, device=DEV)
    code[gather.long()] = T.codes((48, T.M3), 914).to(DEV)
    c = dict(dy=dy, code=code, gather=gather, dest=dest.to(DEV), z=z)
    ref = T.list_wgrad_ref(dy, code, gather, c["dest"], z)
    C.assert_exact(dy, z, mag=T.list_wgrad_ref(dy.abs(), code, gather, c["dest"], z.abs()))
    assert bool(T.list_wgrad_ref(dy, code, gather[32:], c["dest"][32:], z).any())
    ac, ic = _packs(3)
    what = "windows_wgrad_gather_sparse, windows beyond 2 GiB"
    total, _ = _slabs(_sparse_call("sgc_windows_wgrad_gather_sparse", c, 48, z, ac, ic, 1), T.M3, T.N3, 3, 1, 72, what, sparse=True)
    _assert_bits(total.float(), ref.float(), what)


FAR_ENTRIES = 131072 + 32            # zpatch entries of 16 KiB: entry 131072 starts at 2 GiB


def _far_patch_case(cases):
    """A list of 131104 entries over a few maps; only the first and the last 16 entries have a gradient (the others: the zero row 39)."""
    def build():
        c = T.long_list_case(FAR_ENTRIES, 920, DEV, n_maps=8, n_rows=40)
        c["dy"][39] = 0
        c["dest"][16:FAR_ENTRIES - 16] = 39
        c["dest"][:16] = _i32(list(range(16)))
        c["dest"][FAR_ENTRIES - 16:] = _i32(list(range(16, 32)))
        c["n"] = _i32([FAR_ENTRIES])
        live = torch.cat([torch.arange(16), torch.arange(FAR_ENTRIES - 16, FAR_ENTRIES)]).to(DEV)
        ga, de = c["gather"][live], c["dest"][live]
        c["ref"] = T.list_wgrad_ref(c["dy"], c["code"], ga, de, c["z"])
        C.assert_exact(c["dy"], c["z"], mag=T.list_wgrad_ref(c["dy"].abs(), c["code"], ga, de, c["z"].abs()))
        assert bool(T.list_wgrad_ref(c["dy"], c["code"], ga[16:], de[16:], c["z"]).any())
        c["live"] = live
        return c

    return cases("far patch", build)


def _far_zpatch(c, f16):
    """zpatch [131104 + 16][16][512] bf16 (2.0 GiB + 768 KiB) by the copy kernel, NaN behind; the far entries checked against the maps."""
    lib, L = _lib()
    zp = torch.full((FAR_ENTRIES + 16, 16, T.CIN3), NAN, dtype=torch.bfloat16, device=DEV)
    z = c["z"] if f16 else c["z"].to(torch.bfloat16)
    fn = lib.sgc_windows_im2patch_f16 if f16 else lib.sgc_windows_im2patch
    assert fn(L.ptr(z), L.ptr(c["gather"]), L.ptr(c["n"]), FAR_ENTRIES, L.ptr(zp), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert zp[:FAR_ENTRIES].numel() * 2 > 2 ** 31
    want = T.list_patches(c["gather"][c["live"]], c["z"]).to(torch.bfloat16).reshape(32, 16, T.CIN3)
    assert torch.equal(_bits(zp[c["live"]]), _bits(want))
    return zp


def test_windows_wgrad_patch_sparse_with_patches_beyond_2_gib(cases):
    c = _far_patch_case(cases)
    zp = _far_zpatch(c, True)
    ac, ic = _packs(FAR_ENTRIES // 16)
    what = "windows_wgrad_patch_sparse, patches beyond 2 GiB"
    total, _ = _slabs(_sparse_call("sgc_windows_wgrad_patch_sparse", c, FAR_ENTRIES, zp, ac, ic, 0), T.M3, T.N3, FAR_ENTRIES // 16, 0, 72, what,
                      sparse=True)
    _assert_bits(total.float(), c["ref"].float(), what)


def test_windows_wgrad_patch_with_patches_beyond_2_gib(cases):
    lib, L = _lib()
    c = _far_patch_case(cases)
    zp = _far_zpatch(c, False)
    rows = 4 * FAR_ENTRIES
    dy3x = torch.zeros(rows + 64, T.M3, dtype=torch.bfloat16, device=DEV)
    dy3x[rows:] = NAN
    live = c["live"]
    un = T.unpool_rows(c["dy"][c["dest"][live].long()], c["code"][c["gather"][live].long()]).view(32, 4, T.M3)
    dy3x[:rows].view(FAR_ENTRIES, 4, T.M3)[live] = un
    what = "windows_wgrad_patch, patches beyond 2 GiB"
    total, _ = _slabs(lambda s, ns: lib.sgc_windows_wgrad_patch(L.ptr(dy3x), L.ptr(zp), s, rows, 0, ns, L.stream_ptr()),
                      T.M3, T.N3, rows // 64, 0, 72, what)
    _assert_bits(total.float(), c["ref"].float(), what)
