"""The per-pair step kernels of csrc/kernels_fwd.hip and csrc/kernels_bwd.hip (and sgc_slab_sum_ld of csrc/kernels_scene.hip), each on
its own launch through the shipped C ABI, against the definitional float64 / int64 references of tests/step_glue_cases.py
(tests/test_step_glue_cases_cpu.py proves those against torch's max_pool2d, float64 autograd, torch.optim.SGD and as_strided).

EXACT regime: small-integer or power-of-two operands for which ``G.assert_exact`` holds; every output must equal, bit for bit, the exact
result rounded once (RNE) to the output type.  REAL regime: seeded reals, per element |got - ref| <= u_out |ref| + n 2**-24 sum |terms|
with n the number of f32 roundings on the documented path to the element (stated at each check), no element excluded, the worst
got / bound printed (pytest -s).  The expansion is bit-exact in BOTH regimes: its operands are confined so that u + v is exact in f32.
Every output buffer is pre-filled with 0xFF bytes and one row / pair / slab longer than the kernel owns; what the header documents as
unwritten (halos, pixels outside a rectangle, skipped pairs, gaps between rows, the guard) must keep the fill; operand rows the kernel
must not read hold NaN.  A digest of every checked output is kept per (regime, case): a second run in the same process
(pytest FILE FILE --keep-duplicates) must give the same bits.

Which test reaches which entry point and branch:

  test_pair_expand_lists                  sgc_pair_expand (out_elem 0, 1),   one wavefront per (pair, window); 472 pairs; planted 2- and 4-way
                                          sgc_pair_expand_train              ties, four negative sums, u = -v (+0), u = v = -0 (bits 0x0000,
                                                                             code 4); z f16 / z bf16 / amz alone, together, each NULL; halo kept
  test_pair_expand_dense                  sgc_pair_expand_dense,             pair_expand_dense_kernel (pixel_rect NULL): images of 70, 0, 17
                                          sgc_pair_expand_dense_windows      objects, 5 object tiles, pid -1 (diagonal, a whole subject row):
                                                                             skipped pairs keep the fill.  pair_expand_dense_list_kernel
                                                                             (pixel_rect given): second 64-subject chunk with re-used LDS
                                                                             lists, chunks with nothing live (tiles 1 .. 3; pixels where only
                                                                             the other chunk is live), fewer than eight live items (empty
                                                                             eighths), v_max3 + equality-chain routes on every planted tie and
                                                                             zero; rectangles full / one pixel / strip / none; outside: fill.
                                                                             Same bits from all four entry points (one expectation)
  test_pair_contract                      sgc_pair_contract                  lists of 0, 1, 3, 4, 5, 8, 9, 13 pairs (four per trip + remainder),
                                                                             shared pairs, both nibbles, codes 0 .. 4, m3 row mapping (every dz
                                                                             row distinct), empty list: zeros, halo kept
  test_unpool_relu_bwd                    sgc_unpool_relu_bwd                1, 2, 65 pairs (65: second trip of the 2048-block sweep), codes
                                                                             0 .. 4, *n_parts, bias partials, rows behind *n_parts kept
  test_object_masked_maps                 sgc_object_masked_maps             4 + 0 + 3 boxes: full, empty, one pixel, four corners, overlaps
  test_object_masked_maps_bwd             sgc_object_masked_maps_bwd,        dA, every row of dcst_part in its documented order, *n_parts,
                                          sgc_slab_sum                       the image without objects: zeros; the slab-summed total
  test_tanh_bwd                           sgc_tanh_bwd                       n = 1, 255, 256, 257, 65536 * 256 + 3 (grid loop wraps)
  test_pack_image_nhwc                    sgc_pack_image_nhwc                HW 64 / 128, (C0, C1) = (256, 1) / (257, 0, f1 NULL), zero padding
  test_convert_f16_bf16                   sgc_convert_f16_bf16               all 65536 patterns, 2049 times (past 8 * 65536 * 256 elements)
  test_slab_sums                          sgc_slab_sum, sgc_slab_sum_ld      1, 7, 8, 9, 16, 17 slabs (eight per trip + remainder), accumulate,
                                                                             n = 1, 255, 257, 65536 * 256 + 1; ld_out > cols: gap kept
  test_column_sums                        sgc_colsum                         f16 / bf16, rows 1 .. 1000, row_blocks 1, 3, > rows (empty blocks:
                                                                             zeros), cols 8, 264 (partial last column block), 4096
  test_segment_sum_rows                   sgc_segment_sum_rows               segments of 0, 1, 2, 65 rows, rows shared between segments
  test_transpose_cast                     sgc_transpose_cast                 three kinds x the two stride sets of the fc1 layouts, 2 x 3 tiles
  test_permute_cast                       sgc_permute_cast                   ndim 1 .. 5, stride -1 from offset 8, dst_off, three kinds,
                                                                             1 048 576 + 5 elements (second trip of the 4096-block grid)
  test_segment_cast                       sgc_segment_cast                   1 and 48 segments, differing dst_ld, 131 072 + 3 elements per
                                                                             segment (second trip of the 512-block grid)
  test_sgd_step_forms                     sgc_sgd_momentum_step,             float4 body / tail n & 3 / scalar kernel of a view offset by one
                                          sgc_sgd_momentum_multi             float; second trips (16384 * 1024 + 4 * 256 + 3, 16384 * 256 + 5,
                                                                             262 144 + 1); 1, 22, 32 tensors, an empty one, first_mask on some;
                                                                             aligned = misaligned = multi, bit for bit, in REAL
  test_head_loss_bwd                      sgc_head_loss_bwd                  hier / flat x penalty NULL / given (zero coefficients) x dp_extra
                                                                             NULL / given x drop_scale 1 / 2; targets in every block and -1,
                                                                             coef_c 0, conn_y 0 / 1, p zero and negative: dpre exactly 0
  test_head_loss_bwd_position_independent sgc_head_loss_bwd                  rows 0 .. 4096 of 4097 pairs (8 wavefronts, three trips) = the
                                                                             bits of a batch of 5 (4 wavefronts)
  test_head_bwd_upstream                  sgc_head_bwd_upstream              g_sup / g_conn / g_hidden each NULL and given, hier and flat
  test_head_wgrad                         sgc_head_wgrad                     (n_pairs, chunk) = (1, 1), (5, 2), (130, 64); column 512 = bias
                                                                             sum; rows of absent outputs: zeros
  test_argument_checks                    nine entry points                  every documented SGC_ERR_ARG, nothing launched
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from tests import shared_glue_cases as G
from tests import step_glue_cases as S
from tests.test_shared_glue_gpu import KEEP, TDT, _assert_fill, _bits, _dev, _filled, _i32, _lib, _ok

pytestmark = pytest.mark.gpu
DEV = "cuda"
REGIMES = ["exact", "real"]
WORST = {}
DIGEST = {}
F, L_ = ctypes.c_float, ctypes.c_long


@pytest.fixture(autouse=True)
def _keep_operands_alive():
    yield
    KEEP.clear()


@pytest.fixture(scope="module")
def cache():
    built = {}

    def get(key, builder):
        if key not in built:
            built[key] = builder()
        return built[key]

    yield get
    built.clear()
    torch.cuda.empty_cache()


def _digest(regime, what, t):
    """Same bits as the first time this (regime, case) ran in this process.  Large tensors: two position-weighted sums on the device."""
    if t.numel() * t.element_size() <= (8 << 20):
        d = zlib.crc32(_bits(t).tobytes())
    else:
        v = t.contiguous().view(-1).view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]).to(torch.int64)
        k = torch.arange(v.numel(), device=v.device, dtype=torch.int64) % 65521 + 1
        d = (int(v.sum()), int((v * k).sum()))
    assert DIGEST.setdefault((regime, what), d) == d, what + ": other bits than the first time in this process"


def _check(regime, t, ref, fmt, what, mag=None, n=None, bound=None):
    """One output tensor against its float64 reference in the regime's way; ``mag`` / ``n``: sum of |terms| and number of f32 roundings;
    ``bound``: an absolute budget worked out by the caller, to which the output format's rounding is added."""
    _digest(regime, what, t)
    if regime == "exact":
        G.assert_exact(mag, what)
        G.check_bits(_bits(t), ref, fmt, what)
        return
    got = t.double().cpu().numpy()
    if bound is None:
        bound = G.real_bound(ref, mag, n, fmt)
    else:
        bound = bound + G.real_bound(ref, 0.0, 0, fmt)
    WORST[what] = G.check_real(got, ref, bound, what, quiet=True)
    print("STEP-GLUE real regime %-70s worst got/bound = %.4f" % (what, WORST[what]))


def _operand(a, fmt, regime):
    t = _dev(a, torch.float64).to(TDT[fmt])
    back = t.double().cpu().numpy()
    if regime == "exact":
        assert np.array_equal(back, a), "operand not representable in " + fmt
    return t, back


def _refill(t):
    t.view(torch.uint8).fill_(255)
    return t


def _harr(ctype, values):
    return (ctype * max(1, len(values)))(*values)


# ================================================================================================================= 1. expansion
C2 = 512


def _expand_case(cache, regime):
    """Operands, tables and the expected bits of every output buffer (fill where nothing is documented to be written)."""
    def build():
        sc = cache(("expand_scene",), S.ExpandScene)
        P = sc.P
        U, V = S.expand_scene_operands(np.random.default_rng(41 if regime == "exact" else 42), sc.n, C2, regime)
        zf = np.full((P + 1, 18, 18, C2), 0xFFFF, dtype=np.uint16)
        zb = np.full((P + 1, 18, 18, C2), 0xFFFF, dtype=np.uint16)
        am = np.full((P + 1, 256, C2 // 2), 0xFF, dtype=np.uint8)
        seen = np.zeros(5, dtype=np.int64)
        for p in range(P):
            z, code = S.expand_reference(U[sc.sub[p]].reshape(256, 4, C2), V[sc.obj[p]].reshape(256, 4, C2))
            assert (z[:, 2:6] == 0).all() and (code[:, 2:6] == 4).all() and (code[:, 0] == 0).all() and (code[:, 1] == 1).all()      # the planted cases
            i, j = int(sc.sub[p]), int(sc.obj[p])
            assert (z[:, S.SIGN[0]] == i).all() and (z[:, S.SIGN[1]] == j).all()                  # the channels that name the pair's two objects
            zf[p, 1:17, 1:17] = G.to_bits(G.rne(z, "f16"), "f16").reshape(16, 16, C2)
            zb[p, 1:17, 1:17] = G.to_bits(G.rne(z, "bf16"), "bf16").reshape(16, 16, C2)
            am[p] = S.pack_nibbles(code)
            seen += np.bincount(code.reshape(-1), minlength=5)
        assert (seen > 0).all()
        assert (zf[:P, 1:17, 1:17, 3:6] == 0).all() and (zb[:P, 1:17, 1:17, 3:6] == 0).all()          # +0 and -0 sums: the bit pattern 0x0000
        live = np.zeros((P + 1, 16, 16), dtype=bool)
        live[:P] = sc.live
        pid = sc.pid
        return dict(sc=sc, U=_dev(U.view(np.int16)).view(torch.float16), V=_dev(V.view(np.int16)).view(torch.float16),
                    zf=_dev(zf.view(np.int16)), zb=_dev(zb.view(np.int16)), am=_dev(am), live=_dev(live), sub=_i32(sc.sub), obj=_i32(sc.obj),
                    pid=_i32(pid), img_ptr=_i32(sc.img_ptr), rect=_i32(sc.pixrect))
    return cache(("expand", regime), build)


def _expand_outputs(cache):
    def build():
        P = cache(("expand_scene",), S.ExpandScene).P
        return dict(zf=_filled((P + 1, 18, 18, C2), torch.int16), zb=_filled((P + 1, 18, 18, C2), torch.int16),
                    am=_filled((P + 1, 256, C2 // 2), torch.uint8))
    return cache(("expand_out",), build)


OUTPUT_FORMS = ["zf", "zb", "am", "zf+zb+am", "zb+am", "zf+am", "zf+zb"]          # each output alone, all together, each NULL form


def _expect(case, name, rect):
    """The expected buffer: the full expansion, or - with rectangles - fill outside every pair's rectangle."""
    full = case[name]
    if not rect:
        return full
    live = case["live"]
    if name == "am":
        m = live.reshape(-1, 256, 1)
        return torch.where(m, full, torch.full_like(full, 255))
    m = torch.zeros(full.shape[:3], dtype=torch.bool, device=DEV)
    m[:, 1:17, 1:17] = live
    return torch.where(m[..., None], full, torch.full_like(full, -1))


def _check_expand(regime, case, outs, given, rect, what):
    for name in ("zf", "zb", "am"):
        if name in given:
            want = _expect(case, name, rect)
            got = outs[name]
            if not torch.equal(got, want):
                bad = (got != want).nonzero()
                k = tuple(int(v) for v in bad[0])
                raise AssertionError("%s %s: %d elements differ, first at %s: got 0x%X, expected 0x%X"
                                     % (what, name, len(bad), k, int(got[k]) & 0xFFFF, int(want[k]) & 0xFFFF))
            _digest(regime, what + " " + name, got)
        else:
            _assert_fill(outs[name], what + " (NULL output " + name + ")")


@pytest.mark.parametrize("form", ["expand_f16", "expand_bf16"] + ["train " + f for f in OUTPUT_FORMS])
@pytest.mark.parametrize("regime", REGIMES)
def test_pair_expand_lists(cache, regime, form):
    L, lib = _lib()
    case, outs = _expand_case(cache, regime), _expand_outputs(cache)
    P = case["sc"].P
    for t in outs.values():
        _refill(t)
    if form.startswith("expand"):
        name, elem = ("zf", 0) if form == "expand_f16" else ("zb", 1)
        _ok(lib.sgc_pair_expand(L.ptr(case["U"]), L.ptr(case["V"]), L.ptr(case["sub"]), L.ptr(case["obj"]), L.ptr(outs[name]), P, elem, L.stream_ptr()),
            "sgc_pair_expand")
        given = [name]
    else:
        given = form.split(" ")[1].split("+")
        ptrs = [L.ptr(outs[k] if k in given else None) for k in ("zf", "zb", "am")]
        _ok(lib.sgc_pair_expand_train(L.ptr(case["U"]), L.ptr(case["V"]), L.ptr(case["sub"]), L.ptr(case["obj"]), *ptrs, P, L.stream_ptr()),
            "sgc_pair_expand_train")
    _check_expand(regime, case, outs, given, False, "pair_" + form)


@pytest.mark.parametrize("form", OUTPUT_FORMS)
@pytest.mark.parametrize("entry", ["dense", "windows_null", "windows_rect"])
@pytest.mark.parametrize("regime", REGIMES)
def test_pair_expand_dense(cache, regime, entry, form):
    L, lib = _lib()
    case, outs = _expand_case(cache, regime), _expand_outputs(cache)
    sc = case["sc"]
    for t in outs.values():
        _refill(t)
    given = form.split("+")
    ptrs = [L.ptr(outs[k] if k in given else None) for k in ("zf", "zb", "am")]
    head = (L.ptr(case["U"]), L.ptr(case["V"]), L.ptr(case["img_ptr"]), L.ptr(case["pid"]), sc.MAX_N, len(sc.SIZES), sc.MAX_N)
    if entry == "dense":
        _ok(lib.sgc_pair_expand_dense(*head, *ptrs, L.stream_ptr()), "sgc_pair_expand_dense")
    else:
        rect = L.ptr(case["rect"] if entry == "windows_rect" else None)
        _ok(lib.sgc_pair_expand_dense_windows(*head, *ptrs, rect, L.stream_ptr()), "sgc_pair_expand_dense_windows")
    _check_expand(regime, case, outs, given, entry == "windows_rect", "pair_expand_%s %s" % (entry, form))


# ================================================================================================================= 2. contraction
@pytest.mark.parametrize("regime", REGIMES)
def test_pair_contract(cache, regime):
    L, lib = _lib()
    rng = np.random.default_rng(51)
    n, P = 12, 18                                                          # pairs 16 and 17 are in no list: NaN gradients, 0xFF codes
    ptr, lst = S.contract_lists(rng, n, n_pairs=16)
    m3 = S.window_major_rows(16).reshape(-1)                                # row of pixel W = 16 Y + X
    rows = G.values(rng, (P + 1, 256, C2), regime, -20, 127)
    if regime == "exact":                                                   # every dz row distinct: channels 0 and 1 spell the row number
        r = np.arange((P + 1) * 256).reshape(P + 1, 256)
        rows[:, :, 0], rows[:, :, 1] = r % 251 - 125, r // 251 - 8
        assert len({(a, b) for a, b in zip(rows[:, :, 0].reshape(-1), rows[:, :, 1].reshape(-1))}) == (P + 1) * 256
    rows[16:] = np.nan
    dz = _dev(rows, torch.float64).to(torch.bfloat16)
    rows = dz.double().cpu().numpy()
    if regime == "exact":
        assert np.array_equal(np.nan_to_num(rows[:16]), np.nan_to_num(rows[:16]).round())
    dzv = rows[:, m3].reshape(P + 1, 16, 16, C2)                           # by (Y, X)
    codes = rng.integers(0, 5, (P + 1, 16, 16, C2)).astype(np.uint8)
    amz = S.pack_nibbles(codes).reshape(P + 1, 256, C2 // 2)
    amz[16:] = 0xFF
    low, high = codes[:16, ..., 0::2], codes[:16, ..., 1::2]
    assert all(((low == a) & (high == b)).any() for a in range(5) for b in range(5))          # both nibbles, independently
    ref, mag, cnt = S.contract_step_reference(np.nan_to_num(dzv), codes, ptr, lst)
    dU = _filled((n + 1, 34, 34, C2), torch.bfloat16)
    _ok(lib.sgc_pair_contract(L.ptr(dz), L.ptr(_dev(amz)), L.ptr(_i32(ptr)), L.ptr(_i32(lst)), L.ptr(dU), n, L.stream_ptr()), "sgc_pair_contract")
    inner = dU[:n, 1:33, 1:33].reshape(n, 16, 2, 16, 2, C2).permute(0, 1, 3, 2, 4, 5).reshape(n, 16, 16, 4, C2)
    if regime == "exact":
        lost, half = G.rounding_cases(ref, "bf16")
        assert lost > 0 and half > 0
    _check(regime, inner, ref, "bf16", "pair_contract", mag=mag, n=cnt)           # n = the list length: one addition per listed pair
    ring = _bits(dU).copy()
    ring[:n, 1:33, 1:33] = 0xFFFF
    assert (ring == 0xFFFF).all(), "halo ring or the map behind was written"
    empty = np.diff(ptr) == 0
    assert empty.sum() == 2 and (_bits(inner)[empty] == 0).all()                  # an empty list: the interior is written as zeros


# ================================================================================================================= 3. un-pool
C3 = 1024


@pytest.mark.parametrize("n_pairs", [1, 2, 65])
@pytest.mark.parametrize("regime", REGIMES)
def test_unpool_relu_bwd(regime, n_pairs):
    L, lib = _lib()
    rng = np.random.default_rng(60 + n_pairs)
    n_win = n_pairs * 64
    dy, dyv = _operand(G.values(rng, (n_win, C3), regime, -20, 127), "bf16", regime)
    code = rng.integers(0, 5, (n_win, C3)).astype(np.uint8)
    dy3 = _filled((n_pairs + 1, 18, 18, C3), torch.bfloat16)
    want_parts = min(2048, 32 * n_pairs)
    part = _filled((2048 + 1, C3), torch.float32)
    n_parts = ctypes.c_int(-1)
    _ok(lib.sgc_unpool_relu_bwd(L.ptr(dy), L.ptr(_dev(code)), L.ptr(dy3), L.ptr(part), ctypes.byref(n_parts), n_pairs, L.stream_ptr()),
        "sgc_unpool_relu_bwd")
    assert n_parts.value == want_parts
    if n_pairs == 65:
        assert n_win > 2 * 2048                                                    # past one sweep of 2048 blocks x 2 windows
    routed = G.unpool(dyv, code)                                                   # [n_win, 4, C]
    want = routed.reshape(n_pairs, 8, 8, 2, 2, C3).transpose(0, 1, 3, 2, 4, 5).reshape(n_pairs, 16, 16, C3)
    G.check_bits(_bits(dy3[:n_pairs, 1:17, 1:17]), want, "bf16", "unpool_relu_bwd dy3 %d" % n_pairs)      # a routed copy: bits in both regimes
    _digest(regime, "unpool_relu_bwd dy3 %d" % n_pairs, dy3)
    halo = _bits(dy3).copy()
    halo[:n_pairs, 1:17, 1:17] = 0xFFFF
    assert (halo == 0xFFFF).all(), "halo or the map behind was written"
    _assert_fill(part[want_parts:], "dbias_part behind *n_parts")
    alive = np.where(code < 4, dyv, 0.0)
    got = part[:want_parts].double().sum(0).cpu().numpy()                          # the partials are f32; their float64 sum is exact enough
    per_part = -(-n_win // (2 * want_parts)) + 1                                   # additions behind one partial: its windows of either half + 1
    ref, mag = alive.sum(0), np.abs(alive).sum(0)
    _digest(regime, "unpool_relu_bwd parts %d" % n_pairs, part[:want_parts])
    if regime == "exact":
        G.assert_exact(mag, "unpool bias")
        assert np.array_equal(got, ref)
    else:
        what = "unpool_relu_bwd bias %d" % n_pairs
        WORST[what] = G.check_real(got, ref, per_part * 2.0 ** -24 * mag + 1e-300, what, quiet=True)
        print("STEP-GLUE real regime %-70s worst got/bound = %.4f" % (what, WORST[what]))


# ================================================================================================================= 4. masks
def test_object_masked_maps():
    L, lib = _lib()
    bb, ptr, obj_img = S.mask_scene()
    n, n_img, Fz, D = len(bb), len(ptr) - 1, 32, 128
    rng = np.random.default_rng(70)
    a = rng.standard_normal((n_img, Fz * Fz, D)).astype(np.float16)
    covered = np.zeros((n_img, Fz * Fz), dtype=bool)
    for o in range(n):
        covered[obj_img[o]] |= S.box_mask(bb[o:o + 1])[0].reshape(-1)
    a[~covered] = np.nan                                                            # pixels no box holds (all of image 1) are never read
    assert np.isnan(a[1]).all() and np.isnan(a[2]).any() and not np.isnan(a[0]).any()
    cst = rng.standard_normal(D).astype(np.float16)
    a_pad = _filled((n + 1, Fz + 2, Fz + 2, D), torch.float16)
    _ok(lib.sgc_object_masked_maps(L.ptr(_dev(a.view(np.int16))), L.ptr(_i32(obj_img)), L.ptr(_i32(bb.reshape(-1))), L.ptr(_dev(cst.view(np.int16))),
                                   L.ptr(a_pad), n, Fz, D, L.stream_ptr()), "sgc_object_masked_maps")
    want = S.mask_forward_reference(a.view(np.uint16).reshape(-1, D), obj_img, bb, cst.view(np.uint16))
    assert np.array_equal(_bits(a_pad[:n]), want) and not np.isnan(a_pad[:n].float().cpu().numpy()).any()
    _assert_fill(a_pad[n:], "a_pad")
    _digest("bits", "object_masked_maps", a_pad)


@pytest.mark.parametrize("regime", REGIMES)
def test_object_masked_maps_bwd(regime):
    L, lib = _lib()
    bb, ptr, obj_img = S.mask_scene()
    n, n_img, Fz, D = len(bb), len(ptr) - 1, 32, 128
    rng = np.random.default_rng(71)
    da, dav = _operand(G.values(rng, (n, Fz * Fz, D), regime, -20, 127), "bf16", regime)
    dA = _filled((n_img * Fz * Fz + 1, D), torch.float32)
    part = _filled((n_img * 64 + 1, D), torch.float32)
    n_parts = ctypes.c_int(-1)
    _ok(lib.sgc_object_masked_maps_bwd(L.ptr(da), L.ptr(_i32(ptr)), L.ptr(_i32(bb.reshape(-1))), L.ptr(dA), L.ptr(part), ctypes.byref(n_parts), n_img,
                                       Fz, D, L.stream_ptr()), "sgc_object_masked_maps_bwd")
    assert n_parts.value == n_img * 64
    rA, mA, rp, mp = S.mask_backward_reference(dav, ptr, bb, Fz)
    # dA: one addition per object of the image; a partial: per pixel the image's objects, then the block's 16 pixels
    _check(regime, dA[:-1], rA.reshape(-1, D), "f32", "object_masked_maps_bwd dA", mag=mA.reshape(-1, D), n=4)
    _check(regime, part[:-1], rp, "f32", "object_masked_maps_bwd dcst_part", mag=mp, n=4 + 16)
    _assert_fill(dA[-1:], "dA")
    _assert_fill(part[-1:], "dcst_part")
    assert (_bits(dA[1024:2048]) == 0).all() and (_bits(part[64:128]) == 0).all()          # the image without objects
    tot = _filled((D + 1,), torch.float32)
    _ok(lib.sgc_slab_sum(L.ptr(part), L.ptr(tot), L_(D), n_parts.value, 0, L.stream_ptr()), "sgc_slab_sum")
    _check(regime, tot[:D], rp.sum(0), "f32", "object_masked_maps_bwd dcst total", mag=mp.sum(0), n=20 + n_parts.value)
    _assert_fill(tot[D:], "dcst total")


# ================================================================================================================= 5. element-wise
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65536 * 256 + 3])
@pytest.mark.parametrize("regime", REGIMES)
def test_tanh_bwd(regime, n):
    L, lib = _lib()
    rng = np.random.default_rng(80)
    if regime == "exact":
        t = rng.choice(np.array([0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0]), n)
        d = rng.integers(-1000, 1001, n).astype(np.float64)
    else:
        t = np.tanh(rng.standard_normal(n))
        d = rng.standard_normal(n)
    a, tv = _operand(t, "f16", regime)
    dA, dv = _operand(d, "f32", regime)
    out = _filled((n + 1,), torch.bfloat16)
    _ok(lib.sgc_tanh_bwd(L.ptr(dA), L.ptr(a), L.ptr(out), L_(n), L.stream_ptr()), "sgc_tanh_bwd")
    # three f32 roundings before the bf16 one: t * t, 1 - t^2, the product with dA
    _check(regime, out[:n], S.tanh_bwd_reference(dv, tv), "bf16", "tanh_bwd n = %d" % n, mag=np.abs(dv) * (1.0 + tv * tv), n=3)
    _assert_fill(out[n:], "dpre")


@pytest.mark.parametrize("HW", [64, 128])
@pytest.mark.parametrize("C0,C1", [(256, 1), (257, 0)])
def test_pack_image_nhwc(HW, C0, C1):
    L, lib = _lib()
    rng = np.random.default_rng(81)
    XC, n_img = 384, 2
    f0 = rng.standard_normal((n_img, C0, HW)).astype(np.float32)
    f1 = rng.standard_normal((n_img, C1, HW)).astype(np.float32) if C1 else None
    x = _filled((n_img * HW + 1, XC), torch.float16)
    _ok(lib.sgc_pack_image_nhwc(L.ptr(_dev(f0)), C0, L.ptr(_dev(f1) if C1 else None), C1, L.ptr(x), n_img, HW, XC, L.stream_ptr()),
        "sgc_pack_image_nhwc")
    want = S.pack_image_reference(f0.astype(np.float64), None if f1 is None else f1.astype(np.float64), XC)
    lost, _ = G.rounding_cases(want, "f16")
    assert lost > 0
    G.check_bits(_bits(x[:-1]), want, "f16", "pack_image_nhwc")
    assert (_bits(x[:-1])[:, 257:] == 0).all()                                       # the padding channels
    _assert_fill(x[-1:], "x")
    _digest("bits", "pack_image_nhwc %d %d" % (HW, C0), x)


def test_convert_f16_bf16():
    L, lib = _lib()
    reps = 2049
    n = 65536 * reps
    assert n > 8 * 65536 * 256 and n % 8 == 0                                        # the grid loop of 65536 blocks x 256 threads x 8 wraps
    pat = np.arange(65536, dtype=np.uint16)
    src = _dev(pat.view(np.int16)).repeat(reps)
    out = _filled((n + 8,), torch.int16)
    _ok(lib.sgc_convert_f16_bf16(L.ptr(src), L.ptr(out), L_(n), L.stream_ptr()), "sgc_convert_f16_bf16")
    got = out[:n].view(reps, 65536)
    assert torch.equal(got, got[:1].expand(reps, 65536)), "copies of the same pattern gave different bits"
    _assert_fill(out[n:], "out")
    row = _bits(got[0])
    val = pat.view(np.float16).astype(np.float64)
    fin = ~np.isnan(val)
    want = G.to_bits(G.rne(np.where(fin, val, 0.0), "bf16"), "bf16")
    inf = np.isinf(val)
    want[inf] = np.where(val[inf] > 0, 0x7F80, 0xFF80)
    neg0 = pat == 0x8000
    assert np.array_equal(row[fin & ~neg0], want[fin & ~neg0]) and row[0x8000] == 0x8000
    nan_out = ((row & 0x7F80) == 0x7F80) & ((row & 0x7F) != 0)
    assert nan_out[~fin].all() and not nan_out[fin].any()                            # NaN in, NaN out - and nowhere else
    lost, half = G.rounding_cases(val[fin & ~inf], "bf16")
    assert lost > 0 and half > 0
    _digest("bits", "convert_f16_bf16", got[:2])


# ================================================================================================================= 6. reductions
@pytest.mark.parametrize("regime", REGIMES)
def test_slab_sums(regime):
    L, lib = _lib()
    rng = np.random.default_rng(90)
    shapes = [(s, n, acc) for s in (1, 7, 8, 9, 16, 17) for n in (1, 255, 257) for acc in (0, 1)] + [(2, 65536 * 256 + 1, 0)]
    for slabs, n, acc in shapes:
        x, xv = _operand(G.values(rng, (slabs, n), regime, -1000, 1000, channels_last=False), "f32", regime)
        old, oldv = _operand(G.values(rng, (n,), regime, -1000, 1000), "f32", regime)
        out = _filled((n + 1,), torch.float32)
        if acc:
            out[:n] = old
        _ok(lib.sgc_slab_sum(L.ptr(x), L.ptr(out), L_(n), slabs, acc, L.stream_ptr()), "sgc_slab_sum")
        ref, mag, adds = S.slab_sum_reference(xv, oldv if acc else None)
        _check(regime, out[:n], ref, "f32", "slab_sum %d x %d acc %d" % (slabs, n, acc), mag=mag, n=adds)      # n = one addition per slab (+ the old value)
        _assert_fill(out[n:], "out")
        KEEP.clear()
    for slabs in (1, 8, 9):
        rows, cols, ld = 5, 24, 40
        x, xv = _operand(G.values(rng, (slabs, rows, cols), regime, -1000, 1000), "f32", regime)
        out = _filled((rows * ld + 1,), torch.float32)
        _ok(lib.sgc_slab_sum_ld(L.ptr(x), L.ptr(out), rows, cols, L_(ld), slabs, L.stream_ptr()), "sgc_slab_sum_ld")
        ref, mag, adds = S.slab_sum_reference(xv.reshape(slabs, -1))
        view = out[:rows * ld].view(rows, ld)
        _check(regime, view[:, :cols], ref.reshape(rows, cols), "f32", "slab_sum_ld %d" % slabs, mag=mag.reshape(rows, cols), n=adds)
        _assert_fill(view[:, cols:], "the gap between rows")
        _assert_fill(out[rows * ld:], "out")


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("regime", REGIMES)
def test_column_sums(regime, fmt):
    L, lib = _lib()
    rng = np.random.default_rng(91)
    for rows in (1, 7, 8, 9, 1000):
        for cols in (8, 264, 4096):
            X, Xv = _operand(G.values(rng, (rows, cols), regime, -20, 127), fmt, regime)
            for rb in (1, 3, rows + 5):
                part = _filled((rb + 1, cols), torch.float32)
                _ok(lib.sgc_colsum(0 if fmt == "f16" else 1, L.ptr(X), L.ptr(part), L_(rows), cols, rb, L.stream_ptr()), "sgc_colsum")
                ref, mag, rpb = S.colsum_reference(Xv, rb)
                what = "colsum %s %d x %d / %d" % (fmt, rows, cols, rb)
                _check(regime, part[:rb], ref, "f32", what, mag=mag, n=rpb + 8)          # the block's rows over eight row lanes + their eight sums
                _assert_fill(part[rb:], "part")
                if rb > rows:
                    assert (_bits(part[rows:rb]) == 0).all(), what + ": empty row blocks"
            KEEP.clear()


@pytest.mark.parametrize("regime", REGIMES)
def test_segment_sum_rows(regime):
    L, lib = _lib()
    rng = np.random.default_rng(92)
    n_rows, cols = 70, 512
    X, Xv = _operand(np.concatenate([G.values(rng, (n_rows, cols), regime, -20, 127), np.full((1, cols), np.nan)]), "bf16", "real")
    if regime == "exact":
        assert np.array_equal(Xv[:n_rows], Xv[:n_rows].round())
    cnt = [0, 1, 2, 65, 0, 3]
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    lst = np.concatenate([rng.permutation(n_rows)[:c] for c in cnt]).astype(np.int32)          # rows shared between segments, row 70 (NaN) in none
    assert len(set(lst.tolist())) < len(lst)
    out = _filled((len(cnt) + 1, cols), torch.float32)
    _ok(lib.sgc_segment_sum_rows(L.ptr(X), L.ptr(_i32(ptr)), L.ptr(_i32(lst)), L.ptr(out), len(cnt), cols, L.stream_ptr()), "sgc_segment_sum_rows")
    ref, mag, n = S.segment_sum_reference(np.nan_to_num(Xv), ptr, lst)
    _check(regime, out[:-1], ref, "f32", "segment_sum_rows", mag=mag, n=n)                   # n = the segment's rows
    _assert_fill(out[-1:], "out")
    assert (_bits(out[0]) == 0).all()


# ================================================================================================================= 7. layout casts
def _cast_check(dst, pos, val, kind, what):
    """The named positions hold the RNE cast of the source values, every other element of the destination the fill."""
    fmt = S.CAST_FMT[kind]
    got = _bits(dst)
    G.check_bits(got[pos], val, fmt, what)
    other = np.ones(got.shape, dtype=bool)
    other[pos] = False
    assert (got[other] == np.iinfo(got.dtype).max).all(), what + ": elements between the destination rows were written"
    _digest("bits", what, dst)


def _cast_source(rng, n):
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    v[::17] = rng.integers(-2048, 2048, len(v[::17])) + 0.5                                   # halves of both 16-bit formats
    return v.astype(np.float32)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("strides", [(65536, 64, 1024, 65536, 4096, 64), (65536, 4096, 64, 65536, 64, 1024)])
def test_transpose_cast(kind, strides):
    L, lib = _lib()
    rng = np.random.default_rng(100)
    na, nb, size = 2, 3, 2 * 65536
    src = _cast_source(rng, size)
    pos, val = S.transpose_cast_reference(src, size, na, nb, *strides)
    dst = _filled((size + 1,), TDT[S.CAST_FMT[kind]])
    _ok(lib.sgc_transpose_cast(L.ptr(_dev(src)), L.ptr(dst), kind, na, nb, *[L_(s) for s in strides], L.stream_ptr()), "sgc_transpose_cast")
    _cast_check(dst, pos, val, kind, "transpose_cast kind %d %s" % (kind, strides[1]))


PERMUTES = [   # dims, src strides, dst strides, src_off, dst_off, destination size
    ((7,), (3,), (2,), 1, 5, 20),
    ((5, 9), (9, -1), (11, 1), 8, 2, 60),                                       # a flipped 3 x 3 kernel: stride -1 from offset 8
    ((4, 3, 5), (5, 20, 1), (15, 5, 1), 0, 0, 60),
    ((2, 3, 4, 5), (60, 5, 15, 1), (61, 20, 5, 1), 0, 3, 130),
    ((2, 3, 2, 3, 9), (162, 18, 81, 27, -1), (324, 108, 54, 18, 2), 8, 1, 652),  # ndim 5, flipped taps, every second destination element
    ((1024, 1029), (1, 1024), (1030, 1), 0, 7, 1024 * 1030 + 8),                 # 1 053 696 elements: the second trip of 4096 blocks x 256
]


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("case", range(len(PERMUTES)))
def test_permute_cast(case, kind):
    L, lib = _lib()
    dims, ss, ds, so, do, size = PERMUTES[case]
    rng = np.random.default_rng(101 + case)
    n_src = so + 1 + sum((d - 1) * s for d, s in zip(dims, ss) if s > 0)
    src = _cast_source(rng, n_src)
    pos, val = S.scatter_reference(src, size, dims, ss, ds, so, do)
    if case == len(PERMUTES) - 1:
        assert len(pos) > 1048576
    dst = _filled((size + 1,), TDT[S.CAST_FMT[kind]])
    _ok(lib.sgc_permute_cast(L.ptr(_dev(src)), L.ptr(dst), kind, len(dims), _harr(ctypes.c_int, dims), _harr(L_, ss), _harr(L_, ds), L_(so), L_(do),
                             L.stream_ptr()), "sgc_permute_cast")
    _cast_check(dst, pos, val, kind, "permute_cast %d kind %d" % (case, kind))


SEGMENTS = [   # rows, cols, src row stride, src column stride, [(dst_off, dst_ld, src_off)]
    (5, 6, 1, 7, [(3, 9, 2)]),
    (4, 8, 8, 1, [(s * 50 + (s % 3), 8 + s % 4, s * 32) for s in range(48)]),
    (257, 511, 1, 257, [(1, 511, 0), (257 * 520 + 4, 513, 0)]),                 # 131 327 elements per segment: the second trip of 512 blocks x 256
]


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("case", range(len(SEGMENTS)))
def test_segment_cast(case, kind):
    L, lib = _lib()
    rows, cols, sr, scol, segs = SEGMENTS[case]
    rng = np.random.default_rng(110 + case)
    n_src = max(s[2] for s in segs) + (rows - 1) * sr + (cols - 1) * scol + 1
    size = max(s[0] + (rows - 1) * s[1] + cols for s in segs) + 3
    src = _cast_source(rng, n_src)
    d_off, d_ld, s_off = [s[0] for s in segs], [s[1] for s in segs], [s[2] for s in segs]
    pos, val = S.segment_cast_reference(src, size, rows, cols, sr, scol, d_off, d_ld, s_off)
    if case == 2:
        assert rows * cols > 131072
    if case == 1:
        assert len(segs) == 48 and len(set(d_ld)) > 1
    dst = _filled((size + 1,), TDT[S.CAST_FMT[kind]])
    _ok(lib.sgc_segment_cast(L.ptr(_dev(src)), L.ptr(dst), kind, rows, cols, L_(sr), L_(scol), len(segs), _harr(L_, d_off), _harr(L_, d_ld),
                             _harr(L_, s_off), L.stream_ptr()), "sgc_segment_cast")
    _cast_check(dst, pos, val, kind, "segment_cast %d kind %d" % (case, kind))


# ================================================================================================================= 8. SGD
SGD_SMALL = [1, 2, 3, 4, 5, 7, 1023]
HYPER = {"exact": (2.0 ** -3, 0.5, 2.0 ** -4), "real": (3e-3, 0.9, 1e-4)}


def _sgd_data(rng, n, regime):
    if regime == "exact":
        draw = lambda: (rng.integers(-8, 9, n) * 16).astype(np.float64)          # multiples of 16: lr, wd and two momentum steps keep every value an exact f32
        return draw(), draw(), draw()
    return rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)


def _sgd_check(regime, what, w, buf, wv, bv, gv, hyper, first):
    """One step's result against the reference evaluated from the state the DEVICE had before the step (float64 of its bits)."""
    lr, mom, wd = (float(np.float32(h)) for h in hyper)
    rw, rb, mw, mb = S.sgd_reference(wv, gv, bv, lr, mom, wd, first)
    # roundings: g + wd w (2), momentum buf + g' (2) -> buf: 4; w - lr buf (2 more): 6
    _check(regime, buf, rb, "f32", what + " buf", mag=mb, n=S.N_SGD_BUF)
    _check(regime, w, rw, "f32", what + " w", mag=mw, n=S.N_SGD_W)


def _run_single(lib, L, w, g, buf, n, hyper, first):
    _ok(lib.sgc_sgd_momentum_step(L.ptr(w), L.ptr(g), L.ptr(buf), L_(n), F(hyper[0]), F(hyper[1]), F(hyper[2]), first, L.stream_ptr()),
        "sgc_sgd_momentum_step")


@pytest.mark.parametrize("regime", REGIMES)
def test_sgd_step_forms(regime):
    L, lib = _lib()
    rng = np.random.default_rng(120)
    hyper = HYPER[regime]
    # ---- the aligned (float4 + tail) and the misaligned (scalar) kernel: two steps each, and one against the other in REAL
    for n in SGD_SMALL + [16384 * 1024 + 4 * 256 + 3, 16384 * 256 + 5]:
        offsets = (0, 1) if n < 16384 * 1024 else (0,)
        if n == 16384 * 256 + 5:
            offsets = (1,)
        w0, b0, _ = _sgd_data(rng, n, regime)
        gs = [_sgd_data(rng, n, regime)[0] for _ in range(2)]
        results = {}
        for off in offsets:
            base = [_filled((n + 8,), torch.float32) for _ in range(3)]
            w, g, buf = (t[off:off + n] for t in base)
            assert w.data_ptr() % 16 == 4 * off
            w.copy_(_dev(w0, torch.float32))
            buf.copy_(_dev(b0, torch.float32))                                   # what a first step must ignore
            for step in (0, 1):
                g.copy_(_dev(gs[step], torch.float32))
                wv, bv, gv = (t.double().cpu().numpy() for t in (w, buf, g))
                _run_single(lib, L, w, g, buf, n, hyper, 1 - step)
                _sgd_check(regime, "sgd step n = %d offset %d step %d" % (n, off, step), w, buf, wv, bv, gv, hyper, step == 0)
            for t in base:
                _assert_fill(t[:off], "in front of the view")
                _assert_fill(t[off + n:], "behind the view")
            results[off] = (_bits(w).copy(), _bits(buf).copy())
            KEEP.clear()
        if len(results) == 2:
            assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1]), \
                "n = %d: the float4 and the scalar kernel give different bits" % n
    # ---- the multi-tensor form against the single-tensor form on the same data
    for n_t in (1, 22, 32):
        lens = ([262144 + 1] if n_t == 1 else [1, 3, 0, 262144 + 1, 5, 1023] + [int(v) for v in rng.integers(1, 300, n_t - 6)])
        first_mask = 0 if n_t == 1 else int(sum(1 << t for t in range(n_t) if t % 3 == 0))
        ws, gs_, bs, alig, mis = [], [], [], [], []
        for t, n in enumerate(lens):
            m = max(n, 1)
            w0, b0, _ = _sgd_data(rng, m, regime)
            trio = [_filled((m + 4,), torch.float32) for _ in range(3)]
            for buf_t, v in zip(trio, (w0, np.zeros(m), b0)):
                buf_t[:m] = _dev(v, torch.float32)
            ws.append(trio[0]), gs_.append(trio[1]), bs.append(trio[2])
            alig.append([x[:n].clone() for x in trio])                           # the same data for the float4 kernel ...
            mis.append([_filled((m + 5,), torch.float32)[1:1 + n].copy_(x[:n]) for x in trio])      # ... and for the scalar kernel
        ptrs = lambda ts: _harr(ctypes.c_void_p, [t.data_ptr() for t in ts])
        for step in (0, 1):
            mask = first_mask if step == 0 else 0
            state = []
            for t, n in enumerate(lens):
                g_new = _dev(_sgd_data(rng, max(n, 1), regime)[0], torch.float32)
                for form in (alig[t], mis[t]):
                    form[1].copy_(g_new[:n])
                gs_[t][:max(n, 1)] = g_new
                state.append(tuple(x.double().cpu().numpy() for x in alig[t]))
                if n:
                    _run_single(lib, L, *alig[t], n, hyper, (mask >> t) & 1)
                    assert mis[t][0].data_ptr() % 16 == 4
                    _run_single(lib, L, *mis[t], n, hyper, (mask >> t) & 1)
            before = [(_bits(w).copy(), _bits(b).copy()) for w, b in zip(ws, bs)]
            _ok(lib.sgc_sgd_momentum_multi(n_t, ptrs(ws), ptrs(gs_), ptrs(bs), _harr(L_, lens), F(hyper[0]), F(hyper[1]), F(hyper[2]),
                                           ctypes.c_uint(mask), L.stream_ptr()), "sgc_sgd_momentum_multi")
            for t, n in enumerate(lens):
                assert np.array_equal(_bits(ws[t][n:]), before[t][0][n:]) and np.array_equal(_bits(bs[t][n:]), before[t][1][n:]), "behind tensor %d" % t
                if not n:
                    continue
                wv, gv, bv = state[t]
                if n in (1, 3, 262144 + 1):
                    _sgd_check(regime, "sgd multi %d tensors, tensor %d n = %d step %d" % (n_t, t, n, step), ws[t][:n], bs[t][:n], wv, bv, gv, hyper,
                               bool((mask >> t) & 1))
                for name, form in (("float4", alig[t]), ("scalar", mis[t])):
                    assert torch.equal(ws[t][:n], form[0]) and torch.equal(bs[t][:n], form[2]), \
                        "tensor %d of %d, step %d: the multi-tensor and the %s kernel give different bits" % (t, n_t, step, name)
        KEEP.clear()


# ================================================================================================================= 9. head backward
def _head_dev(case):
    d = {k: _dev(case[k], torch.float32) for k in ("rel", "sup", "conn", "p", "a", "b", "c", "y", "W", "dp_extra", "cs_coef", "cand_conf")}
    d["tgt"], d["cand_pred"] = _i32(case["tgt"]), _i32(case["cand_pred"])
    return d


def _head_launch(lib, L, case, d, n, hier, scale, extra, cs, dl, loss, dpre):
    T = case["T"]
    return lib.sgc_head_loss_bwd(L.ptr(d["rel"]), L.ptr(d["sup"]), L.ptr(d["conn"]), L.ptr(d["p"]), L.ptr(d["tgt"]), L.ptr(d["a"]), L.ptr(d["b"]),
                                 L.ptr(d["c"]), L.ptr(d["y"]), L.ptr(d["W"]), n, S.NG if hier else S.R, S.NP if hier else 0, S.NS if hier else 0, hier,
                                 F(T[0]), F(T[1]), F(T[2]), F(scale), L.ptr(dl), L.ptr(loss), L.ptr(dpre), L.ptr(d["dp_extra"] if extra else None),
                                 L.ptr(d["cs_coef"] if cs else None), L.ptr(d["cand_conf"]), L.ptr(d["cand_pred"]), L.stream_ptr())


def _budget_check(t, ref, budget, fmt, what):
    """REAL only: the budget the reference worked out (see step_glue_cases.HEAD_ROUNDINGS) + the output format's own rounding."""
    _check("real", t, ref, fmt, what, bound=budget)


@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("cs", [0, 1])
@pytest.mark.parametrize("hier", [1, 0])
def test_head_loss_bwd(hier, cs, extra, scale):
    L, lib = _lib()
    n = 5
    case = S.head_case(np.random.default_rng(130 + hier), n, hier)
    assert (case["cs_coef"] == 0).any() and (case["cs_coef"] != 0).any()
    d = _head_dev(case)
    dl, loss, dpre = _filled((n + 1, 64), torch.float32), _filled((n + 1,), torch.float32), _filled((n + 1, 512), torch.bfloat16)
    _ok(_head_launch(lib, L, case, d, n, hier, scale, extra, cs, dl, loss, dpre), "sgc_head_loss_bwd")
    rloss, rdl, rdpre, e_dpre, e_loss, e_dl = S.head_loss_reference(
        case["rel"], case["sup"], case["conn"], case["p"], case["tgt"], case["a"], case["b"], case["c"], case["y"], case["W"], hier, case["invT"],
        scale, case["dp_extra"] if extra else None, case["cs_coef"] if cs else None, case["cand_conf"], case["cand_pred"])
    what = "head_loss_bwd hier %d cs %d extra %d scale %g" % (hier, cs, extra, scale)
    _budget_check(dl[:n], rdl, e_dl, "f32", what + " dl")
    _budget_check(loss[:n], rloss, e_loss, "f32", what + " loss")
    _budget_check(dpre[:n], rdpre, e_dpre, "bf16", what + " dpre")
    dead = case["p"] <= 0
    assert dead.any() and (_bits(dpre[:n])[dead] & 0x7FFF == 0).all()                  # p zero or negative: an exact 0
    nrow = S.R + 4 if hier else S.R + 1
    assert (_bits(dl[:n, nrow:]) == 0).all()
    for t in (dl, loss, dpre):
        _assert_fill(t[n:], what)


def test_head_loss_bwd_position_independent():
    L, lib = _lib()
    n, big = 5, 4097
    rows = [0, 1023, 1024, 2047, 2048, 4095, 4096]
    case = S.head_case(np.random.default_rng(131), n, 1)
    bulk = S.head_case(np.random.default_rng(132), big, 1)
    d = _head_dev(case)
    outs = (_filled((n, 64), torch.float32), _filled((n,), torch.float32), _filled((n, 512), torch.bfloat16))
    _ok(_head_launch(lib, L, case, d, n, 1, 2.0, 1, 1, *outs), "sgc_head_loss_bwd")
    small = [_bits(t).copy() for t in outs]
    for shift in range(2):                                                     # the five pairs at rows r, r + 1 .. would overlap: place pair k % 5 at every listed row
        for key in ("rel", "sup", "conn", "p", "a", "b", "c", "y", "dp_extra", "cs_coef", "cand_conf", "tgt", "cand_pred"):
            for i, r in enumerate(rows):
                bulk[key][r] = case[key][(i + shift) % n]
        bulk["W"] = case["W"]
        db = _head_dev(bulk)
        bo = (_filled((big + 1, 64), torch.float32), _filled((big + 1,), torch.float32), _filled((big + 1, 512), torch.bfloat16))
        _ok(_head_launch(lib, L, bulk, db, big, 1, 2.0, 1, 1, *bo), "sgc_head_loss_bwd")
        for t, s in zip(bo, small):
            got = _bits(t)
            for i, r in enumerate(rows):
                assert np.array_equal(got[r], s[(i + shift) % n]), "row %d differs from the batch of five" % r
            _assert_fill(t[big:], "behind the batch")
            assert not np.isnan(t[:big].float().cpu().numpy()).any()
        KEEP.clear()


@pytest.mark.parametrize("given", [(1, 1, 1), (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)])
@pytest.mark.parametrize("hier", [1, 0])
def test_head_bwd_upstream(hier, given):
    L, lib = _lib()
    n = 5
    rng = np.random.default_rng(133)
    case = S.head_case(rng, n, hier)
    g_rel, g_sup, g_conn, g_hid = S.f32(rng.standard_normal((n, S.R))), S.f32(rng.standard_normal((n, 3))), S.f32(rng.standard_normal(n)), \
        S.f32(rng.standard_normal((n, 512)))
    d = _head_dev(case)
    opt = lambda flag, a: _dev(a, torch.float32) if flag else None
    dl, dpre = _filled((n + 1, 64), torch.float32), _filled((n + 1, 512), torch.bfloat16)
    T = case["T"]
    _ok(lib.sgc_head_bwd_upstream(L.ptr(d["rel"]), L.ptr(d["sup"]), L.ptr(d["p"]), L.ptr(_dev(g_rel, torch.float32)), L.ptr(opt(given[0], g_sup)),
                                  L.ptr(opt(given[1], g_conn)), L.ptr(opt(given[2], g_hid)), L.ptr(d["W"]), n, S.NG if hier else S.R,
                                  S.NP if hier else 0, S.NS if hier else 0, hier, F(T[0]), F(T[1]), F(T[2]), F(2.0), L.ptr(dl), L.ptr(dpre),
                                  L.stream_ptr()), "sgc_head_bwd_upstream")
    rdl, rdpre, e_dpre, e_dl = S.head_upstream_reference(case["rel"], case["sup"], case["p"], g_rel, g_sup if given[0] else None,
                                                         g_conn if given[1] else None, g_hid if given[2] else None, case["W"], hier, case["invT"], 2.0)
    what = "head_bwd_upstream hier %d given %s" % (hier, "".join(str(v) for v in given))
    _budget_check(dl[:n], rdl, e_dl, "f32", what + " dl")
    _budget_check(dpre[:n], rdpre, e_dpre, "bf16", what + " dpre")
    _assert_fill(dl[n:], what)
    _assert_fill(dpre[n:], what)


@pytest.mark.parametrize("n,chunk", [(1, 1), (5, 2), (130, 64)])
@pytest.mark.parametrize("regime", REGIMES)
def test_head_wgrad(regime, n, chunk):
    L, lib = _lib()
    rng = np.random.default_rng(134)
    dlv = G.values(rng, (n, 64), regime, -30, 30)
    dlv[:, 54:] = 0.0                                                           # outputs the head does not have
    dl, dlv = _operand(dlv, "f32", regime)
    p, pv = _operand(G.values(rng, (n, 512), regime, -30, 30), "f32", regime)
    nb = -(-n // chunk)
    part = _filled((nb + 1, 64, 513), torch.float32)
    _ok(lib.sgc_head_wgrad(L.ptr(dl), L.ptr(p), L.ptr(part), n, chunk, L.stream_ptr()), "sgc_head_wgrad")
    ref, mag = S.head_wgrad_reference(dlv, pv, chunk)
    _check(regime, part[:nb], ref, "f32", "head_wgrad %d / %d" % (n, chunk), mag=mag, n=chunk)      # one fused multiply-add per pair of the chunk
    assert (_bits(part[:nb, 54:]) & 0x7FFFFFFF == 0).all()
    _assert_fill(part[nb:], "part")


# ================================================================================================================= argument checks
def test_argument_checks():
    """Every documented argument check returns SGC_ERR_ARG (1) before anything is read or launched: all pointers are NULL."""
    L, lib = _lib()
    N, st = L.ptr(None), L.stream_ptr()
    assert lib.sgc_colsum(1, N, N, L_(8), 12, 1, st) == 1
    assert lib.sgc_segment_sum_rows(N, N, N, N, 1, 256, st) == 1
    assert lib.sgc_convert_f16_bf16(N, N, L_(12), st) == 1
    for max_n in (0, 151):
        assert lib.sgc_pair_expand_dense(N, N, N, N, 8, 1, max_n, N, N, N, st) == 1
        assert lib.sgc_pair_expand_dense_windows(N, N, N, N, 8, 1, max_n, N, N, N, N, st) == 1
    for ndim in (0, 6):
        assert lib.sgc_permute_cast(N, N, 0, ndim, N, N, N, L_(0), L_(0), st) == 1
    assert lib.sgc_segment_cast(N, N, 0, 4, 4, L_(4), L_(1), 49, N, N, N, st) == 1
    assert lib.sgc_sgd_momentum_multi(33, N, N, N, N, F(0.1), F(0.9), F(0.0), ctypes.c_uint(0), st) == 1
    assert lib.sgc_object_masked_maps_bwd(N, N, N, N, N, N, 1, 32, 64, st) == 1
    assert lib.sgc_pack_image_nhwc(N, 256, N, 1, N, 1, 96, 384, st) == 1
    assert lib.sgc_pack_image_nhwc(N, 384, N, 1, N, 1, 64, 384, st) == 1
    torch.cuda.synchronize()


def test_worst_ratios_are_reported():
    """Prints the worst got / bound of every REAL check of this run (pytest -s), so that one line per check lands in the profile."""
    for what in sorted(WORST):
        print("STEP-GLUE worst %-74s %.4f" % (what, WORST[what]))
    print("STEP-GLUE peak device memory %.0f MiB" % (torch.cuda.max_memory_allocated() / 2.0 ** 20))
    assert all(v <= 1.0 for v in WORST.values())
