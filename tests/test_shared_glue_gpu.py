"""The non-GEMM kernels of csrc/kernels_shared.hip (and the two row-table kernels of csrc/kernels_scene.hip the plan calls with them),
each on its own launch through the shipped C ABI, against the definitional float64 / int64 references of tests/shared_glue_cases.py.

EXACT regime: small-integer operands for which ``assert_exact`` holds; every output must equal, bit for bit, the exact sum rounded once
(RNE) to the output type.  REAL regime: seeded reals, per element |got - ref| <= u_out |ref| + n 2**-24 sum |terms|, no element
excluded, the worst got / bound printed (pytest -s).  Every checked output's crc is kept per (regime, case): a second run in the same
process (pytest FILE FILE --keep-duplicates) must give the same bits.  Every output buffer is pre-filled with 0xFF bytes and one row /
entry / slab longer than what the kernel owns: what the kernel documents as unwritten must keep the fill; operand rows it must not read hold NaN.

Which test reaches which entry point and branch:

  test_compact_row_table                  sgc_window_rows_compact            base set, its subset; 130 objects: second pass of the 256-thread
                                                                             loop and its running base; background rows outside R_o
  test_object_and_conv_row_tables         sgc_window_rows_objects_compact,   rows of the pseudo-pairs' own windows; rows of the conv list
                                          sgc_window_rows_conv               (linear pairs skipped: first(pair, all) != first(pair, conv));
                                                                             the X entries' rows of the host tables = sgc_bucket_place's
  test_row_source_table                   sgc_window_rows_source             consistent tables | one dest outside the space | one gather with
                                                                             a pair row >= zero_row (names the zero row); prow_src clamp
  test_three_counts_and_class_lists       sgc_shared_windows_count3,         counts / pixel rectangles of all three kinds of pair; both
                                          sgc_shared_windows_fill_class      classes partition the list of sgc_shared_windows_fill
  test_argmax_rows_of_the_pseudo_pairs    sgc_shared_objects_fill_argmax     = the argmax half of sgc_shared_objects_fill_rows; fill kept in R_o
  test_padding_rows_are_zeroed            sgc_fc1_pad_rows_zero              groups with 0, 1, 4, 255 padding rows
  test_background_gradient_rows_compact   sgc_shared_objects_bg_grad_compact pure copy goff[w] + b -> b * 64 + w
  test_im2patch_from_an_entry             sgc_windows_im2patch_f16_from      e0 = 5 (no multiple of 16), zero rows behind *gather_n, f16 -> bf16
                                                                             RNE, same bits as sgc_windows_im2patch_f16
  test_prefix_sums                        sgc_fc1_integral_rows,             81 x 4096 entries per pseudo-pair incl. the zero border, through
                                          sgc_fc1_integral                   prow (compact rows, background rows shared) and through goff
  test_own_rectangle_sums                 sgc_fc1_own_rect_sums              every object, empty R_j: exact 0
  test_fc1_assembly                       sgc_fc1_assemble, _ordered, _x16   own sums given / NULL x pair_order NULL / permutation x dropout
                                                                             off / on x full / compact rows; pairs with 0 and with 64 X
                                                                             entries, R_j empty (no rectangle term), linear and identical boxes
  test_gradient_sums_compact              sgc_fc1_gsum_compact               (goff, prow) and (cbase, prow_src) into a gsrc buffer; images of
                                                                             0, 1, 8, 9, 17 objects; 1, 15, 16, 17 partners in either role;
                                                                             513 partners in either role (re-staging per tile)
  test_gradient_sums_full_rows            sgc_fc1_gsum                       base set, the same reference (role 1 outside R_o: zero rows)
  test_x_rows_and_padding                 sgc_fc1_xrows                      X rows copied, padding zeroed in both buffers, the rest kept
  test_linear_forward                     sgc_windows_linear_forward         y f16 / bf16 / argmax / dest_linear and their NULL forms; ties,
                                                                             killed maxima, raw rows nobody names hold NaN
  test_linear_backward_objects            sgc_windows_linear_backward_objects entries touched by 0, 1, 2 and 71 linear pairs (second ballot
                                                                             chunk); untouched entries keep arbitrary bits
  test_linear_backward_background         sgc_windows_linear_backward_bg     segments of 0, 1, 3, 4, 5, 16, 17, 65, 70 windows (every wave's
                                                                             groups of four, the second round of 16); base set; halo kept
  test_patch_sums                         sgc_windows_patch_sum2,            n16 = 0 | all | a split inside the list; centre pixels: two
                                          sgc_windows_patch_sum_objects2,    20-row slots; pixels outside the rectangle keep the fill;
                                          sgc_windows_patch_sum              linear pairs write nothing
  test_pair_contraction                   sgc_pair_contract_windows          both roles, bg_maps 0 / 1; 0, 1, 4, 5, 8, 9 and 70 candidates
                                                                             (every arm of the request / route schedule, second 64-chunk);
                                                                             background object of an image of 72 objects; zero cells; halo;
                                                                             and the base set (linear pairs: no dz, no candidate)
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from tests import shared_glue_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
REGIMES = ["exact", "real"]
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
WORST = {}
DIGEST = {}                                   # crc of every checked output: a second run in the same process must give the same bits
KEEP = []                                     # operands made inside a call's argument list stay alive until the test ends


@pytest.fixture(autouse=True)
def _keep_operands_alive():
    yield
    KEEP.clear()


def _lib():
    from scene_graph_commonsense_amd import _lib as L
    return L, L.load()


def _ok(status, what):
    assert status == 0, "%s returned %d" % (what, status)
    torch.cuda.synchronize()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    t = t if dtype is None else t.to(dtype)
    KEEP.append(t)
    return t


def _i32(a):
    return _dev(np.asarray(a, dtype=np.int32))


def _filled(shape, dtype):
    """A tensor of 0xFF bytes (-1 for integers, a NaN no kernel computes for floats)."""
    size = torch.empty((), dtype=dtype).element_size()
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[size]
    return torch.full(shape, 255 if size == 1 else -1, dtype=it, device=DEV).view(dtype)


def _bits(t):
    """device tensor -> numpy array of its bit patterns."""
    it, nt = {1: (torch.uint8, np.uint8), 2: (torch.int16, np.uint16), 4: (torch.int32, np.uint32)}[t.element_size()]
    return t.contiguous().view(it).cpu().numpy().view(nt)


def _fill_of(bits):
    return np.iinfo(bits.dtype).max


def _assert_fill(t, what):
    b = _bits(t)
    bad = int((b != _fill_of(b)).sum())
    assert bad == 0, "%s: %d elements the kernel does not own were written" % (what, bad)


def _operand(a, fmt, regime):
    """float64 values -> (device tensor of ``fmt``, the values it holds as float64).  EXACT: the values must be representable."""
    t = _dev(a, torch.float64).to(TDT[fmt])
    back = t.double().cpu().numpy()
    if regime == "exact":
        assert np.array_equal(back, a), "operand not representable in " + fmt
    return t, back


def _check(regime, t, ref, fmt, what, mag=None, n=None, scale=1.0):
    """One output tensor against its float64 reference in the regime's way; ``mag`` / ``n``: sum of |terms| and number of additions."""
    crc = zlib.crc32(_bits(t).tobytes())
    assert DIGEST.setdefault((regime, what), crc) == crc, what + ": other bits than the first time in this process"
    if regime == "exact":
        G.assert_exact(mag, what)
        G.check_bits(_bits(t), ref, fmt, what)
    else:
        got = t.double().cpu().numpy()
        WORST[what] = G.check_real(got, ref, G.real_bound(ref, mag, n, fmt, scale), what)


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


SCENES = {"base": lambda: G.base_scene(), "subset": lambda: G.base_scene(subset=True), "full2": lambda: G.Scene(G.FULL2_IMAGES),
          "many": G.many_objects_scene, "groups": G.gsum_groups_scene, "groups_swap": lambda: G.gsum_groups_scene(swap=True),
          "partners513": G.gsum_many_partners_scene, "contract": G.contract_scene, "linear": G.linear_scene,
          "linear_objects": G.linear_objects_scene}


def _scene(cache, name):
    return cache(("scene", name), SCENES[name])


def _tables(cache, name):
    """The scene's boxes, pair lists and CSR lists on the device."""
    def build():
        sc = _scene(cache, name)
        sp, sl = G.csr(sc.sub, sc.n)
        op, ol = G.csr(sc.obj, sc.n)
        return dict(bb=_i32(sc.bb.reshape(-1)), sub=_i32(sc.sub), obj=_i32(sc.obj), obj_img=_i32(sc.obj_img), img_ptr=_i32(sc.img_ptr),
                    sp=_i32(sp), sl=_i32(sl), op=_i32(op), ol=_i32(ol), sp_h=sp, op_h=op)
    return cache(("tables", name), build)


# ================================================================================================================= 1. row tables
@pytest.mark.parametrize("name", ["base", "subset", "many"])
def test_compact_row_table(cache, name):
    L, lib = _lib()
    sc, tb = _scene(cache, name), _tables(cache, name)
    sp = sc.spaces["compact"]
    if name == "many":
        assert sc.n2 > 256
    prow = _filled((sc.n2 * 64 + 64,), torch.int32)
    _ok(lib.sgc_window_rows_compact(L.ptr(tb["bb"]), L.ptr(tb["obj_img"]), sc.n, sc.n_img, L.ptr(_i32(sp["goff"])), L.ptr(prow), L.stream_ptr()),
        "sgc_window_rows_compact")
    assert np.array_equal(prow[:sc.n2 * 64].cpu().numpy(), sp["prow"])
    _assert_fill(prow[sc.n2 * 64:], "prow")


@pytest.mark.parametrize("name", ["base", "subset"])
def test_object_and_conv_row_tables(cache, name):
    L, lib = _lib()
    sc = _scene(cache, name)
    sp = sc.spaces["compact"]
    assert sc.E_obj > 0 and 0 < sc.E_conv < sc.E_all
    dest = _filled((sc.E_obj + 1,), torch.int32)
    _ok(lib.sgc_window_rows_objects_compact(L.ptr(_i32(sc.gather_all[sc.E_all:])), sc.E_obj, L.ptr(_i32(sp["prow"])), sc.P, L.ptr(dest), L.stream_ptr()),
        "sgc_window_rows_objects_compact")
    assert np.array_equal(dest[:-1].cpu().numpy(), sp["dest"][sc.E_all:])
    _assert_fill(dest[-1:], "dest")
    n = len(sc.gather_conv)
    dconv = _filled((n + 1,), torch.int32)
    _ok(lib.sgc_window_rows_conv(L.ptr(_i32(sc.gather_conv)), n, L.ptr(_i32(sc.incl_conv)), L.ptr(_i32(sc.incl_all)), L.ptr(_i32(sp["dest"])),
                                 L.ptr(dconv), L.stream_ptr()), "sgc_window_rows_conv")
    assert np.array_equal(dconv[:-1].cpu().numpy(), sp["dest_conv"])
    _assert_fill(dconv[-1:], "dest_conv")
    # the X entries' rows as the plan places them (sgc_bucket_place): the host tables every value test below uses are the device's
    dx = _filled((sc.E_all + 1,), torch.int32)
    _ok(lib.sgc_bucket_place(L.ptr(_i32(sc.gather_all)), sc.E_all, L.ptr(None), L.ptr(None), 0, 64, L.ptr(_i32(sp["xbase"])), L.ptr(dx), L.ptr(None), 0,
                             L.stream_ptr()), "sgc_bucket_place")
    assert np.array_equal(dx[:-1].cpu().numpy(), sp["dest"][:sc.E_all])
    _assert_fill(dx[-1:], "dest of the X entries")


def _row_source_tables(sc):
    sp = sc.spaces["compact"]
    Ppad = (sc.P + 63) // 64 * 64
    lead = sp["lead"]
    cbase = (Ppad + 1 + np.concatenate([[0], np.cumsum(lead)[:-1]])).astype(np.int32)
    prow_src = np.array([cbase[i & 63] + max(0, min(int(sp["prow"][i]) - int(sp["goff"][i & 63]), int(lead[i & 63]) - 1))
                         for i in range(sc.n2 * 64)], dtype=np.int32)
    return Ppad, cbase, prow_src


@pytest.mark.parametrize("kind", ["consistent", "dest_outside", "pair_row_beyond"])
def test_row_source_table(cache, kind):
    L, lib = _lib()
    sc = _scene(cache, "base")
    sp = sc.spaces["compact"]
    Ppad, cbase, prow_src = _row_source_tables(sc)
    rows, E = sp["rows"], sc.E_all
    gather, dest = sc.gather_all[:E].copy(), sp["dest"][:E].copy()
    want = np.full(rows, Ppad, dtype=np.int32)                       # the caller's preset: the zero row
    for w in range(64):
        k = np.arange(int(sp["lead"][w]))
        want[sp["goff"][w] + k] = cbase[w] + k
    if kind == "dest_outside":
        dest[3] = rows + 5                                           # guarded: nothing is written for it, its row keeps the preset
    if kind == "pair_row_beyond":
        gather[5] = (Ppad + 7) * 64 + (gather[5] & 63)               # guarded: the entry names the zero row
    for e in range(E):
        if 0 <= dest[e] < rows:
            want[dest[e]] = (gather[e] >> 6) if (gather[e] >> 6) < Ppad else Ppad
    rowsrc = _filled((rows + 1,), torch.int32)
    rowsrc[:rows] = Ppad
    psrc = _filled((sc.n2 * 64 + 1,), torch.int32)
    _ok(lib.sgc_window_rows_source(L.ptr(_i32(gather)), L.ptr(_i32(dest)), E, L.ptr(_i32(sp["goff"])), L.ptr(_i32(sp["xbase"])), L.ptr(_i32(sp["gend"])),
                                   L.ptr(_i32(cbase)), Ppad, int(sp["lead"].max()) + 256, L.ptr(_i32(sp["prow"])), sc.n2 * 64, rows, L.ptr(rowsrc),
                                   L.ptr(psrc), L.stream_ptr()), "sgc_window_rows_source")
    assert np.array_equal(rowsrc[:rows].cpu().numpy(), want)
    assert np.array_equal(psrc[:-1].cpu().numpy(), prow_src)
    _assert_fill(rowsrc[rows:], "rowsrc")
    _assert_fill(psrc[-1:], "prow_src")


@pytest.mark.parametrize("name", ["base", "subset", "linear_objects"])
def test_three_counts_and_class_lists(cache, name):
    L, lib = _lib()
    sc, tb = _scene(cache, name), _tables(cache, name)
    P = sc.P
    assert min(sc.kinds()) > 0
    out = _filled((4, P + 1), torch.int32)
    _ok(lib.sgc_shared_windows_count3(L.ptr(tb["bb"]), L.ptr(tb["sub"]), L.ptr(tb["obj"]), P, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.ptr(out[3]),
                                      L.stream_ptr()), "sgc_shared_windows_count3")
    got = out.cpu().numpy()
    for k, want in enumerate((sc.cnt_all, sc.cnt_conv, sc.cnt_lin, sc.pixrect_conv)):
        assert np.array_equal(got[k, :P], want), k
    _assert_fill(out[:, P], "counts")
    lists = []
    for cls, incl, want in ((1, sc.incl_conv, sc.gather_conv[:sc.E_conv]), (2, sc.incl_lin, sc.gather_lin)):
        g = _filled((len(want) + 1,), torch.int32)
        _ok(lib.sgc_shared_windows_fill_class(L.ptr(tb["bb"]), L.ptr(tb["sub"]), L.ptr(tb["obj"]), P, L.ptr(_i32(incl)), L.ptr(g), cls, L.stream_ptr()),
            "sgc_shared_windows_fill_class")
        assert np.array_equal(g[:-1].cpu().numpy(), want), cls
        _assert_fill(g[-1:], "gather of class %d" % cls)
        lists.append(g[:-1].cpu().numpy())
    g = _filled((sc.E_all + 1,), torch.int32)
    _ok(lib.sgc_shared_windows_fill(L.ptr(tb["bb"]), L.ptr(tb["sub"]), L.ptr(tb["obj"]), P, L.ptr(_i32(sc.incl_all)), L.ptr(g), L.stream_ptr()),
        "sgc_shared_windows_fill")
    assert np.array_equal(g[:-1].cpu().numpy(), sc.gather_all[:sc.E_all])
    assert np.array_equal(np.sort(np.concatenate(lists)), np.sort(g[:-1].cpu().numpy())) and not set(lists[0]) & set(lists[1])


def test_argmax_rows_of_the_pseudo_pairs(cache):
    L, lib = _lib()
    sc, tb = _scene(cache, "base"), _tables(cache, "base")
    sp = sc.spaces["full"]
    gen = torch.Generator(device=DEV).manual_seed(5)
    am_bg = torch.randint(0, 5, (sc.n_img * 64, 1024), device=DEV, dtype=torch.uint8, generator=gen)
    am_ps = _filled(((sc.n2 + 1) * 64, 1024), torch.uint8)
    _ok(lib.sgc_shared_objects_fill_argmax(L.ptr(tb["bb"]), L.ptr(tb["obj_img"]), sc.n, L.ptr(am_bg), L.ptr(am_ps), L.stream_ptr()),
        "sgc_shared_objects_fill_argmax")
    got, bg = am_ps.cpu().numpy().reshape(sc.n2 + 1, 64, 1024), am_bg.cpu().numpy().reshape(sc.n_img, 64, 1024)
    ins = np.tile(sc.inside, (2, 1))
    want = np.where(ins[:, :, None], 255, bg[np.tile(sc.obj_img, 2)])
    assert np.array_equal(got[:sc.n2], want) and (got[sc.n2] == 255).all()
    # the argmax half of sgc_shared_objects_fill_rows
    y_bg = torch.randn(sc.n_img * 64, 1024, device=DEV, generator=gen).half()
    ywm, ywm_bf = _filled((sp["rows"], 1024), torch.float16), _filled((sp["rows"], 1024), torch.bfloat16)
    am2 = _filled(((sc.n2 + 1) * 64, 1024), torch.uint8)
    y_bf = y_bg.bfloat16()
    _ok(lib.sgc_shared_objects_fill_rows(L.ptr(tb["bb"]), L.ptr(tb["obj_img"]), sc.n, L.ptr(_i32(sp["goff"])), L.ptr(y_bg), L.ptr(y_bf),
                                         L.ptr(am_bg), L.ptr(ywm), L.ptr(ywm_bf), L.ptr(am2), L.stream_ptr()), "sgc_shared_objects_fill_rows")
    assert torch.equal(am2, am_ps)


def test_padding_rows_are_zeroed():
    L, lib = _lib()
    pads = np.array([0, 1, 4, 255] * 16)
    used = 1 + np.arange(64) % 5
    goff = np.concatenate([[0], np.cumsum(used + pads)]).astype(np.int32)
    gend = (goff[:64] + used).astype(np.int32)
    rows = int(goff[64])
    y = _filled((rows + 1, 1024), torch.bfloat16)
    _ok(lib.sgc_fc1_pad_rows_zero(L.ptr(_i32(goff)), L.ptr(_i32(gend)), L.ptr(y), L.stream_ptr()), "sgc_fc1_pad_rows_zero")
    got = _bits(y)
    pad = np.zeros(rows + 1, dtype=bool)
    for g in range(64):
        pad[gend[g]:goff[g + 1]] = True
    assert pad.sum() == pads.sum()
    assert (got[pad] == 0).all() and (got[~pad] == 0xFFFF).all()


def test_background_gradient_rows_compact(cache):
    L, lib = _lib()
    sc = _scene(cache, "base")
    sp = sc.spaces["compact"]
    gen = torch.Generator(device=DEV).manual_seed(6)
    dywm = torch.randint(-32768, 32767, (sp["rows"], 1024), device=DEV, dtype=torch.int16, generator=gen).view(torch.bfloat16)
    dy_bg = _filled((sc.n_img * 64 + 1, 1024), torch.bfloat16)
    _ok(lib.sgc_shared_objects_bg_grad_compact(sc.n_img, L.ptr(_i32(sp["goff"])), L.ptr(dywm), L.ptr(dy_bg), L.stream_ptr()),
        "sgc_shared_objects_bg_grad_compact")
    src = np.array([sp["goff"][w] + b for b in range(sc.n_img) for w in range(64)])
    assert np.array_equal(_bits(dy_bg[:-1]), _bits(dywm)[src])
    _assert_fill(dy_bg[-1:], "dy_bg")


def test_im2patch_from_an_entry(cache):
    L, lib = _lib()
    sc = _scene(cache, "base")
    E = len(sc.gather_conv)
    Epad, e0 = (E + 63) // 64 * 64, 5
    assert e0 % 16 and Epad > E
    rng = np.random.default_rng(8)
    zv = rng.standard_normal((sc.P + sc.n2, 18, 18, 512))
    z, zb = _operand(zv, "f16", "real")                                              # f16 values with more bits than bf16 holds
    lost, half = G.rounding_cases(zb, "bf16")
    assert lost > 0
    gather = _i32(np.concatenate([sc.gather_conv, np.full(Epad - E, -1)]))           # behind *gather_n: never read
    gn = _i32([E])
    full = _filled((Epad + 1, 16, 512), torch.bfloat16)
    _ok(lib.sgc_windows_im2patch_f16(L.ptr(z), L.ptr(gather), L.ptr(gn), Epad, L.ptr(full), L.stream_ptr()), "sgc_windows_im2patch_f16")
    part = _filled((Epad - e0 + 1, 16, 512), torch.bfloat16)
    _ok(lib.sgc_windows_im2patch_f16_from(L.ptr(z), L.ptr(gather), L.ptr(gn), e0, Epad - e0, L.ptr(part), L.stream_ptr()),
        "sgc_windows_im2patch_f16_from")
    pair, w = sc.gather_conv >> 6, sc.gather_conv & 63
    want = np.zeros((Epad, 16, 512))
    for pp in range(16):
        want[:E, pp] = zb[pair, 2 * (w >> 3) + pp // 4, 2 * (w & 7) + pp % 4]
    G.check_bits(_bits(full[:-1]), want, "bf16", "im2patch_f16")
    G.check_bits(_bits(part[:-1]), want[e0:], "bf16", "im2patch_f16_from")
    assert (_bits(part[E - e0:-1]) == 0).all()
    _assert_fill(full[-1:], "zpatch")
    _assert_fill(part[-1:], "zpatch from e0")


# ================================================================================================================= 2. fc1 forward chain
C1 = 4096


def _fc1_case(cache, name, regime):
    """Products of one scene in both row spaces, the device's prefix tables and own sums, and the definitional reference."""
    def build():
        L, lib = _lib()
        sc = _scene(cache, name)
        rng = np.random.default_rng(20 + len(name))
        f32 = lambda a: a.astype(np.float32).astype(np.float64)
        own = f32(G.values(rng, (sc.n2, 64, C1), regime, -30, 100))
        bg = f32(G.values(rng, (sc.n_img, 64, C1), regime, -30, 100))
        xp = G.values(rng, (sc.E_all, C1), regime, -30, 100)
        xp = xp.astype(np.float16).astype(np.float64)                          # f16-representable: the x16 form must give the same bits
        bias = f32(G.values(rng, (C1,), regime, -8, 8))
        T = G.pseudo_rows(sc, own, bg)
        pre, mag, nx = G.fc1_reference(sc, T, xp, bias)
        case = dict(sc=sc, T=T, pre=pre, mag=mag, n=77 + nx[:, None], bias=_dev(bias, torch.float32), spaces={})
        pitch = int(lib.sgc_fc1_products_pitch())
        ins = np.tile(sc.inside, (2, 1))
        for space, sp in sc.spaces.items():
            owm = np.full((sp["rows"] + 1, pitch), np.nan, dtype=np.float32)           # padding columns and rows nobody names: NaN
            prow = sp["prow"].reshape(sc.n2, 64)
            if space == "full":
                owm[prow.reshape(-1), :C1] = T.reshape(-1, C1)
            else:
                owm[prow[ins], :C1] = own[ins]
                for b in range(sc.n_img):
                    owm[sp["goff"][:64] + b, :C1] = bg[b]
            owm[sp["dest"][:sc.E_all], :C1] = xp
            oxh = np.full((sp["rows"] + 1, C1), np.nan, dtype=np.float16)
            oxh[sp["dest"][:sc.E_all]] = xp
            owm_d, S = _dev(owm), _filled((sc.n2 + 1, 81, C1), torch.float32)
            if space == "full":
                _ok(lib.sgc_fc1_integral(L.ptr(owm_d), L.ptr(_i32(sp["goff"])), sc.n2, L.ptr(S), L.stream_ptr()), "sgc_fc1_integral")
            else:
                _ok(lib.sgc_fc1_integral_rows(L.ptr(owm_d), L.ptr(_i32(sp["prow"])), sc.n2, L.ptr(S), L.stream_ptr()), "sgc_fc1_integral_rows")
            own_s = _filled((sc.n + 1, C1), torch.float32)
            _ok(lib.sgc_fc1_own_rect_sums(L.ptr(S), L.ptr(_i32(sc.bb.reshape(-1))), sc.n, L.ptr(own_s), L.stream_ptr()), "sgc_fc1_own_rect_sums")
            case["spaces"][space] = dict(owm=owm_d, oxh=_dev(oxh), S=S, own=own_s, dest=_i32(sp["dest"]))
        return case
    return cache(("fc1", name, regime), build)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", ["base", "full2"])
def test_prefix_sums(cache, name, regime):
    case = _fc1_case(cache, name, regime)
    sc = case["sc"]
    Sref, A = G.integral_reference(case["T"])
    tot = np.broadcast_to(A[:, 8:9, 8:9], A.shape)
    for space in ("full", "compact"):
        S = case["spaces"][space]["S"]
        _check(regime, S[:sc.n2].view(sc.n2, 9, 9, C1), Sref, "f32", "fc1_integral%s %s" % ("_rows" if space == "compact" else "", name), mag=tot, n=16)
        _assert_fill(S[sc.n2:], "S")
    assert np.array_equal(_bits(case["spaces"]["full"]["S"]), _bits(case["spaces"]["compact"]["S"]))       # same values, same order of additions


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", ["base", "full2"])
def test_own_rectangle_sums(cache, name, regime):
    case = _fc1_case(cache, name, regime)
    sc = case["sc"]
    ref, _ = G.own_rect_reference(sc, case["T"])
    mag = 4 * np.abs(case["T"][sc.n:]).sum(1)                                              # four prefix values, each over up to 64 windows
    for space in ("full", "compact"):
        own = case["spaces"][space]["own"]
        _check(regime, own[:sc.n], ref, "f32", "fc1_own_rect_sums %s %s" % (name, space), mag=mag, n=19)
        _assert_fill(own[sc.n:], "own")
        empty = ~sc.inside.any(1)
        if name == "base":
            assert empty.sum() == 2
        assert (_bits(own[:sc.n])[empty] == 0).all()                                       # empty R_j: exact 0


@pytest.mark.parametrize("form", ["assemble", "ordered", "x16"])
@pytest.mark.parametrize("own", [False, True])
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("space", ["full", "compact"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", ["base", "subset", "full2"])
def test_fc1_assembly(cache, name, regime, space, drop, own, form):
    from scene_graph_commonsense_amd.synthetic import dropout_keep_mask
    L, lib = _lib()
    case, tb = _fc1_case(cache, name, regime), _tables(cache, name)
    sc, d = case["sc"], case["spaces"][space]
    P, seed = sc.P, 1234
    keep = dropout_keep_mask(seed, P, C1) if drop else None
    ref = G.fc1_activation(case["pre"], keep)
    if regime == "exact":                                     # the cases the bit comparison is about are there - before the device is asked
        lost, half = G.rounding_cases(ref, "f16")
        assert lost > 0 and half > 0 and (case["pre"] == 0).sum() > 0 and (case["pre"] < 0).sum() > 0
        if name == "full2":
            assert sc.cnt_all.max() == 64 and sc.cnt_all.min() == 0
    h1 = _filled((P + 1, C1), torch.float16)
    order = _i32(np.random.default_rng(3).permutation(P)) if form != "assemble" else None
    own_p = L.ptr(d["own"]) if own else L.ptr(None)
    incl = _i32(sc.incl_all)
    head = (L.ptr(tb["bb"]), L.ptr(tb["sub"]), L.ptr(tb["obj"]), L.ptr(incl), L.ptr(d["dest"]), sc.n, L.ptr(case["bias"]), int(drop), seed,
            L.ptr(h1), P, own_p)
    if form == "assemble":
        _ok(lib.sgc_fc1_assemble(L.ptr(d["S"]), L.ptr(d["owm"]), *head, L.stream_ptr()), "sgc_fc1_assemble")
    elif form == "ordered":
        _ok(lib.sgc_fc1_assemble_ordered(L.ptr(d["S"]), L.ptr(d["owm"]), *head, L.ptr(order), L.stream_ptr()), "sgc_fc1_assemble_ordered")
    else:
        _ok(lib.sgc_fc1_assemble_x16(L.ptr(d["S"]), L.ptr(d["oxh"]), *head, L.ptr(order), L.stream_ptr()), "sgc_fc1_assemble_x16")
    what = "fc1_%s %s %s drop %d own %d" % (form, name, space, drop, own)
    _check(regime, h1[:P], ref, "f16", what, mag=case["mag"], n=case["n"], scale=2.0 if drop else 1.0)
    _assert_fill(h1[P:], "h1")
    # all forms of one (scene, regime, space, dropout) give the same bits: the own sums are the same expression, the X products are f16 values
    first = cache(("h1", name, regime, space, drop), lambda: h1[:P].clone())
    assert np.array_equal(_bits(first), _bits(h1[:P])), what


# ================================================================================================================= 3. fc1 backward sums
def _gsum_case(cache, name, regime):
    def build():
        sc = _scene(cache, name)
        rng = np.random.default_rng(40 + len(name))
        dh, dhv = _operand(G.values(rng, (sc.P, C1), regime, -20, 127), "bf16", regime)
        return dict(sc=sc, dh=dh, dhv=dhv)
    return cache(("gsum", name, regime), build)


def _expect_rows(n_rows, fmt):
    return np.full((n_rows, C1), np.nan), np.zeros(n_rows, dtype=bool)


def _check_rows(regime, buf, rows, ref, mag, n, what, keep_bits=None):
    """Rows ``rows`` of ``buf`` against ref / mag / n (one line each); every other row must hold the fill (or ``keep_bits``)."""
    rows = np.asarray(rows)
    assert len(set(rows.tolist())) == len(rows), what + ": a row named twice"
    _check(regime, buf[_dev(rows).long()], ref, "bf16", what, mag=mag, n=n)
    other = np.ones(buf.shape[0], dtype=bool)
    other[rows] = False
    got = _bits(buf)[other]
    want = np.full_like(got, 0xFFFF) if keep_bits is None else keep_bits[other]
    assert np.array_equal(got, want), what + ": rows the kernel does not own were written"


@pytest.mark.parametrize("tables", ["prow", "source"])
@pytest.mark.parametrize("name,regime", [(n, r) for n in ("base", "subset", "groups", "groups_swap") for r in REGIMES] + [("partners513", "exact")])
def test_gradient_sums_compact(cache, name, regime, tables):
    L, lib = _lib()
    case, tb = _gsum_case(cache, name, regime), _tables(cache, name)
    sc = case["sc"]
    sp = sc.spaces["compact"]
    Gs, A, N, BG, BA, BN = cache(("gsum_ref", name, regime), lambda: G.gsum_reference(sc, case["dhv"], only_inside=True))
    if name.startswith("groups"):
        cnt = np.diff(tb["op_h"] if name.endswith("swap") else tb["sp_h"])
        assert {1, 15, 16, 17} <= set(cnt.tolist()) and np.diff(sc.img_ptr).tolist() == [0, 1, 8, 9, 17]
    if name == "partners513":
        assert np.diff(tb["sp_h"]).max() == 513 and np.diff(tb["op_h"]).max() == 513
    if regime == "exact" and name == "base":
        lost, half = G.rounding_cases(np.concatenate([Gs.reshape(-1), BG.reshape(-1)]), "bf16")
        assert lost > 0 and half > 0
    ins = np.tile(sc.inside, (2, 1))
    n_grp = int(lib.sgc_fc1_gsum_groups(sc.n, sc.n_img))
    part = _filled((n_grp * 64, C1), torch.float32)
    if tables == "prow":
        goff, prow, base = sp["goff"], sp["prow"], 0
        buf = _filled((sp["rows"] + 1, C1), torch.bfloat16)
        dh, keep = case["dh"], None
    else:                                                       # [rows of dh1][zero row][per-object rows]: what the row gather reads
        Ppad, cbase, prow = _row_source_tables(sc)
        goff = cbase
        buf = _filled((Ppad + 1 + int(sp["lead"].sum()) + 1, C1), torch.bfloat16)
        buf[:sc.P] = case["dh"]
        dh, keep = buf, _bits(buf).copy()
    _ok(lib.sgc_fc1_gsum_compact(L.ptr(dh), L.ptr(tb["bb"]), L.ptr(tb["sub"]), L.ptr(tb["obj"]), L.ptr(tb["sp"]), L.ptr(tb["sl"]), L.ptr(tb["op"]),
                                 L.ptr(tb["ol"]), L.ptr(tb["img_ptr"]), sc.n_img, L.ptr(_i32(goff)), L.ptr(_i32(prow)), sc.n, L.ptr(buf), L.ptr(part),
                                 L.stream_ptr()), "sgc_fc1_gsum_compact")
    bg_rows = np.array([goff[w] + b for b in range(sc.n_img) for w in range(64)], dtype=np.int64)
    rows = np.concatenate([prow.reshape(sc.n2, 64)[ins], bg_rows])
    ref = np.concatenate([Gs, BG.reshape(-1, C1)])
    mag = np.concatenate([A, BA.reshape(-1, C1)])
    n = np.concatenate([N, BN.reshape(-1, 1)])
    _check_rows(regime, buf, rows, ref, mag, n, "fc1_gsum_compact %s (%s)" % (name, tables), keep_bits=keep)


@pytest.mark.parametrize("regime", REGIMES)
def test_gradient_sums_full_rows(cache, regime):
    L, lib = _lib()
    case, tb = _gsum_case(cache, "base", regime), _tables(cache, "base")
    sc = case["sc"]
    sp = sc.spaces["full"]
    Gs, A, N = G.gsum_reference(sc, case["dhv"])[:3]
    buf = _filled((sp["rows"] + 1, C1), torch.bfloat16)
    _ok(lib.sgc_fc1_gsum(L.ptr(case["dh"]), L.ptr(tb["bb"]), L.ptr(tb["sub"]), L.ptr(tb["obj"]), L.ptr(tb["sp"]), L.ptr(tb["sl"]), L.ptr(tb["op"]),
                         L.ptr(tb["ol"]), L.ptr(_i32(sp["goff"])), sc.n, L.ptr(buf), L.stream_ptr()), "sgc_fc1_gsum")
    _check_rows(regime, buf, sp["prow"], Gs.reshape(-1, C1), A.reshape(-1, C1), N.reshape(-1, 1), "fc1_gsum base")


def test_x_rows_and_padding(cache):
    L, lib = _lib()
    case = _gsum_case(cache, "base", "exact")
    sc = case["sc"]
    sp = sc.spaces["full"]
    rows, E = sp["rows"], sc.E_all
    gwm, ywm = _filled((rows + 1, C1), torch.bfloat16), _filled((rows + 1, 1024), torch.bfloat16)
    _ok(lib.sgc_fc1_xrows(L.ptr(case["dh"]), L.ptr(_i32(sc.gather_all)), L.ptr(_i32(sp["dest"])), E, L.ptr(_i32(sp["goff"])), L.ptr(_i32(sp["gend"])),
                          L.ptr(gwm), L.ptr(ywm), L.stream_ptr()), "sgc_fc1_xrows")
    pad = np.zeros(rows + 1, dtype=bool)
    for g in range(64):
        pad[sp["gend"][g]:sp["goff"][g + 1]] = True
    want = np.full((rows + 1, C1), 0xFFFF, dtype=np.uint16)
    want[pad] = 0
    want[sp["dest"][:E]] = _bits(case["dh"])[sc.gather_all[:E] >> 6]
    assert pad.any() and np.array_equal(_bits(gwm), want)
    assert np.array_equal(_bits(ywm), np.where(pad[:, None], 0, 0xFFFF).astype(np.uint16) + np.zeros((1, 1024), dtype=np.uint16))


# ================================================================================================================= 4. linear pairs
C3 = 1024


def _linear_case(cache, name, regime):
    """raw pre-activations ([per-object entries | 64 windows per image], rows nobody names NaN), gradient rows and routing codes of the
    linear windows of one scene, with the forward's reference."""
    def build():
        sc = _scene(cache, name)
        sp = sc.spaces["compact"]
        rng = np.random.default_rng(60 + len(name))
        f32 = lambda a: a.astype(np.float32).astype(np.float64)
        raw_own = f32(G.values(rng, (sc.E_obj, 4, C3), regime, -1000, 2500))
        raw_bg = f32(G.values(rng, (sc.n_img, 64, 4, C3), regime, -1000, 2500))
        bias = f32(G.values(rng, (C3,), regime, -3, 3))
        pre, mag, used_own, used_bg = G.linear_pre_reference(sc, raw_own, raw_bg)
        raw = np.concatenate([np.where(used_own[:, None, None], raw_own, np.nan), np.where(used_bg[:, :, None, None], raw_bg, np.nan).reshape(-1, 4, C3),
                              np.full((1, 4, C3), np.nan)]).astype(np.float32)
        pos = {int(c): k for k, c in enumerate(sc.gather_all)}
        drow = np.array([sp["dest"][pos[int(c)]] for c in sc.gather_lin], dtype=np.int32)
        val, code = G.pool_reference(pre, bias)
        return dict(sc=sc, raw=_dev(raw), bias=_dev(bias, torch.float32), pre=pre, mag=mag + np.abs(bias), val=val, code=code, drow=drow, biasv=bias)
    return cache(("linear", name, regime), build)


@pytest.mark.parametrize("outputs", ["all", "y_only"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", ["base", "subset", "linear_objects"])
def test_linear_forward(cache, name, regime, outputs):
    L, lib = _lib()
    case, tb = _linear_case(cache, name, regime), _tables(cache, name)
    sc = case["sc"]
    sp = sc.spaces["compact"]
    pre, val, code, drow, EL = case["pre"], case["val"], case["code"], case["drow"], sc.E_lin
    assert EL > 0
    if regime == "exact":
        top = pre.max(1)
        ties = ((pre == top[:, None]).sum(1) > 1).sum()
        assert ties > 0 and (code == 4).sum() > 0 and (top + case["biasv"] == 0).sum() > 0      # ties, killed maxima, exact zeros
        for fmt in ("f16", "bf16"):
            lost, half = G.rounding_cases(val, fmt)
            assert lost > 0 and half > 0, fmt
    y, y_bf = _filled((sp["rows"] + 1, C3), torch.float16), _filled((sp["rows"] + 1, C3), torch.bfloat16)
    am = _filled(((sc.P + 1) * 64, C3), torch.uint8)
    dl = _filled((EL + 1,), torch.int32)
    every = outputs == "all"
    _ok(lib.sgc_windows_linear_forward(L.ptr(tb["bb"]), L.ptr(tb["sub"]), L.ptr(tb["obj"]), L.ptr(tb["obj_img"]), sc.n, sc.P, L.ptr(_i32(sc.gather_lin)),
                                       L.ptr(_i32([EL])), EL, L.ptr(_i32(sc.incl_all)), L.ptr(_i32(sp["dest"])), L.ptr(case["raw"]),
                                       ctypes.c_long(sc.E_obj), L.ptr(case["bias"]), L.ptr(y), L.ptr(y_bf if every else None),
                                       L.ptr(am if every else None), L.ptr(dl if every else None), L.stream_ptr()), "sgc_windows_linear_forward")
    what = "windows_linear_forward %s" % name
    assert len(set(drow.tolist())) == EL
    other = np.ones(sp["rows"] + 1, dtype=bool)
    other[drow] = False
    outs = [(y, "f16")] + ([(y_bf, "bf16")] if every else [])
    for t, fmt in outs:
        _check(regime, t[_dev(drow).long()], val, fmt, what + " " + fmt, mag=case["mag"].max(1), n=3)
        assert (_bits(t)[other] == 0xFFFF).all(), what + ": rows of other windows were written"
    if not every:
        for t in (y_bf, am, dl):
            _assert_fill(t, what + " (NULL outputs)")
        return
    assert np.array_equal(dl[:-1].cpu().numpy(), drow)
    _assert_fill(dl[-1:], "dest_linear")
    got = am.cpu().numpy().reshape(-1, C3)
    named = np.zeros(len(got), dtype=bool)
    named[sc.gather_lin] = True
    assert (got[~named] == 255).all(), what + ": routing rows of other windows were written"
    gc = got[sc.gather_lin]
    if regime == "exact":
        assert np.array_equal(gc, code), what + ": routing codes"
    else:                                                     # a route is right when its pixel is a maximum within the rounding of the three-term sums
        tol = 2 * 3 * 2.0 ** -24 * case["mag"].max(1)
        top = pre.max(1)
        alive = gc < 4
        pick = np.take_along_axis(pre, np.minimum(gc, 3)[:, None, :].astype(np.int64), axis=1)[:, 0]
        assert (gc <= 4).all() and (pick[alive] >= (top - tol)[alive]).all() and ((top + case["biasv"])[~alive] <= tol[~alive]).all()


def _linear_grads(cache, name, regime):
    """Pooled gradient rows (NaN where no linear window lives) and routing codes (0xFF likewise) for the linear windows."""
    def build():
        case = _linear_case(cache, name, regime)
        sc = case["sc"]
        sp = sc.spaces["compact"]
        rng = np.random.default_rng(80 + len(name))
        dyv = G.values(rng, (sc.E_lin, C3), regime, -20, 127)
        dy = np.full((sp["rows"] + 1, C3), np.nan)
        dy[case["drow"]] = dyv
        dy_d = _dev(dy, torch.float64).to(torch.bfloat16)
        dyv = dy_d[_dev(case["drow"]).long()].double().cpu().numpy()
        code = rng.integers(0, 5, (sc.E_lin, C3)).astype(np.uint8)
        am = np.full(((sc.P + 1) * 64, C3), 255, dtype=np.uint8)
        am[sc.gather_lin] = code
        return dict(dy=dy_d, dyv=dyv, code=code, am=_dev(am), un=G.unpool(dyv, code))
    return cache(("linear_grads", name, regime), build)


@pytest.mark.parametrize("regime", REGIMES)
def test_linear_backward_objects(cache, regime):
    L, lib = _lib()
    name = "linear_objects"
    case, gr, tb = _linear_case(cache, name, regime), _linear_grads(cache, name, regime), _tables(cache, name)
    sc = case["sc"]
    sp = sc.spaces["compact"]
    e0, n_pe = sc.E_conv, sc.E_obj
    # the definition: entry (ps, w) collects the linear pairs of its object (in its role) whose X rectangle holds w
    add, mag, cnt = np.zeros((n_pe, 4, C3)), np.zeros((n_pe, 4, C3)), np.zeros(n_pe, dtype=np.int64)
    for t, c in enumerate(sc.gather_lin):
        p, w = c >> 6, c & 63
        for k in (sc.obj_entry[sc.sub[p], w], sc.obj_entry[sc.n + sc.obj[p], w]):
            add[k] += gr["un"][t]
            mag[k] += np.abs(gr["un"][t])
            cnt[k] += 1
    assert {0, 1, 2} <= set(cnt.tolist()) and cnt.max() > 64
    rng = np.random.default_rng(9)
    old, oldv = _operand(G.values(rng, (e0 + n_pe + 1, 4, C3), regime, -100, 100), "bf16", regime)
    untouched = np.concatenate([np.ones(e0, bool), cnt == 0, [True]])
    junk = _dev(rng.integers(0, 65536, (int(untouched.sum()), 4, C3)).astype(np.uint16).view(np.int16)).view(torch.bfloat16)
    old[_dev(untouched)] = junk                                                  # whatever an untouched entry holds, it keeps
    before = _bits(old).copy()
    _ok(lib.sgc_windows_linear_backward_objects(L.ptr(tb["bb"]), L.ptr(tb["sub"]), L.ptr(tb["obj"]), L.ptr(tb["sp"]), L.ptr(tb["sl"]), L.ptr(tb["op"]),
                                                L.ptr(tb["ol"]), sc.n, sc.P, L.ptr(_i32(sc.gather_conv)), e0, n_pe, L.ptr(_i32(sc.incl_all)),
                                                L.ptr(_i32(sp["dest"])), L.ptr(gr["dy"]), L.ptr(gr["am"]), L.ptr(old), L.stream_ptr()),
        "sgc_windows_linear_backward_objects")
    after = _bits(old)
    assert np.array_equal(after[untouched], before[untouched]), "untouched entries changed"
    tch = ~untouched
    k = tch[e0:e0 + n_pe]
    _check(regime, old[_dev(tch)], oldv[tch] + add[k], "bf16", "windows_linear_backward_objects", mag=np.abs(oldv[tch]) + mag[k],
           n=(cnt[k] + 1)[:, None, None])


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", ["base", "linear"])
def test_linear_backward_background(cache, name, regime):
    L, lib = _lib()
    case, gr = _linear_case(cache, name, regime), _linear_grads(cache, name, regime)
    sc = case["sc"]
    n_img = sc.n_img
    code_l = sc.gather_lin.astype(np.int64)
    keys = sc.obj_img[sc.sub[code_l >> 6]].astype(np.int64) * 64 + (code_l & 63)          # as the plan builds them: a stable sort by (image, window)
    order = np.argsort(keys, kind="stable").astype(np.int32)
    seg = np.searchsorted(keys[order], np.arange(64 * n_img + 1)).astype(np.int32)
    assert name != "linear" or {0, 1, 3, 4, 5, 16, 17, 65} <= set(np.diff(seg).tolist())
    tb = _tables(cache, name)
    order_d, seg_d = _filled((sc.E_lin,), torch.int32), _filled((64 * n_img + 1,), torch.int32)
    _ok(lib.sgc_bucket_place(L.ptr(_i32(sc.gather_lin)), sc.E_lin, L.ptr(tb["sub"]), L.ptr(tb["obj_img"]), 1, 64 * n_img, L.ptr(None), L.ptr(order_d),
                             L.ptr(seg_d), 1, L.stream_ptr()), "sgc_bucket_place")
    assert np.array_equal(order_d.cpu().numpy(), order) and np.array_equal(seg_d.cpu().numpy(), seg)      # what the plan hands the kernel
    acc, mag, cnt = np.zeros((64 * n_img, 4, C3)), np.zeros((64 * n_img, 4, C3)), np.diff(seg)
    np.add.at(acc, keys, gr["un"])
    np.add.at(mag, keys, np.abs(gr["un"]))
    rng = np.random.default_rng(10)
    intv = G.values(rng, (n_img, 16, 16, C3), regime, -100, 100)
    bgp = _filled((n_img + 1, 18, 18, C3), torch.bfloat16)                                 # halo and the slab behind: fill
    bgp[:n_img, 1:17, 1:17] = _dev(intv, torch.float64).to(torch.bfloat16)
    intv = bgp[:n_img, 1:17, 1:17].double().cpu().numpy()
    bpart = _filled((64 * n_img + 1, C3), torch.float32)
    _ok(lib.sgc_windows_linear_backward_bg(L.ptr(_i32(sc.gather_lin)), L.ptr(_i32(case["drow"])), L.ptr(_i32(order)), L.ptr(_i32(seg)), n_img,
                                           L.ptr(gr["dy"]), L.ptr(gr["am"]), L.ptr(bgp), L.ptr(bpart), L.stream_ptr()), "sgc_windows_linear_backward_bg")
    # interior pixel (2 wy + qy, 2 wx + qx) of image b  -=  the routed sum of slot q of window w
    a6 = acc.reshape(n_img, 8, 8, 2, 2, C3).transpose(0, 1, 3, 2, 4, 5).reshape(n_img, 16, 16, C3)
    m6 = mag.reshape(n_img, 8, 8, 2, 2, C3).transpose(0, 1, 3, 2, 4, 5).reshape(n_img, 16, 16, C3)
    n6 = np.repeat(np.repeat(cnt.reshape(n_img, 8, 8), 2, 1), 2, 2)[..., None]
    if regime == "exact" and name == "linear":
        lost, half = G.rounding_cases(intv - a6, "bf16")
        assert lost > 0 and half > 0
    _check(regime, bgp[:n_img, 1:17, 1:17], intv - a6, "bf16", "windows_linear_backward_bg %s map" % name, mag=np.abs(intv) + m6, n=n6 + 1)
    halo = _bits(bgp).copy()
    halo[:n_img, 1:17, 1:17] = 0xFFFF
    assert (halo == 0xFFFF).all(), "halo or the slab behind the maps was written"
    _check(regime, bpart[:-1], acc.sum(1), "f32", "windows_linear_backward_bg %s bias" % name, mag=mag.sum(1), n=(cnt + 4)[:, None])
    _assert_fill(bpart[-1:], "bias_part")


# ================================================================================================================= 5. conv3 data-gradient tail
C2 = 512


@pytest.mark.parametrize("split", ["none", "all", "inside"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", ["base", "subset"])
def test_patch_sums(cache, name, regime, split):
    L, lib = _lib()
    sc, tb = _scene(cache, name), _tables(cache, name)
    Et, P, Pt = len(sc.gather_conv), sc.P, sc.P + sc.n2
    n16 = {"none": 0, "all": Et, "inside": max(1, sc.E_conv // 2)}[split]
    assert 0 < sc.E_conv and sc.linear.any() and (split != "inside" or 0 < n16 < sc.E_conv)
    rng = np.random.default_rng(100 + n16)
    a, av = _operand(G.values(rng, (Et, 16, C2), regime, -20, 127), "bf16", regime)
    b, bv = _operand(G.values(rng, (Et, 16, C2), regime, -20, 127), "bf16", regime)
    two = (np.arange(Et) >= n16)[:, None, None] & np.array(G.PATCH_CENTRE)[None, :, None]     # centre pixels of the 20-row layout: two slots
    V, A = av + np.where(two, bv, 0.0), np.abs(av) + np.where(two, np.abs(bv), 0.0)
    n_rows = 16 * n16 + G.PATCH_SLOTS * (Et - n16)
    patch = torch.full((n_rows + 1, C2), float("nan"), device=DEV).bfloat16()
    if n16:
        patch[:16 * n16] = a[:n16].reshape(-1, C2)
    if Et > n16:
        r20 = patch[16 * n16:n_rows].view(Et - n16, G.PATCH_SLOTS, C2)
        slot = torch.tensor(G.PATCH_ROW20, device=DEV)
        r20[:, slot] = a[n16:]
        cen = torch.tensor([k for k in range(16) if G.PATCH_CENTRE[k]], device=DEV)
        r20[:, slot[cen] + 1] = b[n16:][:, cen]
        assert not torch.isnan(r20.float()).any()
    dz = _filled(((Pt + 1) * 256, C2), torch.bfloat16)
    incl = _i32(sc.incl_conv)
    _ok(lib.sgc_windows_patch_sum2(L.ptr(patch), n16, L.ptr(tb["bb"]), L.ptr(tb["sub"]), L.ptr(tb["obj"]), L.ptr(incl), P, L.ptr(dz), L.stream_ptr()),
        "sgc_windows_patch_sum2")
    _ok(lib.sgc_windows_patch_sum_objects2(L.ptr(patch), n16, L.ptr(tb["bb"]), sc.n, P, L.ptr(incl), L.ptr(dz), L.stream_ptr()),
        "sgc_windows_patch_sum_objects2")
    ref, mag, cnt = G.patch_sum_reference(sc, V, A, sc.incl_conv, sc.gather_conv, 0, Pt)
    pix = np.concatenate([sc.pixrect_conv, sc.pixrect_obj])
    live = np.stack([G.pixrect_mask(int(r)) for r in pix])                                   # where dz exists: the pair's pixel rectangle
    assert np.array_equal(live, cnt[..., 0] > 0)
    Y, X = np.mgrid[0:16, 0:16]
    rows = (np.arange(Pt)[:, None, None] * 256 + G.pixel_row(Y, X)[None])[live]
    if regime == "exact":
        lost, half = G.rounding_cases(ref[live], "bf16")
        assert lost > 0 and half > 0
    _check_rows(regime, dz, rows, ref[live], mag[live], cnt[live], "windows_patch_sum2 %s n16 = %s" % (name, split))
    if split == "none":
        dz1 = _filled(((Pt + 1) * 256, C2), torch.bfloat16)
        _ok(lib.sgc_windows_patch_sum(L.ptr(patch), L.ptr(tb["bb"]), L.ptr(tb["sub"]), L.ptr(tb["obj"]), L.ptr(incl), P, L.ptr(dz1), L.stream_ptr()),
            "sgc_windows_patch_sum")
        assert np.array_equal(_bits(dz1[:P * 256]), _bits(dz[:P * 256]))
        _assert_fill(dz1[P * 256:], "dz of sgc_windows_patch_sum")


@pytest.mark.parametrize("role", [0, 1])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", ["base", "contract"])
def test_pair_contraction(cache, name, regime, role):
    L, lib = _lib()
    sc, tb = _scene(cache, name), _tables(cache, name)
    n, P, n_img = sc.n, sc.P, sc.n_img
    Pt = P + sc.n2 + n_img
    pix = np.concatenate([sc.pixrect_conv, sc.pixrect_obj, [G.FULL_PIXRECT] * n_img]).astype(np.int32)
    live = np.stack([G.pixrect_mask(int(r)) for r in pix])
    rng = np.random.default_rng(120 + role)
    dzv = np.where(live[..., None], G.values(rng, (Pt, 16, 16, C2), regime, -20, 127), np.nan)       # dz does not exist outside the rectangle
    Y, X = np.mgrid[0:16, 0:16]
    m3 = G.pixel_row(Y, X).reshape(-1)
    dz_rows = np.full((Pt + 1, 256, C2), np.nan)
    dz_rows[:Pt, m3] = dzv.reshape(Pt, 256, C2)
    dz = _dev(dz_rows, torch.float64).to(torch.bfloat16)
    dzv = dz[:Pt].double().cpu().numpy()[:, m3].reshape(Pt, 16, 16, C2)
    codes = rng.choice(np.array([0, 1, 2, 3, 4, 15], dtype=np.uint8), (Pt, 16, 16, C2))
    amz = _dev((codes[..., 0::2] | (codes[..., 1::2] << 4)).reshape(Pt, 256, 256))               # 4 bits per channel, pixel-major (W = 16 Y + X)
    ptr, lst = (tb["op"], tb["ol"]) if role else (tb["sp"], tb["sl"])
    ref, mag, cnt = G.contract_reference(sc, role, np.nan_to_num(dzv), codes, pix, 0)
    for bg_maps in (0, 1):
        for b in range(n_img if bg_maps else 0):                   # the all-background map of the image joins its background object
            k = P + sc.n2 + b
            ref[n + b] += G.unpool(dzv[k], codes[k])
            mag[n + b][:, :, 0] += np.abs(dzv[k])
            cnt[n + b] += 1
        real = cnt[:n, :, :, 0, 0] - live[P + (n if role else 0):P + (n if role else 0) + n]       # candidates of the list, without the pseudo-pair
        if name == "contract":
            assert {0, 1, 4, 5, 8, 9} <= set(real[1][live[P + (n if role else 0) + 1]].tolist()) and real[0].max() == 70
            assert cnt[n].max() >= 72 + bg_maps and (cnt[2:n] == 0).any()
        dU = _filled((n + n_img + 1, 34, 34, C2), torch.bfloat16)
        _ok(lib.sgc_pair_contract_windows(L.ptr(dz), L.ptr(amz), L.ptr(ptr), L.ptr(lst), L.ptr(_i32(pix)), L.ptr(tb["img_ptr"]), role, P, n, n_img,
                                          bg_maps, L.ptr(dU), L.stream_ptr()), "sgc_pair_contract_windows")
        inner = dU[:n + n_img, 1:33, 1:33].reshape(n + n_img, 16, 2, 16, 2, C2).permute(0, 1, 3, 2, 4, 5).reshape(n + n_img, 16, 16, 4, C2)
        if regime == "exact":
            lost, half = G.rounding_cases(ref, "bf16")
            assert lost > 0 and half > 0
        _check(regime, inner, ref, "bf16", "pair_contract_windows %s role %d bg_maps %d" % (name, role, bg_maps), mag=mag, n=cnt)
        ring = _bits(dU).copy()
        ring[:n + n_img, 1:33, 1:33] = 0xFFFF
        assert (ring == 0xFFFF).all(), "halo ring or the map behind was written"
        zero = cnt[:, :, :, 0, 0] == 0                                                            # cells outside the pseudo-pair's rectangle: exact zeros
        assert zero.any() and (_bits(inner)[zero] == 0).all()


def test_worst_ratios_are_reported():
    """Prints the worst got / bound of every REAL test of this run (pytest -s), so that one line per test lands in the profile."""
    for what in sorted(WORST):
        print("SHARED-GLUE worst %-70s %.4f" % (what, WORST[what]))
    assert all(v <= 1.0 for v in WORST.values())
