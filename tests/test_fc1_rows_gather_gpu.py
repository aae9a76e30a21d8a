"""fc1 backward with the gradient rows read through a row table (``TUNING.fc1_rows_gather``; csrc/kernels_fc1_rows.hip): the two grouped
GEMMs gather row ``rowsrc[r]`` of the source buffer [rows of dh1][zero row][per-object rows] instead of reading a window-major copy.

Every A value and every K position is where the copy path has it, so everything is compared with ``torch.equal``:

  * the data-gradient entry against ``sgc_fc1_xrows`` + ``sgc_fc1_windows_dgrad`` on 256 and 768 rows (one and three M tiles);
  * the weight-gradient entry against ``sgc_fc1_xrows`` + ``sgc_fc1_windows_wgrad`` on 64 groups of 64 / 128 / 192 / 320 rows (one, two
    and three K tiles - prologue only, no steady state - and the steady loop);
  * both on a table that names the last row of a 2 GiB source (the reach of the blocks' 32-bit offsets), and the refusal above it;
  * one training step of a small scene with the switch on and off.

The tables hold what the step's table holds: a source row used in several tiles / groups, the zero row, per-object rows behind it, and
source rows in descending order.  Outputs are pre-filled with 0xFF bytes."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
LIMIT = 262144                      # rows of 4096 bf16 in 2 GiB


def _lib():
    from scene_graph_commonsense_amd import _lib
    return _lib.load(), _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _filled(n, dtype):
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    return torch.full((n,), -1, dtype=bits, device=DEV).view(dtype)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _table(rows, n_pairs, n_objrows, seed, pinned=()):
    """rowsrc [rows] over a source of n_pairs + 1 + n_objrows rows: a run of per-object rows, a descending run of pair rows, ONE pair row
    repeated at the same position of every 256-row tile (and so in several tiles / groups), random pair rows, zero-row padding at the end
    of every 64 rows; ``pinned``: (position, source row) pairs set last."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, n_pairs, (rows,), generator=g, dtype=torch.int32)
    zero_row = n_pairs
    n_o = min(n_objrows, 24)
    t[:n_o] = torch.arange(zero_row + 1, zero_row + 1 + n_o, dtype=torch.int32)                    # per-object rows
    t[32:56] = torch.arange(n_pairs - 1, n_pairs - 25, -1, dtype=torch.int32)                        # descending
    t[7::256] = 5                                                                                   # the same source row in every tile
    t[60::64] = zero_row                                                                            # padding -> the zero row
    t[61::64] = zero_row
    for pos, row in pinned:
        t[pos] = row
    return t.to(DEV)


def _source(n_rows, zero_row, used=None, seed=0):
    """gsrc [n_rows][4096] bf16: random rows, one zero row.  ``used``: only these rows are written (a 2 GiB buffer stays unfilled)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if used is None:
        src = torch.randn(n_rows, 4096, generator=g, device=DEV).to(torch.bfloat16)
    else:
        src = torch.empty(n_rows, 4096, dtype=torch.bfloat16, device=DEV)
        u = torch.unique(used.long())
        src[u] = torch.randn(u.numel(), 4096, generator=g, device=DEV).to(torch.bfloat16)
    src[zero_row].zero_()
    return src


def _gwm_by_xrows(src, rowsrc, goff65):
    """The window-major copy the plain entries read, made by the step's own copy kernel: entry e = row e, its pair = rowsrc[e]."""
    lib, L = _lib()
    rows = rowsrc.numel()
    gwm = _filled(rows * 4096, torch.bfloat16)
    ybf_dummy = torch.zeros(rows * 1024, dtype=torch.bfloat16, device=DEV)
    gather = (rowsrc * 64).contiguous()
    dest = torch.arange(rows, dtype=torch.int32, device=DEV)
    gend = goff65[1:].contiguous()                       # no padding rows of its own: the table's zero-row entries are the padding
    L.check(lib.sgc_fc1_xrows(L.ptr(src), L.ptr(gather), L.ptr(dest), rows, L.ptr(goff65), L.ptr(gend), L.ptr(gwm), L.ptr(ybf_dummy),
                              _stream()), "sgc_fc1_xrows")
    torch.cuda.synchronize()
    assert torch.equal(_bits(gwm).view(rows, 4096), _bits(src)[rowsrc.long()])
    return gwm


def _goff65(group_rows):
    """[65] group offsets; fewer than 64 groups: the rest are empty."""
    sizes = list(group_rows) + [0] * (64 - len(group_rows))
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), device=DEV)


@pytest.fixture(scope="module")
def weights():
    """w1pT rows of four window groups [4 * 1024][4096] bf16 and the operands of the weight gradient, built once."""
    g = torch.Generator(device=DEV).manual_seed(11)
    w = (torch.randn(4 * 1024, 4096, generator=g, device=DEV) * 0.05).to(torch.bfloat16)
    yield w
    torch.cuda.empty_cache()


def _dgrad_both(src, rowsrc, w1pT, tile_group, rows, src_rows):
    lib, L = _lib()
    gwm = _gwm_by_xrows(src, rowsrc, _goff65([rows]))
    want, got = _filled(rows * 1024, torch.bfloat16), _filled(rows * 1024, torch.bfloat16)
    L.check(lib.sgc_fc1_windows_dgrad(L.ptr(gwm), L.ptr(w1pT), L.ptr(tile_group), L.ptr(want), rows, _stream()), "sgc_fc1_windows_dgrad")
    L.check(lib.sgc_fc1_windows_dgrad_rows(L.ptr(src), L.ptr(rowsrc), src_rows, L.ptr(w1pT), L.ptr(tile_group), L.ptr(got), rows, _stream()),
            "sgc_fc1_windows_dgrad_rows")
    torch.cuda.synchronize()
    assert torch.isfinite(want.float()).all()                       # every element written
    return want, got


@pytest.mark.parametrize("rows", [256, 768])
def test_data_gradient_entry_equals_the_copy_path(rows, weights):
    n_pairs, n_obj = 300, 40
    src = _source(n_pairs + 1 + n_obj, n_pairs, seed=rows)
    rowsrc = _table(rows, n_pairs, n_obj, seed=rows + 1)
    tile_group = torch.tensor([2, 0, 3][:rows // 256], dtype=torch.int32, device=DEV)
    want, got = _dgrad_both(src, rowsrc, weights, tile_group, rows, n_pairs + 1 + n_obj)
    assert torch.equal(_bits(got), _bits(want))
    zero = (rowsrc == n_pairs).nonzero().flatten()
    assert zero.numel() > 0 and not got.view(rows, 1024)[zero].float().abs().any()         # zero-row entries give zero rows


def _wgrad_both(src, rowsrc, group_rows, src_rows, seed):
    lib, L = _lib()
    goff = _goff65(group_rows)
    rows = int(goff[64])
    assert rowsrc.numel() == rows
    gwm = _gwm_by_xrows(src, rowsrc, goff)
    g = torch.Generator(device=DEV).manual_seed(seed)
    ybf = torch.randn(rows, 1024, generator=g, device=DEV).to(torch.bfloat16)
    want, got = _filled(4096 * 65536, torch.float32), _filled(4096 * 65536, torch.float32)
    L.check(lib.sgc_fc1_windows_wgrad(L.ptr(gwm), L.ptr(ybf), L.ptr(goff), L.ptr(want), rows, _stream()), "sgc_fc1_windows_wgrad")
    L.check(lib.sgc_fc1_windows_wgrad_rows(L.ptr(src), L.ptr(rowsrc), src_rows, L.ptr(ybf), L.ptr(goff), L.ptr(got), rows, _stream()),
            "sgc_fc1_windows_wgrad_rows")
    torch.cuda.synchronize()
    assert torch.isfinite(want).all()
    return want, got


def test_weight_gradient_entry_equals_the_copy_path():
    sizes = [(64, 128, 192, 320)[(3 * g + g // 4) % 4] for g in range(64)]           # unequal lengths, mixed: 1, 2, 3 and 5 K tiles
    assert {64, 128, 192, 320} == set(sizes) and len(sizes) == 64
    rows = sum(sizes)
    n_pairs, n_obj = 700, 40
    src = _source(n_pairs + 1 + n_obj, n_pairs, seed=5)
    rowsrc = _table(rows, n_pairs, n_obj, seed=6)
    want, got = _wgrad_both(src, rowsrc, sizes, n_pairs + 1 + n_obj, seed=7)
    assert torch.equal(_bits(got), _bits(want))


def test_last_row_of_a_2_gib_source_is_exact(weights):
    """Row 262143 lies 8 KiB below 2 GiB: the largest offset the blocks form is 2^31 - 16.  Both entries on a table that names it (at
    the first and the last lane position of a tile and of a K tile) next to low rows; the buffer is otherwise unfilled."""
    zero_row, n_pairs = 1000, 1000
    pinned = [(0, LIMIT - 1), (255, LIMIT - 1), (63, LIMIT - 1), (64, LIMIT - 2), (130, LIMIT - 1)]
    rows = 256
    rowsrc = _table(rows, n_pairs, 24, seed=21, pinned=pinned)
    src = _source(LIMIT, zero_row, used=rowsrc, seed=22)
    assert src.numel() * 2 == 1 << 31
    tile_group = torch.tensor([1], dtype=torch.int32, device=DEV)
    want, got = _dgrad_both(src, rowsrc, weights, tile_group, rows, LIMIT)
    assert torch.equal(_bits(got), _bits(want))
    assert got.view(rows, 1024)[0].float().abs().max() > 0                               # the far row is data, not zeros
    want, got = _wgrad_both(src, rowsrc, [64, 128, 64], LIMIT, seed=23)
    assert torch.equal(_bits(got), _bits(want))
    del want, got, src
    torch.cuda.empty_cache()


def test_a_source_past_2_gib_is_refused_and_nothing_is_launched(weights):
    lib, L = _lib()
    rows = 256
    rowsrc = _table(rows, 1000, 24, seed=31, pinned=[(17, LIMIT)])                        # names row 262144
    src = torch.zeros(8, 4096, dtype=torch.bfloat16, device=DEV)                          # never read
    tile_group = torch.tensor([0], dtype=torch.int32, device=DEV)
    dy = _filled(rows * 1024, torch.bfloat16)
    assert lib.sgc_fc1_windows_dgrad_rows(L.ptr(src), L.ptr(rowsrc), LIMIT + 1, L.ptr(weights), L.ptr(tile_group), L.ptr(dy), rows,
                                          _stream()) == 1                                # SGC_ERR_ARG
    goff = _goff65([64, 128, 64])
    ybf = torch.zeros(rows * 1024, dtype=torch.bfloat16, device=DEV)
    dw = _filled(4096 * 65536, torch.float32)
    assert lib.sgc_fc1_windows_wgrad_rows(L.ptr(src), L.ptr(rowsrc), LIMIT + 1, L.ptr(ybf), L.ptr(goff), L.ptr(dw), rows, _stream()) == 1
    torch.cuda.synchronize()
    assert (_bits(dy) == -1).all() and (_bits(dw) == -1).all()


def test_row_table_names_only_rows_of_the_source_whatever_the_lists_hold():
    """``sgc_window_rows_source`` on lists that do not match the host's tables (what a scene edited after flattening leaves behind,
    tests/test_scene_gpu.py): destinations outside the row space are not written, sources that are no pair row become the zero row, a
    carried ``prow`` stays inside its group's per-object rows, and a row nobody names keeps the preset zero row.  The GEMMs form
    addresses from this table."""
    lib, L = _lib()
    lead, n_x, zero_row = 3, 5, 64                                     # per group: 3 per-object rows, 5 X rows, padded to 256
    goff = torch.arange(65, dtype=torch.int32) * 256
    xbase, gend = goff[:64] + lead, goff[:64] + lead + n_x
    cbase = zero_row + 1 + torch.arange(64, dtype=torch.int32) * lead
    rows = int(goff[64])
    dest = torch.tensor([3, 4, 5, -7, rows, rows + 100, 259, 260], dtype=torch.int32)
    code = torch.tensor([10, 63, 64, 1, 2, 3, 1 << 20, -5], dtype=torch.int32) * 64 + 9          # pair * 64 + window
    prow = torch.zeros(2 * 64, dtype=torch.int32)
    prow[:64] = goff[:64] + 1                                          # inside the per-object rows
    prow[64:] = goff[:64] + 200                                        # far behind them
    rowsrc = torch.full((rows,), zero_row, dtype=torch.int32, device=DEV)
    prow_src = torch.full((128,), -1, dtype=torch.int32, device=DEV)
    d = lambda t: t.to(DEV)
    tabs = [d(t.contiguous()) for t in (code, dest, goff, xbase, gend, cbase, prow)]
    L.check(lib.sgc_window_rows_source(L.ptr(tabs[0]), L.ptr(tabs[1]), dest.numel(), L.ptr(tabs[2]), L.ptr(tabs[3]), L.ptr(tabs[4]),
                                       L.ptr(tabs[5]), zero_row, lead + 256, L.ptr(tabs[6]), 128, rows, L.ptr(rowsrc), L.ptr(prow_src),
                                       _stream()), "sgc_window_rows_source")
    torch.cuda.synchronize()
    got, n_src = rowsrc.cpu(), zero_row + 1 + 64 * lead
    assert int(got.min()) >= 0 and int(got.max()) < n_src
    want = torch.full((rows,), zero_row, dtype=torch.int32)
    for w in range(64):
        want[w * 256:w * 256 + lead] = cbase[w] + torch.arange(lead, dtype=torch.int32)
    want[3], want[4], want[5] = 10, 63, zero_row                      # pair rows 10 and 63; 64 is no pair row
    want[259], want[260] = zero_row, zero_row                         # sources far outside / negative
    assert torch.equal(got, want)
    ps = prow_src.cpu()
    assert torch.equal(ps[:64], cbase + 1) and torch.equal(ps[64:], cbase + lead - 1)


def _train_step(gather):
    """One training step of 2 images x 6 objects (second level, compact rows) with the switch on / off, on a fresh engine."""
    from scene_graph_commonsense_amd import engine
    from scene_graph_commonsense_amd.engine import RelHeadEngine, csr_by, loss_coefficients
    from scene_graph_commonsense_amd.model import _shared_hint
    from scene_graph_commonsense_amd.pairs import flatten_scene, pair_targets
    from scene_graph_commonsense_amd.synthetic import HeadConfig, make_scene_batch, make_state_dict, predicate_counts
    cfg = HeadConfig()
    sd = make_state_dict(cfg, seed=3, head_gain=4.0)
    batch = make_scene_batch(cfg, [6, 6], seed=23, connect_frac=0.4)
    with engine.tuning(fc1_rows_gather=gather, shared_max_fraction=2.0):
        eng = RelHeadEngine(cfg, "cuda:0")
        eng.load_weights(sd)
        eng.prep_bwd_weights(sd)
        sc = flatten_scene(cfg, batch, "cuda:0")
        pidx = sc.pidx
        directed, _ = pair_targets(batch.relationships, batch.subj_or_obj, pidx)
        counts = predicate_counts(cfg).numpy()
        coefs = loss_coefficients(cfg, pidx.step, len(pidx.call_sizes), directed, 1 - counts / counts.sum())
        coefs_d = tuple(torch.from_numpy(c).to("cuda:0") for c in coefs)
        n_obj = int(sc.obj_img.shape[0])
        sub_csr = tuple(torch.from_numpy(a).to("cuda:0") for a in csr_by(pidx.sub, n_obj))
        obj_csr = tuple(torch.from_numpy(a).to("cuda:0") for a in csr_by(pidx.obj, n_obj))
        img_ptr = torch.from_numpy(pidx.obj_offset.astype(np.int32)).to("cuda:0")
        ctx = eng.train_forward(sc.image_feature, sc.image_depth, sc.obj_img, sc.bbox, sc.cats, sc.super_mh, sc.sub_idx, sc.obj_idx,
                                dropout=True, seeds=(11, 12), dense=(sc.img_ptr, sc.pid, sc.max_n), shared_windows=_shared_hint(sc))
        wm = ctx.shared["wm"]
        assert wm["prow"] is not None and (wm["rowsrc"] is not None) == gather          # second level, compact rows
        loss, grads = eng.train_backward(ctx, coefs_d, sub_csr, obj_csr, img_ptr)
        torch.cuda.synchronize()
        names = set(eng.scratch.bufs)
        virtual_gwm = eng.scratch.bufs["gwm"][:wm["rows"] * 4096].clone()
    return float(loss), {k: v.clone() for k, v in grads.items()}, names, virtual_gwm


def test_training_step_is_bit_identical_with_the_switch_on_and_off():
    l_on, g_on, names_on, gwm_on = _train_step(True)
    l_off, g_off, names_off, gwm_off = _train_step(False)
    assert "gwm" in names_off and "dh1" in names_off and "fc1_gsrc" not in names_off
    assert "gwm" not in names_on and "dh1" not in names_on and "fc1_gsrc" in names_on        # no window-major gradient is allocated
    assert l_on == l_off
    assert set(g_on) == set(g_off)
    for n in sorted(g_on):
        assert torch.equal(g_on[n], g_off[n]), n
    # what the GEMMs gathered is what the copy path wrote, row for row (the padding rows too)
    assert torch.equal(_bits(gwm_on), _bits(gwm_off))
