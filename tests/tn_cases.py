"""Float64 references and operand builders for the direct tests of the TN GEMM family - the weight gradients (csrc/gemm_tn.h,
csrc/gemm_tn_pp_tile.h, csrc/gemm_tn_sp.h; GPU tests: tests/test_tn_blocks_gpu.py, self-test: tests/test_tn_cases_cpu.py).  Plain torch, no
project kernel.  The two data regimes, ``exact_operands``, ``assert_exact`` and ``acc_bound`` are those of tests/nt_epilogue_cases.py.

All references take the operands as the kernel sees them (already rounded to bf16 / f16) and return float64 on the operands' device."""
import torch

from tests import nt_epilogue_cases as C

M3, CIN3, N3 = 1024, 512, 9 * 512            # conv3: output channels, input channels, columns of its weight gradient


# ------------------------------------------------------------------------------------------------------------------ references
def tn_ref(A, B):
    """A [K][M], B [K][N] -> A^T B."""
    return A.double().t() @ B.double()


def conv_wgrad_ref(dy_pad, x_pad, lgS):
    """3x3 convolution weight gradient as nine shifted products over the centre pixels.  dy_pad [n][S+2][S+2][M] (its ring is NOT
    read), x_pad [n][S+2][S+2][Cin] (its ring is the zero padding and IS read).  Returns [M][9*Cin], columns in (tap, c) order."""
    S = 1 << lgS
    M, Cin = dy_pad.shape[3], x_pad.shape[3]
    dy = dy_pad[:, 1:S + 1, 1:S + 1, :].double().reshape(-1, M)
    out = torch.zeros(M, 9, Cin, dtype=torch.float64, device=dy.device)
    for tap in range(9):
        ky, kx = tap // 3, tap % 3
        out[:, tap] = dy.t() @ x_pad[:, ky:ky + S, kx:kx + S, :].double().reshape(-1, Cin)
    return out.reshape(M, 9 * Cin)


def unpool_rows(dy, code):
    """Un-pooled rows of a routed gradient: row 4e + q = dy[e] where code[e] == q, else 0; a code of 4 and above gives nothing."""
    E, Cc = dy.shape
    out = torch.zeros(E, 4, Cc, dtype=dy.dtype, device=dy.device)
    for q in range(4):
        out[:, q] = torch.where(code == q, dy, torch.zeros((), dtype=dy.dtype, device=dy.device))
    return out.reshape(4 * E, Cc)


def list_patches(gather, z_pad):
    """The 4 x 4 input patches [E][4][4][Cin] (dtype of z_pad) of the listed windows: window gather[e] & 63 of map gather[e] >> 6."""
    g = torch.as_tensor(gather).long().to(z_pad.device)
    img, W = g >> 6, g & 63
    r = torch.arange(4, device=z_pad.device)
    iy = (2 * (W >> 3)).unsqueeze(1) + r
    ix = (2 * (W & 7)).unsqueeze(1) + r
    return z_pad[img[:, None, None], iy[:, :, None], ix[:, None, :], :]


def list_wgrad_ref(dy_rows, code_rows, gather, dest, z_pad, chunk=8192):
    """conv3 weight gradient over a window list: dW[oc][(tap, c)] = sum over the entries e and the pixels q = (qy, qx) of their windows of
    dy_rows[dest[e]][oc] * (code_rows[gather[e]][oc] == q) * patch_e[(qy + ky) * 4 + qx + kx][c] - 4 x 9 matmuls over the gathered
    patches.  f16 maps are rounded to bf16 first (torch's round-to-nearest-even: the operand of the sparse block that reads f16 maps)."""
    dev = z_pad.device
    g = torch.as_tensor(gather).long().to(dev)
    d = torch.as_tensor(dest).long().to(dev)
    M, Cin = dy_rows.shape[1], z_pad.shape[3]
    out = torch.zeros(M, 9, Cin, dtype=torch.float64, device=dev)
    for e0 in range(0, g.numel(), chunk):
        ge, de = g[e0:e0 + chunk], d[e0:e0 + chunk]
        dy = dy_rows[de].double()
        code = code_rows[ge]
        patch = list_patches(ge, z_pad)
        if patch.dtype == torch.float16:
            patch = patch.to(torch.bfloat16)
        patch = patch.double()
        for q in range(4):
            a = torch.where(code == q, dy, torch.zeros((), dtype=torch.float64, device=dev)).t().contiguous()
            for tap in range(9):
                out[:, tap] += a @ patch[:, (q >> 1) + tap // 3, (q & 1) + tap % 3, :]
    return out.reshape(M, 9 * Cin)


def grouped_ref(gwm, ywm, goff):
    """Grouped product, one group at a time: yields (g, gwm[g0:g1]^T ywm[g0:g1]) - the columns g * N .. of the output."""
    off = [int(v) for v in torch.as_tensor(goff).cpu()]
    for g in range(len(off) - 1):
        yield g, tn_ref(gwm[off[g]:off[g + 1]], ywm[off[g]:off[g + 1]])


def expected_slabs(nk, splits, tiles, sparse=False):
    """*n_slabs of the launchers: ceil(nk / ceil(nk / min(max(splits, 1), nk))); splits <= 0 mirrors tn_auto_splits (the smallest count that
    fills 256 CUs in whole waves of blocks to >= 95 % while leaving >= 8 K tiles per block); the sparse block with splits == -1 takes 32 K
    ranges from 2048 K tiles on."""
    if sparse and splits == -1 and nk >= 2048:
        splits = 32
    if splits <= 0:
        best = 1
        for s in range(1, 65):
            if s > 1 and nk // s < 8:
                break
            blocks = tiles * s
            waves = (blocks + 255) // 256
            best = s
            if blocks >= 256 and blocks * 100 >= waves * 256 * 95:
                break
        splits = best
    s = min(max(splits, 1), nk)
    per = -(-nk // s)
    return -(-nk // per)


# ------------------------------------------------------------------------------------------------------------------ operands
def _real(shape, seed, scale, sparsity=0.0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g) * scale
    if sparsity:
        t = t * (torch.rand(shape, generator=g) >= sparsity)
    return t


def _vals(regime, shape, seed, density=0.5, signed=True, scale=0.5):
    if regime == "exact":
        return C.exact_operands(shape, (-3, -2, -1, 1, 2, 3) if signed else (1, 2, 3), density, 1.0, seed)
    return _real(shape, seed, scale, 1.0 - density)


def plain_case(regime, K, M, N, dtype, seed, device="cpu"):
    """A [K][M], B [K][N] of ``dtype``."""
    return _vals(regime, (K, M), seed).to(dtype).to(device), _vals(regime, (K, N), seed + 1).to(dtype).to(device)


def conv_case(regime, n, lgS, Cin, M, seed, device="cpu"):
    """dy_pad [n][S+2][S+2][M] bf16 with a NaN ring, x_pad [n][S+2][S+2][Cin] bf16 with the zero ring of the padding."""
    S = 1 << lgS
    dy = torch.full((n, S + 2, S + 2, M), float("nan"), dtype=torch.bfloat16)
    dy[:, 1:S + 1, 1:S + 1] = _vals(regime, (n, S, S, M), seed, 0.4).to(torch.bfloat16)
    x = torch.zeros(n, S + 2, S + 2, Cin, dtype=torch.bfloat16)
    x[:, 1:S + 1, 1:S + 1] = _vals(regime, (n, S, S, Cin), seed + 1, 0.6, signed=False).to(torch.bfloat16)
    return dy.to(device), x.to(device)


def centre_rows(t_pad, lgS):
    """The centre pixels of padded maps [n][S+2][S+2][C] as window-major rows [n*S*S][C]."""
    S = 1 << lgS
    yy, xx = C.window_major(S)
    return t_pad[:, (yy + 1).to(t_pad.device), (xx + 1).to(t_pad.device), :].reshape(-1, t_pad.shape[3]).contiguous()


F16_TIES = (259, 261, 263, 518, 2047)        # f16 integers bf16 cannot hold (ties included): 260, 260, 264, 520, 2048 in bf16


def codes(shape, seed):
    """Routing bytes: 0..4 uniformly, one byte in 64 above 4 (5, 7, 255)."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(0, 5, shape, generator=g, dtype=torch.uint8)
    hi = torch.tensor([5, 7, 255], dtype=torch.uint8)[torch.randint(0, 3, shape, generator=g)]
    return torch.where(torch.rand(shape, generator=g) < 1.0 / 64, hi, c)


def list_case(regime, n_entries, seed, device="cpu", n_maps=6, n_rows=40, z_dtype=torch.bfloat16, z_values=None):
    """A window list and its operands: dy_rows [n_rows][1024] bf16 (pooled gradient rows, row dest[e]), code_rows [n_maps*64][1024] routing
    bytes (row gather[e]), z_pad [n_maps][18][18][512] of ``z_dtype`` with a zero ring, gather / dest int32 [n_entries].
    The list is unsorted, has duplicates and holds windows 0, 7, 56, 63 (the map's corners) of the first and the last map; gather[8] is a
    window whose codes are all 4 (its gradient row is non-zero and must be dropped), gather[9] one whose codes are all 3."""
    g = torch.Generator().manual_seed(seed)
    E = n_entries
    gather = torch.randint(0, n_maps * 64, (E,), generator=g, dtype=torch.int32)
    last = (n_maps - 1) * 64
    gather[:8] = torch.tensor([last + 63, 7, last, 56, 0, last + 7, 63, last + 56], dtype=torch.int32)
    dead, three = 64 + 9, 64 + 10
    gather[8], gather[9], gather[10], gather[11] = dead, three, last + 63, 7
    dest = torch.randint(0, n_rows, (E,), generator=g, dtype=torch.int32)
    dest[12] = dest[3]
    dy = _vals(regime, (n_rows, M3), seed + 1, 0.5).to(torch.bfloat16)
    code = codes((n_maps * 64, M3), seed + 2)
    code[dead] = 4
    code[three] = 3
    assert bool((dy[dest[8].item()] != 0).any())
    z = torch.zeros(n_maps, 18, 18, CIN3, dtype=z_dtype)
    if z_values is not None:
        z[:, 1:17, 1:17] = C.exact_operands((n_maps, 16, 16, CIN3), z_values, 0.5, 1.0, seed + 3).to(z_dtype)
    else:
        z[:, 1:17, 1:17] = _vals(regime, (n_maps, 16, 16, CIN3), seed + 3, 0.5, signed=False).to(z_dtype)
    return dict(dy=dy.to(device), code=code.to(device), z=z.to(device), gather=gather.to(device), dest=dest.to(device))


def list_mag(c):
    """Magnitude sums of a list case's products (``mag`` of assert_exact / acc_bound)."""
    return list_wgrad_ref(c["dy"].abs(), c["code"], c["gather"], c["dest"], c["z"].abs())


def zcol_rows(gather, z_pad):
    """The im2col rows [4E][9*Cin] of the listed windows: row 4e + q, columns (tap, c) = the map at the pixel of q shifted by the tap."""
    p = list_patches(gather, z_pad)
    E, Cin = p.shape[0], p.shape[3]
    out = torch.empty(E, 4, 9, Cin, dtype=p.dtype, device=p.device)
    for q in range(4):
        for tap in range(9):
            out[:, q, tap] = p[:, (q >> 1) + tap // 3, (q & 1) + tap % 3]
    return out.reshape(4 * E, 9 * Cin)


GROUP_CYCLE = (0, 64, 128, 192, 320)


def group_sizes():
    """64 group sizes cycling through GROUP_CYCLE with group 0 and group 63 empty."""
    s = [GROUP_CYCLE[g % 5] for g in range(64)]
    s[0] = s[63] = 0
    return s


def grouped_case(regime, seed, device="cpu", n_src=300):
    """The grouped fc1 weight gradient: gsrc [n_src][4096] bf16, rowsrc [rows] (the row table: unsorted, with repeats), gwm = gsrc[rowsrc],
    ywm [rows][1024] bf16, goff [65]."""
    sizes = group_sizes()
    goff = torch.tensor([0] + list(torch.tensor(sizes).cumsum(0)), dtype=torch.int32)
    rows = int(goff[64])
    g = torch.Generator().manual_seed(seed)
    rowsrc = torch.randint(0, n_src, (rows,), generator=g, dtype=torch.int32)
    gsrc = _vals(regime, (n_src, 4096), seed + 1, 0.5).to(torch.bfloat16).to(device)
    ywm = _vals(regime, (rows, 1024), seed + 2, 0.5).to(torch.bfloat16).to(device)
    rowsrc = rowsrc.to(device)
    return dict(gsrc=gsrc, rowsrc=rowsrc, gwm=gsrc[rowsrc.long()].contiguous(), ywm=ywm, goff=goff.to(device), rows=rows)


def long_list_case(n_entries, seed, device="cpu", n_maps=24, n_rows=300):
    """EXACT operands of the long-K cases: a long list over few rows and maps, f16 maps of bf16-exact integers.  Every product is at most
    3 * 3, so n_entries * 9 < 2**24 is the exactness precondition (``long_exact``)."""
    g = torch.Generator().manual_seed(seed)
    gather = torch.randint(0, n_maps * 64, (n_entries,), generator=g, dtype=torch.int32)
    dest = torch.randint(0, n_rows, (n_entries,), generator=g, dtype=torch.int32)
    dy = C.exact_operands((n_rows, M3), (-3, -2, -1, 1, 2, 3), 0.5, 1.0, seed + 1).to(torch.bfloat16)
    code = codes((n_maps * 64, M3), seed + 2)
    z = torch.zeros(n_maps, 18, 18, CIN3, dtype=torch.float16)
    z[:, 1:17, 1:17] = C.exact_operands((n_maps, 16, 16, CIN3), (1, 2, 3), 0.5, 1.0, seed + 3).half()
    return dict(dy=dy.to(device), code=code.to(device), z=z.to(device), gather=gather.to(device), dest=dest.to(device))


def long_exact(c, n_terms):
    """``assert_exact`` of a long-K case with the magnitude sum by formula: every output element is a sum of at most n_terms products
    (one per entry: the routing byte keeps one pixel of a window), each at most max|dy| * max|z|."""
    top = n_terms * float(c["dy"].double().abs().max()) * float(c["z"].double().abs().max())
    C.assert_exact(c["dy"], c["z"], mag=torch.tensor([top], dtype=torch.float64))


def conv3_pairs_case(regime, n_pairs, seed, device="cpu"):
    """The conv3 weight gradient over whole maps: pooled gradient dy [P*64][1024] bf16, routing bytes [P*64][1024], z_pad [P][18][18][512]
    bf16 - a list case whose list is the identity."""
    E = n_pairs * 64
    dy = _vals(regime, (E, M3), seed, 0.5).to(torch.bfloat16)
    code = codes((E, M3), seed + 1)
    code[E // 2] = 4
    code[E // 2 + 1] = 3
    z = torch.zeros(n_pairs, 18, 18, CIN3, dtype=torch.bfloat16)
    z[:, 1:17, 1:17] = _vals(regime, (n_pairs, 16, 16, CIN3), seed + 2, 0.5, signed=False).to(torch.bfloat16)
    ident = torch.arange(E, dtype=torch.int32)
    return dict(dy=dy.to(device), code=code.to(device), z=z.to(device), gather=ident.to(device), dest=ident.clone().to(device))


def unpooled_pad(c, ring=float("nan")):
    """dy3_pad [P][18][18][1024] bf16 of a conv3_pairs_case: the un-pooled gradient at the centre pixels, ``ring`` around them."""
    P = c["z"].shape[0]
    rows = unpool_rows(c["dy"], c["code"])                                       # window-major [P*256][1024]
    out = torch.full((P, 18, 18, M3), ring, dtype=torch.bfloat16, device=rows.device)
    yy, xx = C.window_major(16)
    out[:, (yy + 1).to(rows.device), (xx + 1).to(rows.device), :] = rows.view(P, 256, M3)
    return out


# ------------------------------------------------------------------------------------------------------------------ the cases
# (M, N, K, splits) of sgc_dbg_gemm_tn; which block and walk each reaches: see the head of tests/test_tn_blocks_gpu.py
PLAIN_STRIDED = [(128, 384, 64, 1), (128, 384, 320, 2), (128, 384, 320, 4), (128, 384, 320, 9)]
PLAIN_SIZE_RULE = [(256, N, K, 1) for N in (768, 1024) for K in (64, 128, 192, 320)]
PLAIN_WALK = [(2048, 256, 192, 1), (4096, 2560, 192, 1)]
CONV_DBG = [(1, 4, 128, 128, 1), (2, 5, 128, 256, 2)]                  # (n_img, lgS, Cin, M, splits)
CONV1 = [(384, 1024, 16), (384, 1024, 3)]                              # (XC, n_rows, splits)
FC2 = [(64, 32), (320, 32), (320, 2)]                                  # (n_rows, splits)
FC1 = [(192, 512), (192, 2560)]                                        # (n_rows, columns)
CONV2 = [(1, 0), (1, 5), (3, 0), (3, 5)]                               # (n_obj, splits)
CONV3 = [(1, 1), (2, 0), (5, 3)]                                       # (n_pairs, splits)
LIST_ROWS = [64, 192, 320]                                             # dense list forms: rows = 4 * entries
SPARSE_ENTRIES = [(16, 1), (32, 2), (48, 1), (80, 2)]                  # (n_entries, splits)
LONG_ENTRIES = [32752, 32768, 32848]                                   # splits = -1: below the threshold, 32 x 64 K tiles, 31 x 65 + 38
LONG_PAIRS = 512
