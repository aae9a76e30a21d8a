"""The float64 references of tests/nt_epilogue_cases.py against torch's own convolution and pooling, on the CPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import nt_epilogue_cases as C


def test_window_major_is_conv_row_base():
    """csrc/gemm_nt.h, conv_row_base: row m of an S x S map -> W = m >> 2, q = m & 3, py = W >> (lgS - 1), px = W & (S/2 - 1),
    y = 2 py + (q >> 1), x = 2 px + (q & 1); and the copy in tests/test_gemm_gpu.py says the same."""
    from tests.test_gemm_gpu import _window_major_index
    for lgS in (1, 2, 4, 5):
        S = 1 << lgS
        yy, xx = C.window_major(S)
        for m in range(S * S):
            W, q = m >> 2, m & 3
            py, px = W >> (lgS - 1), W & ((S >> 1) - 1)
            assert (int(yy[m]), int(xx[m])) == (2 * py + (q >> 1), 2 * px + (q & 1))
        y2, x2 = _window_major_index(S)
        assert torch.equal(yy, y2) and torch.equal(xx, x2)
        assert sorted((int(a) * S + int(b)) for a, b in zip(yy, xx)) == list(range(S * S))          # a permutation of the pixels


def _case(seed=5, n=2, S=16, Cin=64, N=32):
    x = C.exact_operands((n, Cin, S, S), (0, 0, 1, 2, 3), 0.6, 1.0, seed)                   # NCHW, integer data: ties are frequent
    w = C.exact_operands((N, Cin, 3, 3), (-2, -1, 1, 2), 0.5, 1.0, seed + 1)
    bias = C.exact_operands((N,), range(-40, 41), 1.0, 1.0, seed + 2)
    xp = torch.zeros(n, S + 2, S + 2, Cin, dtype=torch.float64)
    xp[:, 1:-1, 1:-1, :] = x.permute(0, 2, 3, 1)
    w_k = w.reshape(N, Cin // 64, 64, 9).permute(0, 1, 3, 2).reshape(N, 9 * Cin)              # K = (c / 64, tap, c % 64)
    return x, w, bias, xp, w_k


def test_conv_and_pool_reference_equal_torch():
    n, S, N = 2, 16, 32
    x, w, bias, xp, w_k = _case()
    pre = C.conv3x3_rows(xp, w_k, 4)
    conv = F.conv2d(x, w, None, padding=1)                                                  # [n][N][S][S], integers: exact in float64
    yy, xx = C.window_major(S)
    assert torch.equal(pre, conv[:, :, yy, xx].permute(0, 2, 1).reshape(n * S * S, N))
    val, code = C.pool_ref(pre, bias)
    pooled, idx = F.max_pool2d(torch.relu(conv + bias.view(1, N, 1, 1)), 2, return_indices=True)      # [n][N][8][8]
    assert torch.equal(val, pooled.permute(0, 2, 3, 1).reshape(n * 64, N))
    # routing: torch's flat index y * S + x -> position inside the window; compared where the maximum is unique and alive
    iy, ix = idx // S, idx % S
    pos = ((iy % 2) * 2 + ix % 2).permute(0, 2, 3, 1).reshape(n * 64, N)
    p4 = pre.view(n * 64, 4, N)
    m = p4.max(1).values
    ties = (p4 == m.unsqueeze(1)).sum(1)
    alive = (m + bias) > 0
    assert bool((ties > 1).any()) and bool((~alive).any()) and bool(((m + bias) == 0).any())
    assert torch.equal(code[alive & (ties == 1)].long(), pos[alive & (ties == 1)])
    assert bool((code[~alive] == 4).all()) and bool((val[~alive] == 0).all())
    first = (p4 == m.unsqueeze(1)).to(torch.uint8).argmax(1)                                 # first position of the maximum
    assert torch.equal(code[alive].long(), first[alive])
    # the listed form returns the same rows
    wins = [0, 5, 63, 64, 100, 127]
    rows = torch.tensor([4 * g + q for g in wins for q in range(4)])
    assert torch.equal(C.conv3x3_rows(xp, w_k, 4, windows=wins), pre[rows])


def test_assert_exact_and_acc_bound():
    A = C.exact_operands((8, 64), (1, 2, 3), 0.5, 0.25, 1)
    B = C.exact_operands((16, 64), (-2, -1, 1, 2), 1.0, 0.5, 2)
    C.assert_exact(A, B, None, 0.25, 0.5)
    assert set((A / 0.25).unique().tolist()) <= {0.0, 1.0, 2.0, 3.0}
    with pytest.raises(AssertionError):                       # 4 products of 2**11 * 2**11: at the limit, not below it
        C.assert_exact(torch.full((1, 4), 2048.0), torch.full((1, 4), 2048.0))
    C.assert_exact(torch.full((1, 3), 2048.0), torch.full((1, 3), 2048.0))
    with pytest.raises(AssertionError):                       # what is added afterwards counts
        C.assert_exact(torch.full((1, 3), 2048.0), torch.full((1, 3), 2048.0), torch.tensor([[float(2 ** 22)]]))
    with pytest.raises(AssertionError):                       # not a multiple of the scale
        C.assert_exact(torch.tensor([[0.5]]), torch.tensor([[1.0]]))
    b = C.acc_bound(A, B, 64)
    assert torch.equal(b, 64 * 2.0 ** -23 * (A.abs() @ B.abs().t()))
