"""The NT GEMM family on v_mfma_f32_16x16x32_{f16,bf16} (csrc/gemm_nt.h, csrc/gemm_nt_pp.h): the register layout of the
instruction, the ping-pong block at the K sizes where its loop forms differ, and the property the bit-equality tests of the
suite rest on - a small problem (128x128 block) and a large one (ping-pong / halo block) give the same bits for the same
output element (the accumulation contract at the top of gemm_nt.h)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [(torch.float16, 0), (torch.bfloat16, 1)]
M_BIG, N = 16421, 1024          # 65 M tiles of the 256x256 block, the last one ragged (37 rows, clamped loads)


def _lib():
    from scene_graph_commonsense_amd import _lib
    return _lib.load(), _lib


def _rand(shape, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1).to(dtype)


@pytest.mark.parametrize("dtype,elem", DTYPES)
def test_mfma16_layout(dtype, elem):
    """One-hot operands: lane l supplies row / column l & 15 at k = 8 * (l >> 4) + j; register r of lane l is the element
    (row 4 * (l >> 4) + r, column l & 15).  A[m][k] = m + 1 where k == ka, B[n][k] = 1 where k == kb: the product is
    (m + 1) * [ka == kb] in every column, so the (lane, register) map of the rows is read off exactly; B[n][k] = n + 1 gives the columns."""
    lib, L = _lib()
    lane = torch.arange(64)
    for ka in (0, 9, 31):
        for kb in (ka, (ka + 8) % 32):
            for which in ("rows", "cols"):
                a = torch.zeros(16, 32)
                b = torch.zeros(16, 32)
                a[:, ka] = torch.arange(1, 17, dtype=torch.float32) if which == "rows" else 1.0
                b[:, kb] = torch.arange(1, 17, dtype=torch.float32) if which == "cols" else 1.0
                # operand registers: lane l holds [l & 15][8 * (l >> 4) .. + 7]
                pack = lambda t: t.view(16, 4, 8).permute(1, 0, 2).contiguous().to(dtype).cuda()
                av, bv = pack(a), pack(b)
                c = torch.full((64, 4), -1.0, dtype=torch.float32, device="cuda")
                assert lib.sgc_dbg_mfma16_probe(elem, L.ptr(av), L.ptr(bv), L.ptr(c), L.stream_ptr()) == 0
                torch.cuda.synchronize()
                got = c.cpu().to(torch.int64)
                row = (4 * (lane // 16)).view(64, 1) + torch.arange(4).view(1, 4)
                col = (lane % 16).view(64, 1).expand(64, 4)
                exp = ((row if which == "rows" else col) + 1) * int(ka == kb)
                assert torch.equal(got, exp), (ka, kb, which, got[:20].tolist())


_SHARED = {}      # (elem, K) -> device operands and output of the two K sizes that the bit-equality test reads again (about 70 MB each)


def _plain_case(elem, K):
    """Device operands and the kernel's output for M = 16 421 (ping-pong block)."""
    if (elem, K) in _SHARED:
        return _SHARED[(elem, K)]
    lib, L = _lib()
    dtype = DTYPES[elem][0]
    A, B = _rand((M_BIG, K), dtype, 11 + K), _rand((N, K), dtype, 12 + K)
    Ad, Bd = A.cuda(), B.cuda()
    C = torch.empty(M_BIG, N, dtype=dtype, device="cuda")
    st = lib.sgc_dbg_gemm_nt(elem, L.ptr(Ad), L.ptr(Bd), L.ptr(C), M_BIG, N, K, ctypes.c_long(K), ctypes.c_long(K),
                             ctypes.c_long(N), None, L.stream_ptr())
    assert st == 0
    torch.cuda.synchronize()
    if K in (192, 1024):
        _SHARED[(elem, K)] = (Ad, Bd, C)
    return Ad, Bd, C


@pytest.mark.parametrize("dtype,elem", DTYPES)
@pytest.mark.parametrize("K", [64, 128, 192, 1024])       # nk = 1: prologue only; 2, 3: the non-steady tiles; 16: the steady loop
def test_pingpong_block_against_float64(dtype, elem, K):
    A, B, C = _plain_case(elem, K)
    ref = A.cpu().double() @ B.cpu().double().t()          # float64 product of the rounded operands
    err = (C.cpu().double() - ref).abs().max().item()
    tol = (2e-3 if elem == 0 else 1.6e-2) * ref.abs().max().item()
    print("K=%d elem=%d max err %.3e (bound %.3e)" % (K, elem, err, tol))
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("dtype,elem", DTYPES)
@pytest.mark.parametrize("K", [192, 1024])
def test_small_block_equals_pingpong_block_bitwise(dtype, elem, K):
    lib, L = _lib()
    A, B, Cbig = _plain_case(elem, K)
    C = torch.empty(128, N, dtype=dtype, device="cuda")
    st = lib.sgc_dbg_gemm_nt(elem, L.ptr(A), L.ptr(B), L.ptr(C), 128, N, K, ctypes.c_long(K), ctypes.c_long(K),
                             ctypes.c_long(N), None, L.stream_ptr())
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(C, Cbig[:128])


@pytest.mark.parametrize("dtype,elem", DTYPES)
@pytest.mark.parametrize("Cin", [64, 128])
def test_small_block_equals_halo_block_bitwise(dtype, elem, Cin):
    """3x3 convolution on 16x16 maps: image 0 alone (M = 256: 128x128 block) against image 0 of 64 images (halo block)."""
    lib, L = _lib()
    n_img, S = 64, 16
    xp = torch.zeros(n_img, S + 2, S + 2, Cin, dtype=dtype)
    xp[:, 1:-1, 1:-1, :] = _rand((n_img, S, S, Cin), dtype, 21)
    xp = xp.cuda()
    w = (_rand((N, 9 * Cin), dtype, 22).float() * 0.1).to(dtype).cuda()
    bias = _rand((N,), torch.float32, 23).cuda()
    out = []
    for n in (1, n_img):
        C = torch.empty(n * S * S, N, dtype=dtype, device="cuda")
        assert lib.sgc_dbg_conv_nt(elem, L.ptr(xp), L.ptr(w), L.ptr(C), n, 4, Cin, N, L.ptr(bias), L.stream_ptr()) == 0
        out.append(C)
    torch.cuda.synchronize()
    assert out[0].abs().max().item() > 0
    assert torch.equal(out[0], out[1][:S * S])
