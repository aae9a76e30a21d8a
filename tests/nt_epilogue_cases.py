"""Float64 references and operand generators for the direct tests of the fused NT GEMM epilogues (tests/test_nt_epilogues_gpu.py;
self-test: tests/test_nt_epilogue_cases_cpu.py).  Plain torch, no project kernel: on the device a float64 matmul is the BLAS library's.

Two data regimes:

* EXACT.  Operands are small integers times a power of two (``exact_operands``).  When ``assert_exact`` holds - the sum of the
  magnitudes of all products of an output element, plus whatever is added to it, stays below 2**24 units - every partial sum, in any
  order and with any grouping inside the matrix instruction, is an integer number of units below 2**24 and therefore an f32 value:
  the kernel's f32 accumulator EQUALS the float64 result and the outputs can be compared bit for bit.  That is a precondition, not
  a tolerance: every exact test calls ``assert_exact`` on its own operands.
* REAL.  Seeded reals rounded to the operand type; the reference is the float64 result of the rounded operands and the bound per
  element is ``u * |ref| + acc_bound`` (u = half an ulp of the output type)."""
import torch


def window_major(S):
    """Row m = 4 * (py * (S/2) + px) + (dy * 2 + dx) of an S x S map -> pixel (y, x) = (2 py + dy, 2 px + dx); two int64 tensors [S*S]
    (csrc/gemm_nt.h, conv_row_base)."""
    m = torch.arange(S * S)
    W, q = m // 4, m % 4
    py, px = W // (S // 2), W % (S // 2)
    return 2 * py + q // 2, 2 * px + q % 2


def conv3x3_rows(xp, w_k_order, lgS, windows=None):
    """The implicit 3x3 convolution of the NT family as nine shifted float64 matmuls.

    xp [n][S+2][S+2][Cin]: zero-padded channels-last maps (any dtype, any device); w_k_order [N][9*Cin] with K = (64-channel chunk, tap,
    channel).  Returns float64 [rows][N] on xp's device: all n*S*S pixels in window-major order, or with ``windows`` (a list / tensor of
    map * (S/2)^2 + window) the rows 4e + q of the listed 2x2 windows."""
    S = 1 << lgS
    n, Cin = xp.shape[0], xp.shape[3]
    N = w_k_order.shape[0]
    dev = xp.device
    w = w_k_order.to(dev).double().view(N, Cin // 64, 9, 64)
    yy, xx = window_major(S)
    if windows is None:
        img = torch.arange(n).repeat_interleave(S * S)
        y, x = yy.repeat(n), xx.repeat(n)
    else:
        g = torch.as_tensor(windows, dtype=torch.int64).cpu()
        wpm = (S // 2) ** 2
        rows = ((g % wpm) * 4).repeat_interleave(4) + torch.arange(4).repeat(g.numel())
        img = (g // wpm).repeat_interleave(4)
        y, x = yy[rows], xx[rows]
    img, y, x = img.to(dev), y.to(dev), x.to(dev)
    out = torch.zeros(img.numel(), N, dtype=torch.float64, device=dev)
    for tap in range(9):
        ky, kx = tap // 3, tap % 3
        a = xp[img, y + ky, x + kx, :].double()                          # [rows][Cin]
        out += a @ w[:, :, tap, :].reshape(N, Cin).t()
    return out


def pool_ref(pre, bias):
    """Bias + ReLU + 2x2 max-pool + routing code as nt_epilogue / nt_epilogue_pool16 state it.  pre [4*W][N] float64 (rows 4w + q),
    bias [N] or None.  Per window and column: the FIRST position of the maximum of the four pre-activations, + bias; when the result
    is not > 0 the value is 0 and the code is 4.  Returns (value float64 [W][N], code uint8 [W][N])."""
    p = pre.view(-1, 4, pre.shape[1])
    v = p[:, 0].clone()
    am = torch.zeros_like(v, dtype=torch.uint8)
    for q in range(1, 4):
        t = p[:, q]
        up = t > v
        v = torch.where(up, t, v)
        am = torch.where(up, torch.full_like(am, q), am)
    if bias is not None:
        v = v + bias.to(v.device).double()
    dead = ~(v > 0)
    v = torch.where(dead, torch.zeros_like(v), v)
    am = torch.where(dead, torch.full_like(am, 4), am)
    return v, am


def exact_operands(shape, values, density, scale, seed, device="cpu"):
    """float64 tensor: with probability ``density`` an entry is ``scale`` (a power of two) times an integer drawn uniformly from
    ``values``, else 0.  Seeded; drawn on the CPU unless ``device`` is given (the large fc1 operands), then with that device's generator."""
    g = torch.Generator(device=device).manual_seed(seed)
    vals = torch.tensor(list(values), dtype=torch.float64, device=device)
    pick = torch.randint(0, len(values), shape, generator=g, device=device)
    keep = torch.rand(shape, generator=g, device=device) < density
    return torch.where(keep, vals[pick], torch.zeros((), dtype=torch.float64, device=device)) * scale


def assert_exact(A, B, extras=None, scale_A=1.0, scale_B=1.0, mag=None):
    """Precondition of bit equality: A / scale_A, B / scale_B and extras / (scale_A scale_B) are integers and
    (|A| @ |B|^T + |extras|).max() < 2**24 * scale_A * scale_B.  ``mag`` replaces |A| @ |B|^T where the product is not a plain
    matmul (the implicit convolution: conv3x3_rows of the absolute values).  Raises AssertionError otherwise."""
    unit = scale_A * scale_B
    for t, s in ((A, scale_A), (B, scale_B), (extras, unit)):
        if t is not None:
            q = t.double() / s
            assert bool((q == q.round()).all()), "operand is not an integer multiple of its scale"
    if mag is None:
        mag = A.double().abs() @ B.double().abs().t()
    if extras is not None:
        mag = mag + extras.double().abs().to(mag.device)
    top = float(mag.max())
    assert top < 2.0 ** 24 * unit, "exactness precondition violated: %.6g >= 2**24 * %g" % (top, unit)


def acc_bound(A, B, K, mag=None):
    """Worst-case error of a K-term f32 sum, per element: K * 2**-24 relative to the sum of the products' magnitudes, doubled because
    the order inside the instruction's 32 products is unspecified: K * 2**-23 * (|A| @ |B|^T).  Derived, not measured.  ``mag`` as in
    assert_exact."""
    if mag is None:
        mag = A.double().abs() @ B.double().abs().t()
    return K * 2.0 ** -23 * mag
