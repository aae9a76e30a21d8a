"""Cases and the float64 definitional reference of the fused attention operator (``sgc_mha_fwd`` / ``attention.fused_mha``).

The reference is the definition written out: explicit scores, masked fill, softmax and ``P V`` in float64, image by image.  A query
without an unmasked key gets zeros (the operator's documented difference from ``nn.MultiheadAttention``, which gives NaN).
``tests/test_attention_cpu.py`` pins it to ``nn.MultiheadAttention`` in float64."""
import math
from collections import namedtuple

import torch

HEAD_DIM = 32
KEY_TILE = 64                      # keys per tile of the kernel (csrc/kernels_attn.hip ATT_KT): the "entirely masked tile" hazards

Case = namedtuple("Case", "name B H Lq Lk mask gain")


def _c(name, B, H, Lq, Lk, mask="none", gain=1.0):
    return Case(name, B, H, Lq, Lk, mask, gain)


# every random case keeps at least one unmasked key per image
RANDOM_CASES = [
    _c("one", 1, 1, 1, 1),
    _c("odd_17x33", 2, 8, 17, 33),
    _c("ragged_63x127", 3, 2, 63, 127, "ragged"),
    _c("ragged_64x128", 3, 2, 64, 128, "ragged"),
    _c("ragged_65x129", 3, 2, 65, 129, "ragged"),
    _c("queries_100x100", 2, 8, 100, 100),
    _c("cross_100x1024", 2, 8, 100, 1024, "cross"),
    _c("detr_rect_1024", 1, 8, 1024, 1024, "rect"),
]
FULL_CASE = _c("full_8x8x1024", 8, 8, 1024, 1024)          # smoke only
HAZARD_CASES = [
    _c("first_tile_masked", 2, 2, 33, 200, "first_tile"),
    _c("middle_tile_masked", 2, 2, 33, 200, "middle_tile"),
    _c("large_scores", 2, 4, 65, 300, "ragged", 6.0),
]
ALL_MASKED_CASE = _c("one_image_all_masked", 3, 2, 40, 150, "image1_all")
NO_KEYS_CASE = _c("no_keys", 2, 2, 19, 0)
BY_NAME = {c.name: c for c in RANDOM_CASES + HAZARD_CASES + [FULL_CASE, ALL_MASKED_CASE, NO_KEYS_CASE]}


def make_mask(case):
    """bool [B, Lk], True = key excluded; None for an unmasked case."""
    B, Lk = case.B, case.Lk
    if case.mask == "none":
        return None
    m = torch.zeros(B, Lk, dtype=torch.bool)
    if case.mask == "ragged":                              # tails that differ per image: 1, 40, 79, ... masked keys at the end
        for b in range(B):
            m[b, Lk - (1 + 39 * b):] = True
    elif case.mask == "cross":
        m[0, :64] = True
        m[0, 70::3] = True
        m[1, Lk // 2:] = True
    elif case.mask == "rect":                              # 20 x 27 valid cells of a 32 x 32 grid, flattened (DETR's padding mask)
        g = torch.ones(B, 32, 32, dtype=torch.bool)
        g[:, :20, :27] = False
        m = g.flatten(1)
    elif case.mask == "first_tile":
        m[:, :KEY_TILE] = True
    elif case.mask == "middle_tile":
        m[:, KEY_TILE:2 * KEY_TILE] = True
        m[1, 190:] = True
    elif case.mask == "image1_all":
        m[1, :] = True
        m[2, 100:] = True
    else:
        raise KeyError(case.mask)
    return m


def make_inputs(case, dtype, seed=0):
    """q [Lq, B, E], k, v [Lk, B, E] on the CPU, already ROUNDED to ``dtype`` (the reference is computed from the rounded values), and
    the mask."""
    gen = torch.Generator().manual_seed(1000 + seed)
    E = HEAD_DIM * case.H
    q = (torch.randn(case.Lq, case.B, E, generator=gen) * case.gain).to(dtype)
    k = (torch.randn(case.Lk, case.B, E, generator=gen) * case.gain).to(dtype)
    v = (torch.randn(case.Lk, case.B, E, generator=gen) * case.gain).to(dtype)
    return q, k, v, make_mask(case)


def reference(q, k, v, num_heads, key_padding_mask=None, scale=None):
    """The definition in float64 on the tensors' device: ``[Lq, B, E]`` float64."""
    scale = 1.0 / math.sqrt(HEAD_DIM) if scale is None else scale
    Lq, B, E = q.shape
    Lk = k.shape[0]
    out = torch.zeros(Lq, B, E, dtype=torch.float64, device=q.device)
    for b in range(B):
        qh = q[:, b].double().reshape(Lq, num_heads, HEAD_DIM).transpose(0, 1)          # [H, Lq, 32]
        kh = k[:, b].double().reshape(Lk, num_heads, HEAD_DIM).transpose(0, 1)
        vh = v[:, b].double().reshape(Lk, num_heads, HEAD_DIM).transpose(0, 1)
        s = torch.matmul(qh, kh.transpose(1, 2)) * scale                                # [H, Lq, Lk]
        if key_padding_mask is not None:
            s = s.masked_fill(key_padding_mask[b].bool().view(1, 1, Lk), float("-inf"))
        if Lk > 0:
            mx = s.amax(dim=-1, keepdim=True)
            p = torch.exp(s - torch.where(torch.isinf(mx), torch.zeros_like(mx), mx))   # all keys masked: exp(-inf) = 0 everywhere
            den = p.sum(dim=-1, keepdim=True)
            p = torch.where(den > 0, p / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(p))
            out[:, b] = torch.matmul(p, vh).transpose(0, 1).reshape(Lq, E)
    return out


def vmax(v):
    """max_j |v[j, b, h, d]| as float64 [B, E] (broadcasts against an output [Lq, B, E]); zeros without keys."""
    if v.shape[0] == 0:
        return torch.zeros(v.shape[1:], dtype=torch.float64, device=v.device)
    return v.double().abs().amax(dim=0)


UNIT = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}
