"""Fused head-dim-32 attention on the MI355X: ``sgc_mha_fwd`` against the float64 definition (tests/attention_cases.py) on every
case and dtype, its hazards and contract, ``attention.mha_forward`` against ``nn.MultiheadAttention``, and the opt-in route through
the DETR extractor (detr.py) against the default route."""
import ctypes
import functools

import pytest
import torch
from torch import nn

from tests import attention_cases as AC

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
_ids = lambda d: str(d).split(".")[-1]


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    """(q, k, v, mask) on the device, rounded to dtype, + the float64 reference from the rounded values + vmax.  Shared, never written."""
    c = AC.BY_NAME[name]
    q, k, v, mask = AC.make_inputs(c, dtype)
    q, k, v = q.cuda(), k.cuda(), v.cuda()
    mask = None if mask is None else mask.cuda()
    return c, q, k, v, mask, AC.reference(q, k, v, c.H, mask), AC.vmax(v)


def _torch_f32(q, k, v, H, mask):
    """torch's own f32 math on the device: softmax(q k^T * scale) v with the mask as -inf."""
    Lq, B, E = q.shape
    Lk = k.shape[0]
    sp = lambda t, L: t.reshape(L, B, H, AC.HEAD_DIM).permute(1, 2, 0, 3)          # [B, H, L, 32]
    s = torch.matmul(sp(q, Lq), sp(k, Lk).transpose(2, 3)) * (AC.HEAD_DIM ** -0.5)
    if mask is not None:
        s = s.masked_fill(mask.view(B, 1, 1, Lk), float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), sp(v, Lk)).permute(2, 0, 1, 3).reshape(Lq, B, E)


def _assert_within(tag, out, q, k, v, H, mask, ref, vm, images=None):
    """16-bit: |out - ref| <= 3 u vmax elementwise (rounding of P and of the output: u vmax each, one u of slack).  f32: the maximum
    error is at most 4 x that of torch's own f32 math against the same float64 result (only the summation order differs) plus
    4 * 2^-24 * vmax.  ``images`` restricts the comparison (torch gives NaN for an image without an unmasked key)."""
    dtype = out.dtype
    sel = slice(None) if images is None else images
    err = (out.double() - ref).abs()[:, sel]
    vm = vm[sel]
    if dtype == torch.float32:
        terr = (_torch_f32(q, k, v, H, mask).double() - ref).abs()[:, sel]
        bound = 4.0 * float(terr.max()) + 4.0 * 2.0 ** -24 * float(vm.max())
        print("%s f32: kernel max err %.3e, torch f32 max err %.3e, bound %.3e" % (tag, float(err.max()), float(terr.max()), bound))
        assert float(err.max()) <= bound, (tag, float(err.max()), float(terr.max()))
    else:
        u = AC.UNIT[dtype]
        worst = float((err / (u * vm).clamp_min(1e-300)).max())
        print("%s %s: max err = %.3f u vmax" % (tag, _ids(dtype), worst))
        assert bool((err <= 3.0 * u * vm).all()), (tag, worst)


def _check(name, dtype):
    from scene_graph_commonsense_amd.attention import fused_mha
    c, q, k, v, mask, ref, vm = _case(name, dtype)
    out = fused_mha(q, k, v, c.H, mask)
    assert out.shape == q.shape and out.dtype == dtype and out.is_contiguous()
    assert torch.isfinite(out).all()
    _assert_within(name, out, q, k, v, c.H, mask, ref, vm)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", [c.name for c in AC.RANDOM_CASES])
def test_kernel_against_float64(name, dtype):
    _check(name, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", [c.name for c in AC.HAZARD_CASES])
def test_hazard_cases(name, dtype):
    """A first / a middle key tile with every key masked; operands scaled by 6 (|score| ~ 180): the same bounds."""
    c, q, k = _case(name, dtype)[:3]
    if c.gain > 1:
        s = torch.einsum("lbhd,mbhd->bhlm", q.float().view(c.Lq, c.B, c.H, 32), k.float().view(c.Lk, c.B, c.H, 32)) * 32 ** -0.5
        assert float(s.abs().max()) > 120
    _check(name, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_image_with_every_key_masked_gives_exact_zeros(dtype):
    from scene_graph_commonsense_amd.attention import fused_mha
    c, q, k, v, mask, ref, vm = _case(AC.ALL_MASKED_CASE.name, dtype)
    out = fused_mha(q, k, v, c.H, mask)
    assert torch.isfinite(out).all()
    assert float(out[:, 1].abs().max()) == 0.0
    _assert_within(c.name, out, q, k, v, c.H, mask, ref, vm, images=[0, 2])
    assert float(out[:, 0].abs().max()) > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_no_keys_gives_zeros(dtype):
    from scene_graph_commonsense_amd.attention import fused_mha
    c, q, k, v, mask, ref, vm = _case(AC.NO_KEYS_CASE.name, dtype)
    out = fused_mha(q, k, v, c.H)
    assert out.shape == q.shape and float(out.abs().max()) == 0.0
    assert fused_mha(q[:0], k, v, c.H).shape == (0, c.B, 32 * c.H)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_strided_slices_are_read_in_place_and_give_the_same_bits(dtype):
    from scene_graph_commonsense_amd import attention
    torch.manual_seed(3)
    L, B, H = 77, 3, 4
    E = 32 * H
    qk = torch.randn(L, B, 2 * E, device="cuda").to(dtype)
    v3 = torch.randn(L, B, 3 * E, device="cuda").to(dtype)
    q, k, v = qk[..., :E], qk[..., E:], v3[..., 2 * E:]
    assert attention._kernel_view(q) is q and attention._kernel_view(k) is k and attention._kernel_view(v) is v
    mask = torch.zeros(B, L, dtype=torch.bool, device="cuda")
    mask[1, 50:] = True
    a = attention.fused_mha(q, k, v, H, mask)
    b = attention.fused_mha(q.contiguous(), k.contiguous(), v.contiguous(), H, mask)
    assert torch.equal(a, b)
    odd = torch.randn(L, B, E + 2, device="cuda").to(dtype)[..., 1:E + 1]          # misaligned view: copied once, not rejected
    assert attention._kernel_view(odd) is not odd
    assert torch.equal(attention.fused_mha(odd, k, v, H, mask), attention.fused_mha(odd.contiguous(), k, v, H, mask))
    _assert_within("strided", a, q, k, v, H, mask, AC.reference(q, k, v, H, mask), AC.vmax(v))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_two_calls_and_a_side_stream_give_identical_bits(dtype):
    from scene_graph_commonsense_amd.attention import fused_mha
    c, q, k, v, mask, ref, vm = _case("cross_100x1024", dtype)
    a = fused_mha(q, k, v, c.H, mask)
    b = fused_mha(q, k, v, c.H, mask)
    assert torch.equal(a, b)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        s = fused_mha(q, k, v, c.H, mask)
    side.synchronize()
    assert torch.equal(a, s)


def test_bad_arguments_return_err_arg_without_a_launch():
    from scene_graph_commonsense_amd import _lib, attention
    fn = attention._fn()
    L, B, H = 16, 2, 2
    E = 32 * H
    q = torch.randn(L, B, E, device="cuda", dtype=torch.float16)
    k, v = torch.randn_like(q), torch.randn_like(q)
    out = torch.full_like(q, 7.0)
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def call(qp=None, H_=H, sL=B * E, dtype=1, scale=0.25, Lq=L):
        return fn(qp or P(q), P(k), P(v), None, P(out), Lq, L, B, H_, sL, E, B * E, E, B * E, E, B * E, E, dtype, scale, None)
    assert call(qp=P(q, 4)) == 1                           # misaligned pointer
    assert call(sL=6) == 1                                 # stride 6
    assert call(dtype=7) == 1
    assert call(H_=0) == 1
    assert call(Lq=-1) == 1
    assert call(scale=float("nan")) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                        # nothing ran
    assert call(Lq=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, attention.fused_mha(q, k, v, H, scale=0.25))


def test_forward_only():
    from scene_graph_commonsense_amd.attention import fused_mha
    q = torch.randn(4, 1, 32, device="cuda", requires_grad=True)
    with pytest.raises(RuntimeError):
        fused_mha(q, q.detach(), q.detach(), 1)
    with torch.no_grad():
        assert fused_mha(q, q, q, 1).shape == (4, 1, 32)


def _module(seed):
    torch.manual_seed(seed)
    mha = nn.MultiheadAttention(256, 8).cuda().eval()
    with torch.no_grad():
        mha.in_proj_bias.normal_(std=0.5)
        mha.out_proj.bias.normal_(std=0.5)
    return mha


def test_mha_forward_self_attention_with_mask_matches_the_module():
    from scene_graph_commonsense_amd.attention import mha_forward
    mha = _module(5)
    before = {n: p.clone() for n, p in mha.named_parameters()}
    x, pos = torch.randn(90, 3, 256, device="cuda"), torch.randn(90, 3, 256, device="cuda")
    mask = torch.zeros(3, 90, dtype=torch.bool, device="cuda")
    mask[0, 70:] = True
    mask[2, :64] = True
    with torch.no_grad():
        qk = x + pos
        want = mha(qk, qk, value=x, key_padding_mask=mask)[0]
        got = mha_forward(mha, qk, qk, x, mask)
    assert torch.allclose(got, want, atol=1e-4, rtol=1e-4), float((got - want).abs().max())
    assert all(torch.equal(p, before[n]) for n, p in mha.named_parameters())


def test_mha_forward_cross_attention_matches_the_module():
    from scene_graph_commonsense_amd.attention import mha_forward
    mha = _module(6)
    qx, kx, vx = torch.randn(100, 2, 256, device="cuda"), torch.randn(80, 2, 256, device="cuda"), torch.randn(80, 2, 256, device="cuda")
    with torch.no_grad():
        want = mha(qx, kx, value=vx)[0]
        got = mha_forward(mha, qx, kx, vx)
    assert torch.allclose(got, want, atol=1e-4, rtol=1e-4), float((got - want).abs().max())


@functools.lru_cache(maxsize=None)
def _small_detr():
    from scene_graph_commonsense_amd.detr import DETR
    torch.manual_seed(11)
    model = DETR(blocks=(1, 1, 1, 1), enc=2, dec=2).cuda().eval()
    images = [torch.randn(3, 256, 320, device="cuda"), torch.randn(3, 192, 256, device="cuda")]      # unequal: the padding mask is real
    return model, images


def _count_calls(monkeypatch):
    from scene_graph_commonsense_amd import attention
    calls, real = [], attention.fused_mha

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(attention, "fused_mha", counted)
    return calls


def test_extractor_encode_fused_matches_unfused_f32(monkeypatch):
    model, images = _small_detr()
    calls = _count_calls(monkeypatch)
    plain = model.encode(images)
    assert not calls
    fused = model.encode(images, fused_attention=True)
    assert len(calls) == 2                                 # both encoder layers
    assert not any(l.fused_attention for l in model.transformer.encoder.layers)
    assert plain.shape == (2, 256, 8, 10) and torch.isfinite(fused).all()
    assert torch.allclose(fused, plain, atol=1e-4, rtol=1e-4), float((fused - plain).abs().max())


def test_extractor_forward_fused_matches_unfused_f32(monkeypatch):
    model, images = _small_detr()
    calls = _count_calls(monkeypatch)
    with torch.no_grad():
        plain = model(images)
        assert not calls
        model.set_fused_attention(True)
        try:
            fused = model(images)
        finally:
            model.set_fused_attention(False)
    assert len(calls) == 2 + 2 * 2                         # encoder self-, decoder self- and cross-attention of every layer
    for key in ("pred_logits", "pred_boxes"):
        assert torch.allclose(fused[key], plain[key], atol=1e-4, rtol=1e-4), (key, float((fused[key] - plain[key]).abs().max()))


def test_extractor_bf16_fused_is_as_close_to_f32_as_unfused_bf16(monkeypatch):
    model, images = _small_detr()
    calls = _count_calls(monkeypatch)
    ref = model.encode(images)
    half = model.encode(images, autocast=torch.bfloat16)
    fused = model.encode(images, autocast=torch.bfloat16, fused_attention=True)
    assert len(calls) == 2
    d_half = float((half - ref).norm() / ref.norm())
    d_fused = float((fused - ref).norm() / ref.norm())
    print("bf16 distance to the f32 route: unfused %.3e, fused %.3e" % (d_half, d_fused))
    assert d_fused < 5e-2, d_fused
    assert d_fused <= 1.5 * d_half, (d_fused, d_half)


def test_training_mode_with_dropout_takes_the_unfused_line(monkeypatch):
    from scene_graph_commonsense_amd import attention
    model, images = _small_detr()

    def boom(*a, **kw):
        raise AssertionError("the kernel was called with attention dropout active")
    monkeypatch.setattr(attention, "fused_mha", boom)
    model.set_fused_attention(True)
    model.train()
    try:
        assert model.transformer.encoder.layers[0].self_attn.dropout == 0.1
        with torch.no_grad():
            out = model(images)
        assert torch.isfinite(out["pred_logits"]).all()
    finally:
        model.eval()
        model.set_fused_attention(False)


def test_config_key_and_process_image_features(monkeypatch):
    from scene_graph_commonsense_amd import train_utils as TU
    from scene_graph_commonsense_amd.detr import build_detr101
    from scene_graph_commonsense_amd.synthetic import HeadConfig
    torch.manual_seed(0)
    args = HeadConfig().args()
    args["models"].update(num_img_feature=256, feature_size=32, feature_encoder_attention="fused")
    detr = build_detr101(args).cuda().eval()
    assert all(l.fused_attention for l in list(detr.transformer.encoder.layers) + list(detr.transformer.decoder.layers))
    calls = _count_calls(monkeypatch)
    images = [torch.randn(3, 1024, 1024, device="cuda") for _ in range(2)]
    with torch.no_grad():
        fused = TU.process_image_features(args, images, detr, "cuda:0")
        assert len(calls) == 6
        detr.set_fused_attention(False)
        plain = TU.process_image_features(args, images, detr, "cuda:0")
        assert len(calls) == 6
    assert tuple(fused.shape) == (2, 256, 32, 32)
    assert torch.allclose(fused, plain, atol=1e-4, rtol=1e-4), float((fused - plain).abs().max())


def test_full_shape_smoke_bf16():
    from scene_graph_commonsense_amd.attention import fused_mha
    c, q, k, v, mask, ref, vm = _case(AC.FULL_CASE.name, torch.bfloat16)
    out = fused_mha(q, k, v, c.H)
    assert torch.isfinite(out).all()
    assert bool(((out.double() - ref).abs() <= 3.0 * AC.UNIT[torch.bfloat16] * vm).all())
